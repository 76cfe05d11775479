"""staticsMod 1 on the CPU: the longdouble reference (tests/statics_nl_reference.py), the fp64 model of k_mean_pose_nl
(tests/statics_nl_device_model.py) and the case list (tests/statics_nl_cases.py) held to each other and to three anchors
that do not come from either:

  1. a closed form: one vertical cylinder and one point mass on a line pair in the vertical plane of the load -- buoyancy,
     weight and their moments written by hand from raft_member.py:838-1010, evaluated at the returned pose;
  2. F_env = 0 on a unit trimmed at x_ref returns x_ref, for staticsMod 0 and 1;
  3. the statics at a pose are what tests/test_geom_reference.py holds to the reference's recorded goldens (the same
     ``design_reference``: nothing to do here).

The live reference cannot run solveStatics here (its mooring library is not installed); DESIGN section 3.u-nl says so.
"""
import numpy as np
import pytest

from . import geom_reference as gr
from . import mean_pose_device_model as mp
from . import mooring_reference as mr
from . import statics_nl_cases as sc
from . import statics_nl_device_model as dm
from . import statics_nl_reference as nr
from .geom_cases import vcyl

NAMES = tuple(sc.cases())


def _firm(case, pose):
    st = case["stations"] if case["drho"] is None else nr.apply_drho(case["stations"], case["drho"])
    return gr.design_firmness(case["members"], st, case["caps"], np.asarray(pose, dtype=np.float64), case["rho"], case["g"])


def _worst(case, res, ref):
    ev = nr.evaluation_multiples(case, res)
    w = {k: float(v.max()) for k, v in ev.items()}
    w["pose"] = float(nr.convergence_excess(res["pose"], ref, mp.TOL).max())
    return w


@pytest.mark.parametrize("name", NAMES)
def test_case_is_firm_and_contracts(name):
    """The conditions on a case: no discontinuous decision differs between fp64 and longdouble at the root or at the model's
    pose, and the reference's own iteration contracts by rho_hat <= 0.5 (a case that fails is replaced, not excused)."""
    case, ref, m = sc.cases()[name], sc.reference(name), sc.model(name)
    print("%s: rho_hat %.3f, %d reference steps, %d model steps, pose %s" % (name, ref["rho_hat"], ref["iterations"], m["iterations"],
                                                                              np.array2string(m["pose"], precision=5)))
    assert m["flags"] == 0 and m["iterations"] <= mp.MAX_ITER
    assert _firm(case, ref["x"].astype(np.float64)) == []
    assert _firm(case, m["pose"]) == []
    assert 0.0 < ref["rho_hat"] <= 0.5
    assert len(case["members"]) <= 6


def test_gate_constant_is_the_measured_one():
    worst = {}
    for name in NAMES:
        w = _worst(sc.cases()[name], sc.model(name), sc.reference(name))
        print(name, {k: round(v, 3) for k, v in w.items()})
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
    top = max(worst.values())
    print("worst multiples of eps E over the cases:", worst)
    assert top <= nr.GATE_WORST_CPU
    assert nr.GATE == 2 ** int(np.ceil(np.log2(4 * nr.GATE_WORST_CPU)))
    assert top > nr.GATE_WORST_CPU / 2, "GATE_WORST_CPU is stale: measured %.3g" % top


@pytest.mark.parametrize("name", NAMES)
def test_model_within_both_gates(name):
    case, ref, m = sc.cases()[name], sc.reference(name), sc.model(name)
    for k, v in nr.evaluation_multiples(case, m).items():
        assert v.max() <= nr.GATE, (name, k, float(v.max()))
    assert nr.convergence_excess(m["pose"], ref, mp.TOL).max() <= nr.GATE, name
    # ... and the mooring outputs at the returned pose are the mooring model's there
    fl, C, F, T, J = mp.moor(case["lines"], m["pose"], case["depth"])
    assert fl == 0 and np.array_equal(C, m["C"]) and np.array_equal(F, m["F"])


SEEDED = (("frozen_hydrostatics", "straight columns"), ("frozen_hydrostatics", "pontoon that surfaces"),
          ("pm_arm_not_rotated", "two point masses"), ("drho_ignored", "ballast trim, no point mass"))


@pytest.mark.parametrize("seed,name", SEEDED)
def test_gates_reject_seeded_errors(seed, name):
    """hydrostatics frozen at x_ref (staticsMod 0 passed off as staticsMod 1), the point masses' arms not rotated, drho
    ignored: each is far outside at least one gate."""
    case, ref = sc.cases()[name], sc.reference(name)
    bad = dm.solve(case, seed=seed, max_iter=400)                 # (a wrong Jacobian contracts slowly: the cap is not the point here)
    assert bad["flags"] == 0, "the seeded solve must converge: the gates, not a flag, have to reject it"
    ev = {k: float(v.max()) for k, v in nr.evaluation_multiples(case, bad).items()}
    conv = float(nr.convergence_excess(bad["pose"], ref, mp.TOL).max())
    print(seed, name, ev, conv)
    assert conv > 1e3 * nr.GATE
    assert max(ev.values()) > 1e3 * nr.GATE


def test_mod1_root_is_not_the_mod0_root():
    """The two modes differ by many gates where a pontoon surfaces on the way: the data the device test asserts on."""
    name = "pontoon that surfaces"
    case, ref = sc.cases()[name], sc.reference(name)
    K_hs, F0 = sc.linear(name)
    lin = mp.solve(case["lines"], case["depth"], K_hs, F0, case["F_env"], case["x_ref"])
    assert lin["flags"] == 0
    assert nr.convergence_excess(lin["pose"], ref, mp.TOL).max() > 1e3 * nr.GATE
    assert abs(lin["pose"][4] - sc.model(name)["pose"][4]) > 1e-3     # rad of pitch


@pytest.mark.parametrize("name", ("straight columns", "ballast trim, no point mass", "non-zero x_ref"))
def test_unloaded_unit_trimmed_at_x_ref_stays_there(name):
    """Anchor 2.  The unit is trimmed at x_ref in all six components: F_extra takes -Y(x_ref) of the longdouble evaluation,
    rounded to fp64, so Y(x_ref) is one rounding of E_F.  Both modes must return x_ref within the convergence gate taken
    about x_ref (with rho_hat = 0.5, the largest a case may have), in at most three steps."""
    case = sc.unloaded(name)
    y0 = nr.evaluate(case, case["x_ref"])["Y"]
    case["F_extra"] = ((0 if case["F_extra"] is None else case["F_extra"]) - y0).astype(np.float64)
    at = nr.evaluate(case, case["x_ref"])
    Kinv = np.abs(np.linalg.inv(at["K"].astype(np.float64)))
    about = dict(x=case["x_ref"].astype(np.longdouble), rho_hat=0.5, bound=Kinv @ at["E_F"])
    one = dm.solve(case)
    K_hs, F0 = dm.hydrostatics(case, case["x_ref"])
    zero = mp.solve(case["lines"], case["depth"], K_hs, F0, case["F_env"], case["x_ref"])
    for what, res in (("staticsMod 1", one), ("staticsMod 0", zero)):
        assert res["flags"] == 0, what
        ex = nr.convergence_excess(res["pose"], about, mp.TOL)
        print(what, res["pose"], res["iterations"], ex)
        assert ex.max() <= nr.GATE, what
        assert res["iterations"] <= 3, what


def test_c3_variants_that_do_not_settle():
    """The iteration of staticsMod 1 is not contracting on every unit: on variant 0 of the C3 sweep sway, roll and yaw grow
    from rounding until the step caps bind, and the fp64 model ends at the step cap; variant 1 settles.
    The device test asserts the same outcomes on the kernel, so a kernel that stops converging cannot hide behind this."""
    stuck, fine = dm.solve(sc.c3_variant(0)), dm.solve(sc.c3_variant(1))
    print("variant 0: flags %d after %d steps; variant 1: flags %d after %d steps, pose %s"
          % (stuck["flags"], stuck["iterations"], fine["flags"], fine["iterations"], fine["pose"]))
    assert stuck["flags"] == mp.FLAG_POSE_CAP and stuck["iterations"] == mp.MAX_ITER
    assert fine["flags"] == 0 and fine["iterations"] <= 20


def test_closed_form_cylinder_with_a_point_mass():
    """Anchor 1.  A buoy -- one vertical cylinder of diameter d from z = -D to z = +h, a point mass hung on its axis below the
    keel (the moment the reference procedure gives an inclined cylinder, M below, leaves a spar ballasted inside it
    unstable) -- on two
    lines in the x-z plane, under a thrust in x and its moment about y: the motion stays in that plane (surge xs, heave zs,
    pitch th).  With a = d / 2, the axis q = (sin th, 0, cos th), the bottom end at rA = (xs - D sin th, zs - D cos th):
        wet length     l  = (D cos th - zs) / cos th                                   raft_member.py:915
        buoyancy       B  = rho g pi a^2 l
        its moment about the bottom end (sic, :921)   M = -rho g pi (d^2 / 32 (2 + tan^2 th) + l^2 / 2) sin th
        about the PRP                                 M + D sin th B
        shell mass     ms = rho_shell pi / 4 (d^2 - (d - 2 t)^2) (D + h), at z_c = (h - D) / 2 on the axis
        weights' moment about the PRP                 (ms z_c + mp z_p) g sin th
    Heave and pitch equilibrium, with the lines' F_z and M_y from the mooring reference at the returned pose, must hold to
    1e-9 of the buoyancy (times the hub height for the moment): the step tolerance 1e-9 m through a stiffness of 1e6 N/m."""
    d, D, h, t, zp = 20.0, 20.0, 10.0, 0.05, -45.0
    deck = [vcyl(-D, h, d=d, dls=5.0)]
    lines, depth = sc.deck_lines(3)
    pair = lines[:2].copy()                                       # two lines, put into the x-z plane up- and downwind
    for i, sgn in enumerate((-1.0, 1.0)):
        r_anchor, r_fair = np.hypot(*lines[i, 0:2]), 12.0
        pair[i, 0:3] = [sgn * r_anchor, 0.0, lines[i, 2]]
        pair[i, 3:6] = [sgn * r_fair, 0.0, -14.0]
    case = sc._case(deck)
    case.update(lines=np.ascontiguousarray(pair), F_env=sc.thrust(0.5e6))
    # the point mass: the heave balance at rest, on the axis at zp (this replaces the trim mass _case put at PM_Z)
    rho_shell = float(case["members"][0][gr.GM_RHOSHELL])
    a = d / 2
    ms = rho_shell * np.pi / 4 * (d * d - (d - 2 * t) ** 2) * (D + h)
    Fz0 = float(mr.evaluate(pair[None], np.zeros((1, 6)), depth)["F"][0, 2])
    mpm = (sc.RHO * sc.GRAV * np.pi * a * a * D + Fz0) / sc.GRAV - ms
    assert mpm > 0
    case["pm"] = np.array([[mpm, 0.0, 0.0, zp]])
    res = dm.solve(case)
    assert res["flags"] == 0
    xs, _, zs, _, th, _ = res["pose"]
    assert abs(res["pose"][1]) < 1e-9 and abs(res["pose"][3]) < 1e-10 and abs(res["pose"][5]) < 1e-10
    assert th > 0.02, "the case must pitch for the moments to count"
    rg = sc.RHO * sc.GRAV
    wet = (D * np.cos(th) - zs) / np.cos(th)
    B = rg * np.pi * a * a * wet
    M = -rg * np.pi * (d * d / 32 * (2 + np.tan(th) ** 2) + wet * wet / 2) * np.sin(th)
    moor = mr.evaluate(pair[None], res["pose"][None], depth)["F"][0].astype(np.float64)
    heave = B - (ms + mpm) * sc.GRAV + case["F_env"][2] + moor[2]
    pitch = M + D * np.sin(th) * B + (ms * (h - D) / 2 + mpm * zp) * sc.GRAV * np.sin(th) + case["F_env"][4] + moor[4]
    surge = case["F_env"][0] + moor[0]
    print("pose", res["pose"], "heave", heave, "pitch", pitch, "surge", surge, "buoyancy", B)
    assert abs(heave) <= 1e-9 * B
    assert abs(surge) <= 1e-9 * B
    assert abs(pitch) <= 1e-9 * B * sc.HUB
    # ... and the same three at the reference's root
    ref = nr.solve(case)
    assert nr.convergence_excess(res["pose"], ref, mp.TOL).max() <= nr.GATE
