"""The mean-pose solve of include/raftx_statics.h on the CPU: the longdouble reference (tests/mean_pose_reference.py)
against the reference implementation's recorded poses (tests/golden/refgold_mean_pose.npz), the fp64 model of the kernel
(tests/mean_pose_device_model.py) against that reference under the gate, the deliberate errors the gate must reject or
tolerate, and the safeguards and flags.  The kernel itself is held to the same gate in tests/test_hip_mean_pose.py.
"""
import math

import numpy as np
import pytest

from . import mean_pose_cases as cs
from . import mean_pose_device_model as mdm
from . import mean_pose_reference as mpr
from . import mooring_cases as mc

CASES = sorted(cs.cases())
DECK_CASES = [(deck, case) for deck in cs.decks() for case in ("wave", "current")]


def model(name, **kw):
    c = cs.cases()[name]
    return mdm.solve(c["lines"], c["depth"], c["K_hs"], c["F0"], c["F_env"], c["x_ref"], **kw)


@pytest.mark.parametrize("deck,case", DECK_CASES)
def test_reference_reproduces_the_recorded_pose(deck, case):
    """The root lies within the reference implementation's own stopping tolerance (0.05 m, 0.005 rad; raft_model.py:664)
    of its recorded desired_X0, and root - record is the Newton step at the record to 5 % of that step's largest
    translation: the record is a loosely converged iterate of the same equations.  Measured: worst distance 0.039 m
    (OC4semi-WAMIT_Coefs, 'current'), worst step mismatch 0.08 % of the step."""
    name = deck + ("/unloaded" if case == "wave" else "/current")
    c, ref = cs.cases()[name], cs.reference(name)
    record = cs.decks()[deck]["records"][case]
    diff = (ref["x"] - record).astype(np.float64)
    print("%s %s: |root - record| %.3g m, %.3g rad" % (deck, case, np.abs(diff[:3]).max(), np.abs(diff[3:]).max()))
    assert np.abs(diff[:3]).max() <= mpr.REF_TOL[0] and np.abs(diff[3:]).max() <= mpr.REF_TOL[1]
    step = mpr.newton_step(c["lines"], c["depth"], c["K_hs"], c["F0"], c["F_env"], c["x_ref"], at=record).astype(np.float64)
    print("   step mismatch %.3g of the step" % (np.abs(diff - step).max() / np.abs(step[:3]).max()))
    assert np.abs(diff - step).max() <= 0.05 * np.abs(step[:3]).max()


def test_gate_constant_is_four_times_the_measured_worst():
    worst = {}
    for name in CASES:
        m = model(name)
        assert m["flags"] == 0, name
        worst[name] = float(mpr.pose_multiples(m["pose"], cs.reference(name)).max())
    w = max(worst.values())
    print("worst multiple of eps |K^-1| E_F: %.3g (%s)" % (w, max(worst, key=worst.get)))
    assert w <= mpr.GATE_WORST_CPU
    assert mpr.GATE == 2 ** math.ceil(math.log2(4 * mpr.GATE_WORST_CPU))


@pytest.mark.parametrize("name", CASES)
def test_model_within_gate(name):
    m, ref = model(name), cs.reference(name)
    assert m["flags"] == 0
    mult = mpr.pose_multiples(m["pose"], ref)
    print("%s: pose multiples %s, %d steps" % (name, np.array2string(mult, precision=3), m["iterations"]))
    assert np.all(mult <= mpr.GATE)
    rn = np.linalg.norm(m["F_res"]) / (mpr.EPS * np.linalg.norm(ref["E_F"].astype(np.float64)))
    assert rn <= mpr.GATE


def _stagnation_tol(ref):
    """Step tolerances at the rounding level of a case: eps times the smallest non-zero bound of the translations / rotations."""
    b = ref["bound"].astype(np.float64)
    return (mpr.EPS * b[:3][b[:3] > 0].min(), mpr.EPS * b[3:][b[3:] > 0].min())


@pytest.mark.parametrize("name", ["single/contact", "single/anchor_off_seabed"])
def test_jacobian_without_arm_term_still_converges(name):
    """-[f x][r x] dropped from the Jacobian K': the root is that of the same Y, reached in more steps -- linearly, at the
    rate rho(I - K'^-1 K), so the cases are those where that rate is below one (asserted on the Jacobians at the
    reference's root) and the step tolerance is set at the rounding level: a linearly converging iterate whose step is
    1e-9 m is still far outside the gate.  On the decks the dropped term is most of the yaw stiffness (the hydrostatics
    have none): there rho > 1 and the seeded iteration diverges, which the gate rejects as well."""
    c, ref = cs.cases()[name], cs.reference(name)
    x = ref["x"].astype(np.float64)
    K = c["K_hs"] + mdm.moor(c["lines"], x, c["depth"])[1]
    Kp = c["K_hs"] + mdm.moor(c["lines"], x, c["depth"], "no_fr")[1]
    rho = np.abs(np.linalg.eigvals(np.eye(6) - np.linalg.solve(Kp, K))).max()
    print("%s: rate %.3f" % (name, rho))
    assert rho < 1
    tol = _stagnation_tol(ref)
    good, bad = model(name, tol=tol, max_iter=100), model(name, seed="no_fr", tol=tol, max_iter=100)
    assert good["flags"] == 0 and bad["flags"] == 0
    assert np.all(mpr.pose_multiples(bad["pose"], ref) <= mpr.GATE)
    assert bad["iterations"] > good["iterations"]


def test_jacobian_without_arm_term_diverges_on_a_deck():
    c, ref = cs.cases()["VolturnUS-S/thrust"], cs.reference("VolturnUS-S/thrust")
    x = ref["x"].astype(np.float64)
    K = c["K_hs"] + mdm.moor(c["lines"], x, c["depth"])[1]
    Kp = c["K_hs"] + mdm.moor(c["lines"], x, c["depth"], "no_fr")[1]
    assert np.abs(np.linalg.eigvals(np.eye(6) - np.linalg.solve(Kp, K))).max() > 1
    assert model("VolturnUS-S/thrust", seed="no_fr")["flags"] == mdm.FLAG_POSE_CAP


@pytest.mark.parametrize("seed,name", [("khs_sign", "VolturnUS-S/thrust"), ("khs_sign", "single/contact"), ("no_xref", "x_ref")])
def test_gate_rejects_seeded_errors(seed, name):
    bad, ref = model(name, seed=seed), cs.reference(name)
    assert bad["flags"] != 0 or np.any(mpr.pose_multiples(bad["pose"], ref) > mpr.GATE)


def test_zero_diagonal_takes_the_mean():
    K = cs.synthetic_K()
    K[5, :] = 0.0
    K[:, 5] = 0.0
    Y = np.array([1.0e4, -2.0e4, 3.0e4, 1.0e6, 2.0e6, 5.0e6])
    log = []
    dX, sing = mdm.step(K, Y, log)
    assert not sing and ("zero_diagonal", 5) in log
    Kfix = K.copy()
    Kfix[5, 5] = np.trace(K) / 6.0
    assert np.allclose(dX, np.linalg.solve(Kfix, Y), rtol=1e-12)
    assert dX[5] == pytest.approx(Y[5] / Kfix[5, 5], rel=1e-12)


def test_backward_step_enlarges_the_diagonal():
    """An indefinite K for which K^-1 Y points against Y: the diagonal grows by 10 % per try until dX.Y >= 0 or ten tries."""
    K = np.diag([1.0e5, 1.0e5, 1.0e5, 1.0e8, 1.0e8, 1.0e8])
    K[0, 1] = K[1, 0] = 1.2e5                                       # eigenvalues of the block: 2.2e5, -0.2e5
    Y = np.array([1.0e4, -1.0e4, 0.0, 0.0, 0.0, 0.0])               # along the negative eigenvector
    assert float(np.dot(np.linalg.solve(K, Y), Y)) < 0
    log = []
    dX, sing = mdm.step(K, Y, log)
    n = sum(1 for what, _ in log if what == "enlarged")
    assert not sing and 1 <= n <= 10
    assert float(np.dot(dX, Y)) >= 0
    Kn = K.copy()
    Kn[np.diag_indices(6)] *= 1.1 ** n
    assert np.allclose(dX, np.linalg.solve(Kn, Y), rtol=1e-9)
    K[0, 1] = K[1, 0] = 1.0e7                                       # ten tries do not suffice: the last solve is kept
    log = []
    dX, sing = mdm.step(K, Y, log)
    assert not sing and sum(1 for what, _ in log if what == "enlarged") == 10


def test_step_caps_hold_under_a_large_surge_load():
    c = cs.cases()["VolturnUS-S/unloaded"]
    F_env = np.array([5.0e6, 0, 0, 0, 0, 0])
    K = c["K_hs"] + mdm.moor(c["lines"], np.zeros(6), c["depth"])[1]
    Y = mdm.residual(c["K_hs"], c["F0"], F_env, np.zeros(6), np.zeros(6), mdm.moor(c["lines"], np.zeros(6), c["depth"])[2])
    raw = np.linalg.solve(K, Y)
    assert np.any(np.abs(raw) > mdm.CAPS)
    log = []
    dX, sing = mdm.step(K, Y, log)
    assert not sing and any(what == "capped" for what, _ in log)
    assert np.all(np.abs(dX) <= np.array(mdm.CAPS) * (1 + 4 * mpr.EPS))
    ratio = dX / raw
    assert np.allclose(ratio, ratio[0], rtol=1e-12) and np.any(np.isclose(np.abs(dX), mdm.CAPS, rtol=1e-12))


def test_cap_bit_with_two_iterations():
    m = model("VolturnUS-S/thrust", max_iter=2)
    assert m["flags"] == mdm.FLAG_POSE_CAP and m["iterations"] == 2
    assert all(np.all(np.isnan(m[k])) for k in ("pose", "C", "F", "T", "J", "F_res"))


def test_line_going_slack_mid_iteration_is_flagged():
    """A load that pushes the unit towards the anchor of a single line: the first pose is fine, a later one is slack."""
    rec, depth = mc.single_lines()["contact"]
    K = cs.synthetic_K()
    F0 = np.array([-4.0e7, 0, 0, 0, 0, 0])                         # 200 m of surge against K_hs: steps of 30 m
    assert mdm.moor(rec[None], np.zeros(6), depth)[0] == 0
    m = mdm.solve(rec[None], depth, K, F0)
    assert m["flags"] == 4 and m["iterations"] >= 2
    assert np.all(np.isnan(m["pose"]))
