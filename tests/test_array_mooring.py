"""The array mooring system of include/raftx_array_mooring.h on the CPU: the longdouble reference
(tests/array_mooring_reference.py) against central differences of its own force function and against the pinned single-line
path, its invariants, the fp64 model of the device algorithm (tests/array_mooring_device_model.py) against it under the gates
-- whose constants are measured HERE -- the seeded errors the gates must reject, and the record errors of
``raft_amd.mooring.array_lines``.  The kernels themselves: tests/test_hip_array_mooring.py."""
import numpy as np
import pytest

from raft_amd import mooring
from tests import array_mooring_cases as ac
from tests import array_mooring_device_model as adm
from tests import array_mooring_reference as ar
from tests import mooring_reference as mr


def _root64(name):
    c = ac.cases()[name]
    return ac.reference(name)["x"].astype(np.float64).reshape(len(c["K_hs"]), 6)


@pytest.mark.parametrize("name", ["pair", "pair_yaw_pitch", "row3"])
def test_reference_against_central_differences(name):
    """C and J over all 6 nUnit DOFs at the solved pose (ZF != 0, rotations != 0) against the reference's own force function."""
    c = ac.cases()[name]
    eC, eJ = ar.fd_check(c["lines"], _root64(name), c["depth"])
    print("%s: analytic vs central differences, worst / envelope: C %.3g, J %.3g" % (name, eC, eJ))
    assert eC < 1e-6 and eJ < 1e-6        # h = 1e-4 m / rad: the differences' own O(h^2) error; a wrong term is O(1)


def test_pair_is_the_case_the_header_describes():
    """ZF exactly 0 at the first iterate; about 8 m towards each other; the lowest point at -137 m; cond K about 4e4."""
    c = ac.cases()["pair"]
    assert adm.shared(c["lines"][-1], c["x_ref"][0], c["x_ref"][1], c["depth"])[1]["lo"][1] * 2 == c["lines"][-1, 8] * c["lines"][-1, 6]  # VF = wL/2: ZF == 0
    r = ac.reference("pair")
    dx = r["x"].astype(np.float64).reshape(2, 6) - c["x_ref"]
    assert 8.2 < dx[0, 0] < 8.4 and -8.4 < dx[1, 0] < -7.5
    assert abs(np.nanmin(r["moor"]["low"]) + 137.0) < 0.5
    assert 3e4 < np.linalg.cond(r["K"].astype(np.float64)) < 6e4
    assert r["iterations"] <= 6


def test_frozen_partner_identity():
    """With unit A held fixed and A's end the lower one, unit B's block of a shared row is ``mooring_reference.evaluate`` of an
    anchored row whose suspended anchor is A's global attachment point: C, F, T, J and the solve itself (HF, VF)."""
    depth = 600.0
    pose = np.array([[0.0, 0.0, -2.0, 0.01, -0.02, 0.3], [1500.0, 40.0, 1.0, -0.02, 0.015, -0.1]])
    sh = mooring.array_lines([np.zeros((0, 16)), np.zeros((0, 16))], [(0, 0), (0, 0)],
                             shared=[dict(unitA=0, rA=(58.0, 3.0, -150.0), unitB=1, rB=(-58.0, -2.0, -14.0), L=1460.0, EA=2.0e8, w=300.0)])
    a = ar.evaluate(sh, pose, depth)
    assert a["flags"] == 0
    pA = pose[0, :3] + np.asarray(mr.rotation(pose[0, 3:], np.float64) @ sh[0, 0:3])
    rec = sh[0].copy()
    rec[0:3], rec[11], rec[12] = pA, 0.0, 0.0                    # (the anchor rounds to fp64: the identity holds to that rounding)
    m = mr.evaluate(rec[None, None], pose[1][None], depth)
    assert m["flags"][0] == 0 and m["line_out"][0, 0, 6] == 0    # suspended: no seabed contact
    for k, sub in (("C", (slice(6, 12), slice(6, 12))), ("F", (slice(6, 12),)), ("J", (slice(None), slice(6, 12)))):
        got, want = a[k][sub].astype(np.float64), m[k][0].astype(np.float64)
        assert np.allclose(got, want, rtol=1e-11, atol=1e-11 * np.abs(want).max()), k
    assert np.allclose(a["T"].astype(np.float64), m["T"][0].astype(np.float64), rtol=1e-12)


def test_shared_rows_alone_balance():
    """An array of shared rows only: sum over the units of F[:3] = (0, 0, -sum wL) within the envelope."""
    c = ac.cases()["ring6"]
    sh = c["lines"][c["lines"][:, 12] > 0]
    pose = _root64("ring6")
    a = ar.evaluate(sh, pose, c["depth"])
    tot = a["F"].reshape(6, 6)[:, :3].sum(axis=0)
    E = a["EF"].reshape(6, 6)[:, :3].sum(axis=0)
    want = np.array([0.0, 0.0, -float(np.sum(sh[:, 8] * sh[:, 6]))])
    assert np.all(np.abs(tot - want) <= 4 * ar.EPS * E), (tot, want)
    m = adm.evaluate(sh, pose, c["depth"])
    assert np.all(np.abs(m["F"].reshape(6, 6)[:, :3].sum(axis=0) - want) <= ar.GATE_C * ar.EPS * E.astype(np.float64))


def test_exchanging_the_ends_of_a_shared_row():
    """... exchanges T_A and T_B and leaves C and F within the gate (reference against reference: to rounding; model against it)."""
    c = ac.cases()["pair_yaw_pitch"]
    pose = _root64("pair_yaw_pitch")
    sw = c["lines"].copy()
    l = len(sw) - 1
    sw[l, 0:3], sw[l, 3:6] = c["lines"][l, 3:6], c["lines"][l, 0:3]
    sw[l, 11], sw[l, 12] = c["lines"][l, 12] - 1, c["lines"][l, 11] + 1
    a, b = ar.evaluate(c["lines"], pose, c["depth"]), ar.evaluate(sw, pose, c["depth"])
    nL = len(sw)
    assert np.all(mr.gate_multiples(b["C"], a["C"], a["EC"]) <= 1e-2) and np.all(mr.gate_multiples(b["F"], a["F"], a["EF"]) <= 1e-2)
    assert abs(b["T"][l] - a["T"][nL + l]) <= 1e-2 * ar.EPS * a["ET"][nL + l] and abs(b["T"][nL + l] - a["T"][l]) <= 1e-2 * ar.EPS * a["ET"][l]
    m = adm.evaluate(sw, pose, c["depth"])
    w = {k: float(mr.gate_multiples(m[k], a[k], a["E" + k]).max()) for k in ("C", "F")}
    print("exchanged ends, model against the reference of the original: %s" % w)
    assert max(w.values()) <= ar.GATE_C


def test_horizontal_shift():
    """Shifting all poses and anchors horizontally by one vector leaves C and F within the gate."""
    c = ac.cases()["row3"]
    pose = _root64("row3")
    shift = np.array([317.25, -1280.5])
    lines, moved = c["lines"].copy(), pose.copy()
    lines[lines[:, 12] == 0, 0:2] += shift
    moved[:, :2] += shift
    a = ar.evaluate(c["lines"], pose, c["depth"])
    b = ar.evaluate(lines, moved, c["depth"])
    m = adm.evaluate(lines, moved, c["depth"])
    for res in (b, m):
        w = {k: float(mr.gate_multiples(res[k], a[k], b["E" + k]).max()) for k in ("C", "F")}
        print("shifted by %s: %s" % (shift, w))
        assert max(w.values()) <= ar.GATE_C


def test_model_against_the_reference_under_the_gates():
    """The gates' constants: the model's worst multiples over the case list, C / F / T / J at the reference poses and at its own
    solved poses, and the pose itself.  GATE_WORST_CPU and POSE_WORST_CPU of tests/array_mooring_reference.py are these."""
    worst, worst_pose, worst_res = 0.0, 0.0, 0.0
    for name in ac.NAMES:
        c = ac.cases()[name]
        ref = ac.reference(name)
        m = adm.solve(c["lines"], c["depth"], c["K_hs"], c["F0"], c["F_env"], c["x_ref"])
        assert m["flags"] == 0, name
        pm = float(ar.multiples(m["pose"].reshape(-1), ref["x"], ref["bound"]).max())
        rn = float(np.linalg.norm(m["F_res"]) / (ar.EPS * np.linalg.norm(ref["E_F"].astype(np.float64))))
        w0 = ar.worst_multiples(adm.evaluate(c["lines"], c["x_ref"], c["depth"]), ar.evaluate(c["lines"], c["x_ref"], c["depth"]))
        w1 = ar.worst_multiples(m, ar.evaluate(c["lines"], m["pose"], c["depth"]))
        print("%-18s %d steps (reference %d)  pose %.3g  residual %.3g  at x_ref %s  at the pose %s" % (
            name, m["iterations"], ref["iterations"], pm, rn, {k: round(v, 2) for k, v in w0.items()}, {k: round(v, 2) for k, v in w1.items()}))
        assert m["iterations"] <= ref["iterations"] + 1
        worst, worst_pose, worst_res = max(worst, *w0.values(), *w1.values()), max(worst_pose, pm), max(worst_res, rn)
    print("worst C/F/T/J multiple %.3g (gate %g), worst pose multiple %.3g (gate %g), worst residual %.3g" % (
        worst, ar.GATE_C, worst_pose, ar.GATE_POSE, worst_res))
    assert worst <= ar.GATE_WORST_CPU * 1.001 and worst_pose <= ar.POSE_WORST_CPU * 1.001
    assert ar.GATE_C == 2.0 ** np.ceil(np.log2(4 * ar.GATE_WORST_CPU)) and ar.GATE_POSE == 2.0 ** np.ceil(np.log2(4 * ar.POSE_WORST_CPU))
    assert worst_res <= ar.GATE_POSE


def test_pair_grounded_rises_mid_iteration():
    c = ac.cases()["pair_grounded"]
    first = ar.evaluate(c["lines"], c["x_ref"], c["depth"])
    assert first["flags"] == 0 and abs(np.nanmin(first["low"]) + 128.0) < 1.0
    with pytest.raises(ValueError, match="flags the iterate [1-9]"):
        ac.reference("pair_grounded")
    m = adm.solve(c["lines"], c["depth"], c["K_hs"], c["F0"], c["F_env"], c["x_ref"])
    assert m["flags"] == adm.FLAG_GROUNDED and m["iterations"] >= 1 and np.all(np.isnan(m["pose"]))


@pytest.mark.parametrize("seed", adm.SEEDS)
def test_the_gates_reject_seeded_errors(seed):
    """A dropped cross block, a cross block of the wrong sign, an arm-turning term on the wrong unit, VA taken as 0."""
    c = ac.cases()["pair_yaw_pitch"]
    pose = _root64("pair_yaw_pitch")
    at = ar.evaluate(c["lines"], pose, c["depth"])
    w = ar.worst_multiples(adm.evaluate(c["lines"], pose, c["depth"], seed=seed), at)
    print("seed %-15s worst multiples %s" % (seed, {k: "%.3g" % v for k, v in w.items()}))
    assert max(w["C"], w["F"]) > 1e3 * ar.GATE_C
    ref = ac.reference("pair_yaw_pitch")
    m = adm.solve(c["lines"], c["depth"], c["K_hs"], c["F0"], c["F_env"], c["x_ref"], seed=seed)
    if seed == "va_zero":                                        # a wrong force moves the root itself
        assert m["flags"] or float(ar.multiples(m["pose"].reshape(-1), ref["x"], ref["bound"]).max()) > 1e3 * ar.GATE_POSE


def test_array_lines_records_and_errors():
    d = ac.cases()["pair"]["lines"]
    assert d.shape == (7, 16) and list(d[:, 11]) == [0, 0, 0, 1, 1, 1, 1] and list(d[:, 12]) == [0] * 6 + [1]
    one = ac.cases()["single_unit"]["lines"]
    assert np.array_equal(d[:3], one)                             # unit 0: the deck's own records
    assert np.allclose(d[3:6, 0], 1600.0 - one[:, 0], atol=1e-9) and np.allclose(d[3:6, 1], -one[:, 1], atol=1e-9)   # unit 1: turned, then shifted
    assert np.allclose(d[3:6, 3], -one[:, 3], atol=1e-12) and np.array_equal(d[3:6, 6:9], one[:, 6:9])
    assert list(d[6, :9]) == [58.0, 0.0, -14.0, -58.0, 0.0, -14.0, 1490.0, 2.0e8, 300.0]
    sh = dict(unitA=0, rA=(58, 0, -14), unitB=1, rB=(-58, 0, -14), L=1490.0, EA=2e8, w=300.0)
    for bad, msg in ((dict(sh, unitB=0), "both ends"), (dict(sh, unitA=2), "no unit index"), (dict(sh, unitB=0.5), "no unit index"),
                     (dict(sh, L=0.0), "positive"), ({k: v for k, v in sh.items() if k != "w"}, "lacks")):
        with pytest.raises(ValueError, match=msg):
            mooring.array_lines([one, one], [(0, 0), (1600, 0)], [0, 180], [bad])
    with pytest.raises(ValueError, match="1 to 6 units"):
        mooring.array_lines([one] * 7, np.zeros((7, 2)))
    with pytest.raises(ValueError, match="unit fields already"):
        mooring.array_lines([d], [(0, 0)])
    with pytest.raises(ValueError, match="no rows"):
        mooring.array_lines([np.zeros((0, 16))], [(0, 0)])
