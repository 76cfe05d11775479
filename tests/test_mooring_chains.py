"""Composite mooring lines on the CPU: the longdouble reference's own checks (tests/mooring_chain_reference.py: every accuracy
case solves, fd_check, the split identity), the gate constant measured with the fp64 model of the device algorithm
(tests/mooring_chain_device_model.py) and the seeded errors it must reject, the flag cases, and
raft_amd.mooring.chains_from_design."""
import copy

import numpy as np
import pytest

from raft_amd.mooring import ML_CONT, ML_WJOINT, MooringProgram, chains_from_design, lines_from_design
from raft_amd.strips import UnsupportedFOWT
from tests import mooring_cases as mc
from tests import mooring_chain_cases as cc
from tests import mooring_chain_device_model as cm
from tests import mooring_chain_reference as cr
from tests import mooring_reference as mr


def test_every_accuracy_case_solves_in_the_reference():
    for name, lines, pose, depth in cc.batches():
        ref = cc.reference()[name]
        assert not ref["flags"].any(), (name, ref["flags"])
        for k in ("C", "F", "T", "J", "line_out"):
            assert np.all(np.isfinite(np.asarray(ref[k], dtype=float))), (name, k)
    # the cases are what they are named for
    lo = np.asarray(cc.reference()["chain-rope-chain"]["line_out"], dtype=float)
    assert lo[0, 0, 6] == 1 and lo[-1, 0, 6] == 0 and set(lo[:, 0, 6]) == {0.0, 1.0}     # resting, then lifted off
    assert np.all(lo[:, 1:, 6] == 0) and np.all(lo[:, 1:, 4] == 0)
    assert np.all(np.asarray(cc.reference()["clump+buoy"]["line_out"], dtype=float)[:, 2, 3] < 0)      # V_bottom < 0 above the buoy
    off = np.asarray(cc.reference()["anchor-off-the-bed"]["line_out"], dtype=float)
    assert np.all(off[:, 0, 6] == 0) and np.all(off[:, 0, 3] < 0)                          # suspended: the chain sags below its anchor


def test_reference_fd_check():
    """C and J of the reference against central differences of its own force function: one design of every accuracy batch
    (h = 1e-4 m / rad: a correct derivative agrees to about h^2 times a curvature ratio, a wrong one is off by O(1)).  At the
    displaced and rotated pose POSES[3], not the batch's own: at a pure surge the entries that vanish by symmetry are rounding
    noise of the heading's sine in the analytic result and exact zeros in the differences."""
    for name, lines, pose, depth in cc.batches():
        eC, eJ = cr.fd_check(lines[-1], cc.POSES[3], depth)
        print("%-28s fd_check: C %.3g  J %.3g" % (name, eC, eJ))
        assert eC < 1e-6 and eJ < 1e-6, (name, eC, eJ)


def test_split_identity_in_the_reference():
    """A line cut into rows of equal properties with weightless joints is the line: C, F of the design, and the tension and
    its gradient at the anchor (end A of the head row) and at the fairlead (end B of the last row), against the single-line
    reference that tests/golden/refgold_mooring.npz pins.  Both sides are longdouble solves to stagnation, each good to a few
    tens of longdouble roundings times the conditioning that Ek carries; a longdouble rounding is 2^-11 of an fp64 one, so
    they must agree within 2^-4 of eps Ek (128 longdouble roundings), a 512th of the chain gate."""
    for name, lines, pose, depth, recs in cc.split_batches():
        ref, one = cc.reference()[name], cc.split_reference()[name]
        k, nR, nL = len(cc.SPLITS[int(name[-1])]), lines.shape[1], len(recs)
        for q in ("C", "F"):
            m = cr.gate_multiples(ref[q], one[q], one["E" + q])
            assert m.max() < 2.0 ** -4, (name, q, float(m.max()))
        first, last = np.arange(nL) * k, nR + np.arange(nL) * k + (k - 1)
        for q in ("T", "J"):
            got = np.concatenate([ref[q][:, first], ref[q][:, last]], axis=1)
            m = cr.gate_multiples(got, one[q], one["E" + q])
            assert m.max() < 2.0 ** -4, (name, q, float(m.max()))


def _model_worst(seed=None):
    worst = {}
    for name, lines, pose, depth in cc.batches():
        res = cm.evaluate(lines, pose, depth, seed=seed)
        ref = cc.reference()[name]
        if res["flags"].any():
            worst[name] = np.inf
            continue
        worst[name] = max(cc.worst_multiples(res, ref).values())
        lo, lr = res["line_out"], np.asarray(ref["line_out"], dtype=float)
        if seed is None:
            assert np.array_equal(lo[..., 6], lr[..., 6]), name
    return worst


def test_gate_constant_is_the_measured_one():
    worst = _model_worst()
    for name, v in worst.items():
        print("%-28s worst multiple of eps Ek (fp64 model): %.3g" % (name, v))
    w = max(worst.values())
    print("worst over the cases: %.4g -> gate %d" % (w, cr.GATE_C))
    assert abs(w - cr.GATE_WORST_CPU) <= 0.02 * cr.GATE_WORST_CPU, (w, cr.GATE_WORST_CPU)
    assert cr.GATE_C == 2 ** int(np.ceil(np.log2(4 * cr.GATE_WORST_CPU)))


@pytest.mark.parametrize("seed", cm.SEEDS)
def test_gate_rejects_seeded_errors(seed):
    worst = _model_worst(seed)
    hit = {k: v for k, v in worst.items() if v > cr.GATE_C}
    print(seed, {k: ("%.3g" % v) for k, v in worst.items()})
    assert hit, (seed, worst)


def test_split_identity_in_the_model():
    """... and in the device algorithm: cut lines against the uncut single-line reference under the chain gate."""
    for name, lines, pose, depth, recs in cc.split_batches():
        res, one = cm.evaluate(lines, pose, depth), cc.split_reference()[name]
        k, nR, nL = len(cc.SPLITS[int(name[-1])]), lines.shape[1], len(recs)
        first, last = np.arange(nL) * k, nR + np.arange(nL) * k + (k - 1)
        for q in ("C", "F"):
            assert cr.gate_multiples(res[q], one[q], one["E" + q]).max() <= cr.GATE_C, (name, q)
        for q in ("T", "J"):
            got = np.concatenate([res[q][:, first], res[q][:, last]], axis=1)
            assert cr.gate_multiples(got, one[q], one["E" + q]).max() <= cr.GATE_C, (name, q)


def test_flag_cases_in_the_model():
    for name, lines, depth, flag in cc.flag_cases():
        res = cm.evaluate(lines, None, depth)
        assert list(res["flags"]) == [0, flag, 0], (name, res["flags"])
        assert np.all(np.isnan(res["C"][1])) and np.all(np.isfinite(res["C"][[0, 2]]))
        alone = cm.evaluate(lines[:1], None, depth)
        assert np.array_equal(alone["C"][0], res["C"][0]) and np.array_equal(alone["J"][0], res["J"][0])


def test_single_rows_take_the_single_line_model():
    g = mc.golden()["VolturnUS-S"]
    lines = np.broadcast_to(g["lines"], (4, 3, 16)).copy()
    a, b = cm.evaluate(lines, mc.POSES, g["depth"]), mc.mr.evaluate(lines, mc.POSES, g["depth"])
    assert max(mc.worst_multiples(a, b).values()) <= mr.GATE_C
    c = cr.evaluate(lines, mc.POSES, g["depth"])
    for q in ("C", "F", "T", "J"):
        assert cr.gate_multiples(c[q], b[q], b["E" + q]).max() < 2.0 ** -4, q


# ---- chains_from_design
def _crc_deck():
    """The VolturnUS-S deck with every line edited to chain - rope - chain through named free points; the lower joint of line 1
    carries a clump (m, v)."""
    g = mc.golden()["VolturnUS-S"]
    design = copy.deepcopy(g["design"])
    moor = design["mooring"]
    moor["water_depth"] = 600
    moor["line_types"].append(dict(name="rope", diameter=0.2, mass_density=60.0, stiffness="5e8"))
    lines, points = [], []
    for p in moor["points"]:
        if p["type"] == "fixed":
            p["location"][2] = -600.0
            p["location"][0] *= 2
            p["location"][1] *= 2
    for k in (1, 2, 3):
        a, v = "line%d_anchor" % k, "line%d_vessel" % k
        j1, j2 = "line%d_joint_lower" % k, "line%d_joint_upper" % k
        points.append(dict(name=j1, type="free", location=[0, 0, -500.0], **(dict(m=30000.0, v=3.0) if k == 1 else {})))
        points.append(dict(name=j2, type="connection", location=[0, 0, -100.0]))
        # the rope first and the top chain written from the vessel down: the order and the direction in the list do not matter
        lines.append(dict(name="rope%d" % k, endA=j1, endB=j2, type="rope", length=1000))
        lines.append(dict(name="top%d" % k, endA=v, endB=j2, type="chain", length=100))
        lines.append(dict(name="bottom%d" % k, endA=a, endB=j1, type="chain", length=600))
    moor["points"] += points
    moor["lines"] = lines
    return design, g["rho"], g["g"]


def test_chains_from_design_follows_the_free_points():
    design, rho, g = _crc_deck()
    recs, depth, names = chains_from_design(design, rho, g)
    assert depth == 600.0 and recs.shape == (9, 16)
    assert names == [n % k for k in (1, 2, 3) for n in ("bottom%d", "rope%d", "top%d")]
    assert list(recs[:, ML_CONT]) == [0, 1, 1] * 3
    w_chain = (685.0 - rho * np.pi / 4 * 0.185 ** 2) * g
    w_rope = (60.0 - rho * np.pi / 4 * 0.2 ** 2) * g
    for k in range(3):
        h, r, t = recs[3 * k:3 * k + 3]
        pts = {p["name"]: p["location"] for p in design["mooring"]["points"]}
        assert list(h[0:3]) == pts["line%d_anchor" % (k + 1)] and list(h[3:6]) == pts["line%d_vessel" % (k + 1)]
        assert (h[6], h[7], h[8]) == (600.0, 3270e6, w_chain) and (r[6], r[7], r[8]) == (1000.0, 5e8, w_rope)
        assert (t[6], t[7], t[8]) == (100.0, 3270e6, w_chain)
        assert np.all(r[0:6] == 0) and np.all(t[0:6] == 0) and np.all(recs[3 * k:3 * k + 3, 11:15] == 0) and h[ML_WJOINT] == 0
        assert r[ML_WJOINT] == ((30000.0 - rho * 3.0) * g if k == 0 else 0.0) and t[ML_WJOINT] == 0.0
    # the records solve
    ref = cr.evaluate(recs[None], None, depth)
    assert ref["flags"][0] == 0
    # the program refuses the ends of a continuation row
    prog = MooringProgram(recs, 2)
    prog.ends(3, np.zeros((3, 3)), np.zeros((3, 3)))
    with pytest.raises(ValueError, match="continuation row"):
        prog.ends(4, np.zeros((3, 3)), np.zeros((3, 3)))


def test_chains_from_design_without_free_points_is_lines_from_design():
    for deck, g in mc.golden().items():
        a, da, names = chains_from_design(g["design"], g["rho"], g["g"])
        b, db = lines_from_design(g["design"], g["rho"], g["g"])
        assert np.array_equal(a, b) and da == db and len(names) == len(b), deck


def test_chains_from_design_refusals():
    design, rho, g = _crc_deck()

    def refused(edit, match):
        d = copy.deepcopy(design)
        edit(d["mooring"])
        with pytest.raises(UnsupportedFOWT, match=match):
            chains_from_design(d, rho, g)

    def bridle(m):
        m["points"].append(dict(name="fair_b", type="vessel", location=[-58.0, 5.0, -14.0]))
        m["lines"].append(dict(name="bridle", endA="line1_joint_upper", endB="fair_b", type="chain", length=100))
    refused(bridle, "'line1_joint_upper' joins 3 lines")
    refused(lambda m: m["lines"].pop(1), "dangling")                                        # top1 gone: its joint ends a single line
    def vessel_to_vessel_chain(m):                                                          # vessel - free - vessel
        m["points"].append(dict(name="fair4", type="vessel", location=[0, 58.0, -14.0]))
        m["points"].append(dict(name="fair5", type="vessel", location=[0, -58.0, -14.0]))
        m["points"].append(dict(name="mid", type="free", location=[0, 0, -50.0]))
        m["lines"] += [dict(name="u1", endA="fair4", endB="mid", type="chain", length=80), dict(name="u2", endA="mid", endB="fair5", type="chain", length=80)]
    refused(vessel_to_vessel_chain, "without a fixed end")
    def both_on_vessel(m):
        m["points"].append(dict(name="fair4", type="vessel", location=[0, 58.0, -14.0]))
        m["points"].append(dict(name="fair5", type="vessel", location=[0, -58.0, -14.0]))
        m["lines"].append(dict(name="u", endA="fair4", endB="fair5", type="chain", length=150))
    refused(both_on_vessel, "both ends on the vessel")
    def five_segments(m):
        m["points"] += [dict(name="x1", type="free", location=[0, 0, -90.0]), dict(name="x2", type="free", location=[0, 0, -80.0])]
        top = [l for l in m["lines"] if l["name"] == "top1"][0]
        top["endA"] = "x1"
        m["lines"] += [dict(name="t2", endA="x1", endB="x2", type="chain", length=10), dict(name="t3", endA="x2", endB="line1_vessel", type="chain", length=10)]
    refused(five_segments, "more than 4 segments")
    refused(lambda m: m.__setitem__("file", "lines.dat"), "MoorDyn file")
    refused(lambda m: m.__setitem__("moorMod", 1), "moorMod")
    with pytest.raises(UnsupportedFOWT, match="no mooring section"):
        chains_from_design({}, rho, g)
    # lines_from_design still refuses the deck as a whole
    with pytest.raises(UnsupportedFOWT, match="free points are not covered"):
        lines_from_design(design, rho, g)
