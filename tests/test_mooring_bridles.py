"""Bridle mooring lines on the CPU: the longdouble reference's own checks (tests/mooring_bridle_reference.py: every accuracy case
solves, fd_check, the coincident-legs and mirror identities), the gate constant measured with the fp64 model of the device
algorithm (tests/mooring_bridle_device_model.py) and the seeded errors it must reject, the flag cases, and
raft_amd.mooring.bridles_from_design."""
import copy

import numpy as np
import pytest

from raft_amd.mooring import (MAX_LEG, ML_CONT, ML_LEG, ML_WJOINT, MooringProgram, bridles_from_design, chains_from_design,
                              lines_from_design)
from raft_amd.strips import UnsupportedFOWT
from tests import mooring_bridle_cases as bc
from tests import mooring_bridle_device_model as bm
from tests import mooring_bridle_reference as br
from tests import mooring_cases as mc
from tests import mooring_chain_reference as cr

_REF = {}


def reference(name, ip):
    """The longdouble reference of an accuracy case at POSES[ip], computed once."""
    if (name, ip) not in _REF:
        rows, depth = bc.ACCURACY[name]
        _REF[name, ip] = br.evaluate(rows[None], bc.POSES[ip][None], depth)
    return _REF[name, ip]


def worst_multiples(res, ref):
    out = {k: float(br.gate_multiples(res[k], ref[k], ref["E" + k]).max()) for k in ("C", "F", "T", "J")}
    lo, lr = np.asarray(res["line_out"], dtype=float), np.asarray(ref["line_out"], dtype=float)
    # line_out: forces against the tensions' envelope of their row (HF, V <= T), L_B in metres against the stem's length scale
    nL = lo.shape[1]
    ET = np.asarray(ref["ET"], dtype=np.longdouble)
    for k, e in ((0, 1), (1, 1), (2, 0), (3, 1)):
        out["lo%d" % k] = float(br.gate_multiples(lo[..., k], lr[..., k], np.maximum(ET[:, :nL], ET[:, nL:])).max())
    return out


def test_every_accuracy_case_solves_in_the_reference():
    for name in bc.ACCURACY:
        for ip in range(len(bc.POSES)):
            ref = reference(name, ip)
            assert not ref["flags"].any(), (name, ip, ref["flags"])
            for k in ("C", "F", "T", "J", "line_out"):
                assert np.all(np.isfinite(np.asarray(ref[k], dtype=float))), (name, ip, k)
    # the cases are what they are named for
    assert float(reference("stem_on_seabed", 0)["line_out"][0, 0, 4]) > 100.0 and reference("stem_on_seabed", 0)["line_out"][0, 0, 6] == 1
    assert float(reference("chain_rope_600", 1)["line_out"][0, 0, 4]) > 100.0
    for name in ("symmetric_200", "clump", "buoy", "chain_rope_600", "stem_on_seabed"):
        T = np.asarray(reference(name, 1)["T"][0], dtype=float)
        n = len(T) // 2
        assert T[2 * n - 1] > 3.0 * T[2 * n - 2], name             # at the yawed offset one leg is much slacker than the other
    assert float(reference("buoy", 0)["C"][0, 5, 5]) > 0 and float(reference("symmetric_200", 0)["C"][0, 5, 5]) > 1e8   # yaw stiffness


def test_reference_fd_check():
    """C and J of the reference against central differences of its own force function, every case at the yawed offset
    (h = 1e-4 m / rad: a correct derivative agrees to about h^2 times a curvature ratio, a wrong one is off by O(1))."""
    for name, (rows, depth) in bc.ACCURACY.items():
        ns = int(np.sum(rows[:, ML_LEG] == 0))
        eC, eJ = br.fd_check(rows, ns, bc.POSES[1], depth)
        print("%-18s fd_check: C %.3g  J %.3g" % (name, eC, eJ))
        assert eC < 1e-6 and eJ < 1e-6, (name, eC, eJ)


def _coincident(evaluate):
    """Multiples of eps E of (bridle with coincident legs) - (composite line), E = the chain reference's envelope + the bridle
    reference's: either side is a solve of its own, each good to its own envelope -- the bridle's carries the conditioning of
    the junction, which the chain's two-unknown system does not have."""
    two, one, depth = bc.coincident_legs()
    out = []
    for pose in bc.POSES:
        a = evaluate(two[None], pose[None], depth)
        e = br.evaluate(two[None], pose[None], depth)
        b = cr.evaluate(one[None], pose[None], depth)
        assert not a["flags"].any() and not b["flags"].any() and not e["flags"].any()
        m = {q: float(br.gate_multiples(a[q], b[q], b["E" + q] + e["E" + q]).max()) for q in ("C", "F")}
        # the two legs together carry what the chain's last segment carries; the stem is the chain's first
        for q in ("T", "J"):
            x, y, Eb, Ee = np.asarray(a[q][0]), np.asarray(b[q][0]), np.asarray(b["E" + q][0]), np.asarray(e["E" + q][0])
            got = np.stack([x[0], x[1] + x[2], x[3], x[4] + x[5]])
            env = Eb + np.stack([Ee[0], Ee[1] + Ee[2], Ee[3], Ee[4] + Ee[5]])
            m[q] = float(br.gate_multiples(got, y, env).max())
        out.append(m)
    return out


def test_coincident_legs_identity_in_the_reference():
    """Two legs to one fairlead, each with EA/2 and w/2 and the same L, are the composite line whose last segment has EA and w:
    C, F, the stem's tensions and the SUMMED leg tensions (and their gradients) against tests/mooring_chain_reference.py, which
    the split identity ties to refgold_mooring.npz.  Both sides are longdouble solves to stagnation; a longdouble rounding is
    2^-11 of an fp64 one, so they must agree within 2^-4 of eps (128 longdouble roundings) of the two envelopes together."""
    for m in _coincident(br.evaluate):
        print({k: "%.3g" % v for k, v in m.items()})
        assert max(m.values()) < 2.0 ** -4, m


def test_coincident_legs_identity_in_the_model():
    for m in _coincident(bm.evaluate):
        print({k: "%.3g" % v for k, v in m.items()})
        assert max(m.values()) <= br.GATE_C, m


def _mirror(evaluate, bound):
    rows, depth = bc.ACCURACY["symmetric_200"]
    ref = br.evaluate(rows[None], bc.MIRROR_POSE[None], depth)
    a = evaluate(rows[None], bc.MIRROR_POSE[None], depth)
    F, EF = np.asarray(a["F"][0], dtype=np.longdouble), np.asarray(ref["EF"][0])
    for k in (1, 3, 5):                                            # F_y, M_x, M_z
        assert abs(F[k]) <= bound * br.EPS * EF[k], (k, float(F[k]), float(EF[k]))
    T, ET = np.asarray(a["T"][0], dtype=np.longdouble), np.asarray(ref["ET"][0])
    assert abs(T[1] - T[2]) <= bound * br.EPS * ET[1] and abs(T[4] - T[5]) <= bound * br.EPS * ET[4]


def test_mirror_identity():
    """A bridle symmetric about the x-z plane at a pose in that plane: F_y = M_x = M_z = 0 and equal leg tensions, within the
    envelope -- of the reference under 2^-4, of the model under the gate."""
    _mirror(br.evaluate, 2.0 ** -4)
    _mirror(bm.evaluate, br.GATE_C)


def _model_worst(seed=None):
    worst = {}
    for name, (rows, depth) in bc.ACCURACY.items():
        for ip, pose in enumerate(bc.POSES):
            res = bm.evaluate(rows[None], pose[None], depth, seed=seed)
            if res["flags"].any():
                worst[name, ip] = np.inf
                continue
            w = worst_multiples(res, reference(name, ip))
            worst[name, ip] = max(w.values())
            if seed is None:
                assert np.array_equal(res["line_out"][..., 6], np.asarray(reference(name, ip)["line_out"], dtype=float)[..., 6]), name
    return worst


def test_gate_constant_is_the_measured_one():
    worst = _model_worst()
    for (name, ip), v in worst.items():
        print("%-18s pose %d  worst multiple of eps Ek (fp64 model): %.3g" % (name, ip, v))
    w = max(worst.values())
    print("worst over the cases: %.4g -> gate %d" % (w, br.GATE_C))
    assert abs(w - br.GATE_WORST_CPU) <= 0.02 * br.GATE_WORST_CPU, (w, br.GATE_WORST_CPU)
    assert br.GATE_C == 2 ** int(np.ceil(np.log2(4 * br.GATE_WORST_CPU)))


@pytest.mark.parametrize("seed", bm.SEEDS)
def test_gate_rejects_seeded_errors(seed):
    worst = _model_worst(seed)
    hit = {k: v for k, v in worst.items() if v > br.GATE_C}
    print(seed, {k: ("%.3g" % v) for k, v in worst.items()})
    assert hit, (seed, worst)
    if seed == "junction_weight_dropped":                           # the cases with a weight or a buoy at the junction, both of them
        assert {k[0] for k in hit} >= {"clump", "buoy"}, hit


def test_flag_cases_poison_only_their_own_design():
    good = bc.ACCURACY["symmetric_200"][0]
    for name, (rows, depth, pose, flag) in bc.FLAGS.items():
        lines = np.stack([good, rows, good])
        poses = np.stack([bc.POSES[1], pose, bc.POSES[0]])
        for ev in (bm.evaluate, br.evaluate):
            res = ev(lines, poses, depth)
            want = [0, flag, 0]
            if depth != 200.0:                                      # (the neighbours are cases of 200 m of water: alone)
                res, want = ev(lines[1:2], poses[1:2], depth), [flag]
            assert list(res["flags"]) == want, (name, ev.__module__, res["flags"])
            bad = want.index(flag)
            assert np.all(np.isnan(np.asarray(res["C"][bad], dtype=float)))
            for d in range(len(want)):
                if d != bad:
                    assert np.all(np.isfinite(np.asarray(res["C"][d], dtype=float))) and np.all(np.isfinite(np.asarray(res["J"][d], dtype=float)))
        if depth == 200.0:
            alone, batch = bm.evaluate(lines[:1], poses[:1], depth), bm.evaluate(lines, poses, depth)
            assert np.array_equal(alone["C"][0], batch["C"][0]) and np.array_equal(alone["J"][0], batch["J"][0])


def test_mixed_design_takes_each_kind_through_its_own_path():
    """Bridle + chain + single line in one design: the chain and the single line contribute what the chain model gives them."""
    rows, depth = bc.mixed_design()
    res = bm.evaluate(rows[None], bc.POSES[1][None], depth)
    ref = br.evaluate(rows[None], bc.POSES[1][None], depth)
    assert not res["flags"].any() and not ref["flags"].any()
    assert max(worst_multiples(res, ref).values()) <= br.GATE_C
    b = bm.evaluate(rows[None, :3], bc.POSES[1][None], depth)
    c = bm.cdm.evaluate(rows[None, 3:], bc.POSES[1][None], depth)
    assert np.allclose(res["F"][0], b["F"][0] + c["F"][0], rtol=1e-13, atol=1e-6)
    assert np.array_equal(res["T"][0, 3:6], c["T"][0, :3]) and np.array_equal(res["J"][0, 9:12], c["J"][0, 3:6])


# ---- bridles_from_design
def _bridle_deck(legs=2):
    """The VolturnUS-S deck with line 1 ending in a bridle: a stem of two segments (a clump on its joint) to the junction
    ``j1`` (a buoy), and ``legs`` legs to vessel points of their own."""
    g = mc.golden()["VolturnUS-S"]
    design = copy.deepcopy(g["design"])
    moor = design["mooring"]
    moor["line_types"].append(dict(name="rope", diameter=0.2, mass_density=60.0, stiffness="5e8"))
    moor["points"] = [p for p in moor["points"] if p["name"] != "line1_vessel"]
    moor["points"] += [dict(name="mid1", type="free", location=[-400.0, 0.0, -150.0], m=20000.0, v=2.0),
                       dict(name="j1", type="connection", location=[-150.0, 0.0, -60.0], m=1000.0, v=10.0)]
    fair = [[-58.0, 20.0, -14.0], [-58.0, -20.0, -14.0], [-60.0, 0.0, -16.0]][:legs]
    for k, f in enumerate(fair):
        moor["points"].append(dict(name="fair1%s" % "abc"[k], type="vessel", location=f))
    lines = [ln for ln in moor["lines"] if ln["name"] != "line1"]
    # the legs first, one of them written from the vessel down: the order and the direction in the list do not matter
    lines.insert(0, dict(name="leg_a", endA="fair1a", endB="j1", type="rope", length=110))
    lines.append(dict(name="leg_b", endA="j1", endB="fair1b", type="chain", length=105))
    if legs > 2:
        lines.append(dict(name="leg_c", endA="j1", endB="fair1c", type="rope", length=108))
    lines.append(dict(name="stem_top", endA="mid1", endB="j1", type="rope", length=290))
    lines.append(dict(name="stem_bottom", endA="line1_anchor", endB="mid1", type="chain", length=420))
    moor["lines"] = lines
    return design, g["rho"], g["g"]


def test_bridles_from_design_accepts_a_bridle():
    for legs in (2, 3):
        design, rho, g = _bridle_deck(legs)
        recs, depth, names = bridles_from_design(design, rho, g)
        n = 2 + 2 + legs
        assert depth == 200.0 and recs.shape == (n, 16)
        # lines in the order of the list's anchor-side segments: line2, line3, then the bridle (stem, then legs in list order)
        assert names == ["line2", "line3", "stem_bottom", "stem_top", "leg_a", "leg_b"] + (["leg_c"] if legs > 2 else [])
        assert list(recs[:, ML_CONT]) == [0, 0, 0, 1] + [0] * legs and list(recs[:, ML_LEG]) == [0, 0, 0, 0] + [1] * legs
        w_chain = (685.0 - rho * np.pi / 4 * 0.185 ** 2) * g
        w_rope = (60.0 - rho * np.pi / 4 * 0.2 ** 2) * g
        head, top, la, lb = recs[2:6]
        assert list(head[0:3]) == [-837.0, 0.0, -200.0] and np.all(head[3:6] == 0) and (head[6], head[7], head[8]) == (420.0, 3270e6, w_chain)
        assert np.all(top[0:6] == 0) and (top[6], top[7], top[8]) == (290.0, 5e8, w_rope) and top[ML_WJOINT] == (20000.0 - rho * 2.0) * g
        assert list(la[3:6]) == [-58.0, 20.0, -14.0] and (la[6], la[7], la[8]) == (110.0, 5e8, w_rope) and np.all(la[0:3] == 0)
        assert la[ML_WJOINT] == (1000.0 - rho * 10.0) * g and la[ML_WJOINT] < 0                   # the junction is a buoy
        assert list(lb[3:6]) == [-58.0, -20.0, -14.0] and (lb[6], lb[7], lb[8]) == (105.0, 3270e6, w_chain) and lb[ML_WJOINT] == 0
        assert np.all(recs[:, 11:14] == 0) and np.all(recs[4:, 9] == 0)
        # the records solve, in the reference and in the model of the device
        ref = br.evaluate(recs[None], None, depth)
        assert ref["flags"][0] == 0 and bm.evaluate(recs[None], None, depth)["flags"][0] == 0
        # the program: a leg row has a fairlead only, the head row of a bridle an anchor only
        prog = MooringProgram(recs, 2)
        z, one = np.zeros((3, 3)), np.ones((3, 3))
        prog.ends(4, None, one)
        prog.ends(2, one, None)
        prog.ends(0, one, one)
        with pytest.raises(ValueError, match="leg row"):
            prog.ends(5, one, z)
        with pytest.raises(ValueError, match="heads a bridle"):
            prog.ends(2, z, one)
        with pytest.raises(ValueError, match="continuation row"):
            prog.ends(3, z, z)
        ex = prog.expand(np.array([[0.5, -1.0]]))
        assert np.all(ex[0, 4, 0:3] == 0) and np.all(ex[0, 4, 3:6] == 0.5) and np.all(ex[0, 2, 3:6] == 0) and np.all(ex[0, 2, 0:3] == 0.5)


def test_bridles_from_design_without_bridles_is_chains_from_design():
    for deck, g in mc.golden().items():
        a, da, na = bridles_from_design(g["design"], g["rho"], g["g"])
        b, db, nb = chains_from_design(g["design"], g["rho"], g["g"])
        assert np.array_equal(a, b) and da == db and na == nb, deck
    from tests.test_mooring_chains import _crc_deck
    design, rho, g = _crc_deck()
    a, b = bridles_from_design(design, rho, g), chains_from_design(design, rho, g)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def test_bridles_from_design_refusals():
    design, rho, g = _bridle_deck()

    def refused(edit, match, base=design):
        d = copy.deepcopy(base)
        edit(d["mooring"])
        with pytest.raises(UnsupportedFOWT, match=match):
            bridles_from_design(d, rho, g)

    def too_many_legs(m):
        for k in range(2):
            m["points"].append(dict(name="extra%d" % k, type="vessel", location=[-50.0, 5.0 * k, -14.0]))
            m["lines"].append(dict(name="x%d" % k, endA="j1", endB="extra%d" % k, type="chain", length=100))
    refused(too_many_legs, "at most %d legs" % MAX_LEG)

    def shared_anchor(m):
        m["points"].append(dict(name="fair9", type="vessel", location=[-50.0, 0.0, -14.0]))
        m["lines"].append(dict(name="second", endA="line2_anchor", endB="fair9", type="chain", length=900))
    refused(shared_anchor, "fixed mooring point 'line2_anchor' joins 2 lines: shared anchors")

    def shared_fairlead(m):
        [ln for ln in m["lines"] if ln["name"] == "leg_b"][0]["endB"] = "fair1a"
    refused(shared_fairlead, "vessel mooring point 'fair1a' joins 2 lines")

    def junction_to_junction(m):                                    # leg_b ends at a second junction with two legs of its own
        m["points"].append(dict(name="j2", type="free", location=[-100.0, -10.0, -40.0]))
        m["points"].append(dict(name="fair1c", type="vessel", location=[-58.0, -30.0, -14.0]))
        [ln for ln in m["lines"] if ln["name"] == "leg_b"][0]["endB"] = "j2"
        m["lines"] += [dict(name="y1", endA="j2", endB="fair1b", type="chain", length=50), dict(name="y2", endA="j2", endB="fair1c", type="chain", length=50)]
    refused(junction_to_junction, "joined to another junction")

    def leg_through_a_joint(m):                                     # a leg of two segments: legs run straight to the vessel
        m["points"].append(dict(name="k", type="free", location=[-100.0, -10.0, -40.0]))
        [ln for ln in m["lines"] if ln["name"] == "leg_b"][0]["endB"] = "k"
        m["lines"].append(dict(name="y1", endA="k", endB="fair1b", type="chain", length=50))
    refused(leg_through_a_joint, "do not end on the vessel")

    def two_anchors(m):                                             # a second path to a fixed point
        m["points"].append(dict(name="anchor9", type="fixed", location=[-837.0, 100.0, -200.0]))
        [ln for ln in m["lines"] if ln["name"] == "leg_b"][0]["endB"] = "anchor9"
    refused(two_anchors, "do not end on the vessel")

    def both_on_vessel(m):
        m["lines"].append(dict(name="u", endA="fair1a", endB="fair1b", type="chain", length=50))
    refused(both_on_vessel, "both ends on the vessel")
    refused(lambda m: m.__setitem__("file", "lines.dat"), "MoorDyn file")
    refused(lambda m: m.__setitem__("moorMod", 1), "moorMod")
    with pytest.raises(UnsupportedFOWT, match="no mooring section"):
        bridles_from_design({}, rho, g)
    # chains_from_design and lines_from_design still refuse the deck as a whole, in the words they always used
    with pytest.raises(UnsupportedFOWT, match="'j1' joins 3 lines: bridles and shared anchors or fairleads are not covered"):
        chains_from_design(design, rho, g)
    with pytest.raises(UnsupportedFOWT, match="free points are not covered"):
        lines_from_design(design, rho, g)
