"""Composite mooring lines on the device (include/raftx_mooring.h) through the C-ABI: raftx_mooring_lines on the cases of
tests/mooring_chain_cases.py against the longdouble joint-position reference of tests/mooring_chain_reference.py under the gate
|x - ref| <= C eps Ek (C = 32, from the fp64 model on the CPU, whose worst is 4.28; every batch prints its own), the split
identity against the single-line reference, the flag cases, chains across the workgroup boundary, the mooring program, the
mean pose and one crossing."""
import numpy as np
import pytest

from raft_amd import geometry as G
from raft_amd._abi import RaftxError
from raft_amd.mooring import MooringProgram
from tests import mean_pose_cases as cs
from tests import mean_pose_reference as mpr
from tests import mooring_cases as mc
from tests import mooring_chain_cases as cc
from tests import mooring_chain_reference as cr

pytestmark = pytest.mark.gpu
KEYS = ("C", "F", "T", "J", "line_out", "flags")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_cases_against_the_reference(hip_ctx):
    worst = 0.0
    for name, lines, pose, depth in cc.batches():
        ref = cc.reference()[name]
        res = hip_ctx.mooring_lines(lines, depth, pose=pose)
        assert np.array_equal(res["flags"], ref["flags"]) and not res["flags"].any(), (name, res["flags"])
        w = cc.worst_multiples(res, ref)
        print("%-28s kappa %.3g  worst multiples of eps Ek: %s" % (name, ref["kappa"].max(), {k: round(v, 2) for k, v in w.items()}))
        assert max(w.values()) <= cr.GATE_C, (name, w)
        worst = max(worst, max(w.values()))
        # line_out: HF, V_top, HA, V_bottom and L_B w as forces, against max(HF, |V_top|) + the weight of the whole line
        lo, lr = res["line_out"], np.asarray(ref["line_out"], dtype=float)
        assert np.array_equal(lo[..., 6], lr[..., 6]), name                                    # the branch
        assert np.all(lo[..., 5] >= 1) and np.all(lo[..., 5] < 60) and np.all(lo[..., 7] == 0), name
        for a, n in cr.chains_of(lines[0]):
            assert np.all(lo[:, a:a + n, 5] == lo[:, a:a + 1, 5]), name                        # the head's iteration count
        k1 = 1 + ref["kappa"][..., None]
        a, b = lo[..., :5].copy(), lr[..., :5].copy()
        a[..., 4] *= lines[..., 8]
        b[..., 4] *= lines[..., 8]
        Wline = np.zeros(lines.shape[:2])
        for s, n in cr.chains_of(lines[0]):
            Wline[:, s:s + n] = (np.abs(lines[:, s:s + n, 8] * lines[:, s:s + n, 6]) + np.abs(lines[:, s:s + n, cr.ML_WJOINT])).sum(axis=1, keepdims=True)
        E = np.abs(lr[..., :2]).max(axis=-1) + Wline
        m = np.abs(a - b) / (cr.EPS * k1 * E[..., None])
        assert m.max() <= cr.GATE_C, (name, float(m.max()))
    print("worst multiple over all batches: %.3g (gate %d)" % (worst, cr.GATE_C))


def test_split_identity(hip_ctx):
    """A line cut into rows of its own EA and w with weightless joints against the single-line reference of the uncut line:
    C, F, and T, J at the anchor (end A of the head row) and the fairlead (end B of the last row)."""
    for name, lines, pose, depth, recs in cc.split_batches():
        res, one = hip_ctx.mooring_lines(lines, depth, pose=pose), cc.split_reference()[name]
        assert not res["flags"].any()
        k, nR, nL = len(cc.SPLITS[int(name[-1])]), lines.shape[1], len(recs)
        first, last = np.arange(nL) * k, nR + np.arange(nL) * k + (k - 1)
        for q in ("C", "F"):
            m = cr.gate_multiples(res[q], one[q], one["E" + q]).max()
            assert m <= cr.GATE_C, (name, q, m)
        for q in ("T", "J"):
            got = np.concatenate([res[q][:, first], res[q][:, last]], axis=1)
            m = cr.gate_multiples(got, one[q], one["E" + q]).max()
            assert m <= cr.GATE_C, (name, q, m)


def test_flag_cases_poison_only_their_design(hip_ctx):
    for name, lines, depth, flag in cc.flag_cases():
        res = hip_ctx.mooring_lines(lines, depth)
        assert list(res["flags"]) == [0, flag, 0], (name, res["flags"])
        for i in (0, 2):
            alone = hip_ctx.mooring_lines(lines[i:i + 1], depth)
            assert all(same_bits(alone[k][0], res[k][i]) for k in KEYS), (name, i)
        for k in ("C", "F", "T", "J", "line_out"):
            assert np.all(np.isnan(res[k][1])), (name, k)


def test_chains_across_the_workgroup_boundary(hip_ctx):
    """90 designs x 3 rows = 270 lanes of 256-lane workgroups: the chain of design 85 has its head row in lane 255 and its
    continuation rows in the next workgroup.  Every design's bits are those it has alone."""
    pool = [cc.crc(), cc.crc(150.0, W1=3.0e5), cc.crc(60.0, L=(600.0, 1000.0, 150.0), W1=2.0e5, W2=-1.2e6),
            np.concatenate([cc.single(180.0), cc.chain_rope(60.0)]), np.concatenate([cc.chain_rope(-60.0), cc.single(60.0)])]
    n = 90
    lines = np.array([pool[i % len(pool)] for i in range(n)])
    pose = np.tile(cc.POSES, (n // 4 + 1, 1))[:n]
    full = hip_ctx.mooring_lines(lines, cc.DEEP, pose=pose)
    assert not full["flags"].any()
    for i in (0, 1, 2, 3, 4, 84, 85, 86, 89):
        one = hip_ctx.mooring_lines(lines[i:i + 1], cc.DEEP, pose=pose[i:i + 1])
        assert all(same_bits(one[k][0], full[k][i]) for k in KEYS), i


def test_single_rows_in_a_batch_with_chains(hip_ctx):
    """A single line gives the same bits whether or not the batch holds a composite line (the chain kernels' single path
    against the single-row kernels')."""
    g = mc.golden()["VolturnUS-S"]
    singles = np.broadcast_to(g["lines"], (4, 3, 16)).copy()
    plain = hip_ctx.mooring_lines(singles, g["depth"], pose=mc.POSES)
    mixed = np.concatenate([singles, cc.split_batches()[1][1][:, :3]])
    both = hip_ctx.mooring_lines(mixed, g["depth"], pose=np.concatenate([mc.POSES, mc.POSES]))
    assert not both["flags"].any()
    assert all(same_bits(both[k][:4], plain[k]) for k in KEYS)


def _program_base():
    rows = np.concatenate([cc.crc(180.0, W1=3.0e5), cc.single(60.0), cc.chain_rope(-60.0)])
    return rows


def test_program_with_a_chain_base(hip_ctx):
    import json
    from raft_amd import snapshot as standin
    vp = G.volturnus_program(json.loads(standin.load_fixture("geom_units.npz")["c3_base_json"]))
    hip_ctx.variant_program(vp)
    rows = _program_base()
    rng = np.random.default_rng(5)
    prog = MooringProgram(rows, 5)
    for l in (0, 3, 4):                                          # the head rows and the single line
        c = np.zeros((6, 6))
        c[:, 0] = rows[l, :6]
        c[[0, 1, 3, 4], 1:] = rng.normal(size=(4, 5)) * 0.5          # x and y move; the anchors stay on the seabed
        prog.ends(l, c[:3], c[3:])
    hip_ctx.mooring_program(prog)
    params = rng.uniform(-1, 1, (65, 5))
    got = hip_ctx.mooring_expand(params)
    assert same_bits(got, prog.expand(params))
    for l in (1, 2, 5):                                          # the continuation rows are carried as they are
        assert same_bits(got[:, l], np.broadcast_to(rows[l], (65, 16)).copy())
    res = hip_ctx.mooring_lines(got[:4], cc.DEEP)
    ref = cr.evaluate(got[:4], None, cc.DEEP)
    assert not res["flags"].any() and max(cc.worst_multiples(res, ref).values()) <= cr.GATE_C
    # an edit on a continuation row, a continuation row first, a chain of five rows
    bad = MooringProgram(rows, 5)
    bad.edit[1] = 1
    with pytest.raises(RaftxError, match="continuation row"):
        hip_ctx.mooring_program(bad)
    with pytest.raises(RaftxError, match="row 0 is a continuation row"):
        hip_ctx.mooring_program(MooringProgram(rows[1:], 5))
    five = np.concatenate([rows[:3], rows[1:3]])
    with pytest.raises(RaftxError, match="more than 4 rows"):
        hip_ctx.mooring_program(MooringProgram(five, 5))
    hip_ctx.mooring_program(None)
    # ... and the same record errors in the stateless entry, before any launch
    with pytest.raises(RaftxError, match="row 0 of design 1 is a continuation row"):
        hip_ctx.mooring_lines(np.array([rows[:3], rows[1:4]]), cc.DEEP)
    with pytest.raises(RaftxError, match="more than 4 rows"):
        hip_ctx.mooring_lines(five[None], cc.DEEP)
    fr = rows[None].copy()
    fr[0, 1, 9] = 0.25
    with pytest.raises(RaftxError, match="CB = 0.25"):
        hip_ctx.mooring_lines(fr, cc.DEEP)


@pytest.mark.parametrize("layout", ["chain of 3", "chain of 3 + 2 singles"])
def test_mean_pose(hip_ctx, layout):
    """nLine = 3 (a group of 4 lanes) and nLine = 5 (a group of 8): the residual at the returned pose within the bound of
    tests/test_hip_mean_pose.py, ||Y|| <= GATE eps ||E_F|| with E_F = |F0| + |F_env| + |K_hs| |x - x_ref| + EF of the chain
    reference at that pose, and C_moor, F_moor, T, J bit for bit those of raftx_mooring_lines there.
    The bound is one on the rounding floor, so the solve is given tolerances below it (1e-12 m, 1e-12 rad).  The iteration
    converges linearly near the root (C_moor is the derivative for a rotation VECTOR, the pose holds angles: a rate of about the
    angles' size, 1e-3 here), and with the default tolerances it may stop right after a step that was just inside them: the
    third design then stops on a 5e-11 m step with 4.83 eps |E_F| left -- the fp64 model of the same iteration, on the CPU,
    stops there too with 4.84 -- and one more step takes it to 0.004."""
    rows = cc.crc(180.0, W1=1.0e5) if layout == "chain of 3" else np.concatenate([cc.single(60.0), cc.crc(180.0, W1=1.0e5), cc.single(-60.0)])
    F_at_0 = cr.evaluate(rows[None], None, cc.DEEP)["F"][0].astype(np.float64)
    n = 5
    F0 = np.array([-(0.9 + 0.04 * i) * F_at_0 for i in range(n)])
    F_env = np.array([i * 0.02 * cs.thrust_load() for i in range(n)])
    lines = np.broadcast_to(rows, (n,) + rows.shape).copy()
    K = np.broadcast_to(cs.synthetic_K(), (n, 6, 6)).copy()
    tol = (1e-12, 1e-12)
    res = hip_ctx.mean_pose(K, F0, cc.DEEP, lines=lines, F_env=F_env, x_ref=np.zeros((n, 6)), tol=tol)
    assert not res["flags"].any(), res["flags"]
    assert np.all(res["iterations"] >= 2)
    ref = cr.evaluate(lines, res["pose"], cc.DEEP)
    assert not ref["flags"].any()
    for i in range(n):
        E_F = np.abs(F0[i]) + np.abs(F_env[i]) + np.abs(K[i]) @ np.abs(res["pose"][i]) + ref["EF"][i].astype(np.float64)
        rn = float(np.linalg.norm(res["F_res"][i]) / (mpr.EPS * np.linalg.norm(E_F)))
        print("%s, design %d: %d steps, residual %.3g of eps |E_F|" % (layout, i, res["iterations"][i], rn))
        assert rn <= mpr.GATE, (layout, i, rn)
    at = hip_ctx.mooring_lines(lines, cc.DEEP, pose=res["pose"], want=("C", "F", "T", "J"))
    assert not at["flags"].any()
    for k in ("C", "F", "T", "J"):
        assert same_bits(res[k], at[k]), (layout, k)
    assert max(cc.worst_multiples(at, ref).values()) <= cr.GATE_C
    # a design alone has the bits it has in the batch
    one = hip_ctx.mean_pose(K[3:4], F0[3:4], cc.DEEP, lines=lines[3:4], F_env=F_env[3:4], x_ref=np.zeros((1, 6)), tol=tol)
    assert all(same_bits(one[k][0], res[k][3]) for k in ("pose", "C", "F", "T", "J", "F_res", "iterations", "flags"))


def test_one_crossing_with_chains(hip_ctx):
    """Three C3 variants and the fixture's sea state with the deck's lines cut into chain - chain - chain rows, a clump on one
    joint: add_stiffness is bit for bit the crossing fed C0 + C_moor, and T_std is the channel kernel on J (as
    tests/test_hip_sweep_mooring.py checks single lines)."""
    from tests.test_hip_modal import _variant_sweep
    from tests.test_hip_sweep_channels import reference, within
    from tests.test_hip_sweep_mooring import BITS, DEPTH, run
    n = 3
    g = mc.golden()["VolturnUS-S"]
    assert DEPTH == g["depth"]
    rows = cc.split_batches()[1][1][0].copy()                    # 3 lines x 3 rows
    lines = np.broadcast_to(rows, (n,) + rows.shape).copy()
    lines[:, 1, cr.ML_WJOINT] = [0.0, 5.0e4, 1.0e5]
    sw = _variant_sweep(n)
    m = hip_ctx.mooring_lines(lines, DEPTH)
    assert not m["flags"].any()
    C_base = sw.C0
    sw.C0 = C_base + m["C"]
    want = run(hip_ctx, sw)
    LJ = np.zeros((n, m["J"].shape[1], 3, 6))
    LJ[:, :, 0, :] = m["J"]
    chan = run(hip_ctx, sw, channels=dict(L=LJ))
    sw.C0 = C_base
    got = run(hip_ctx, sw, mooring=dict(lines=lines))
    assert not got["moor_flags"].any()
    for k in BITS:
        assert same_bits(got[k], want[k]), k
    assert same_bits(got["C_moor"], m["C"]) and same_bits(got["F_moor"], m["F"]) and same_bits(got["T_mean"], m["T"])
    assert got["T_std"].shape == (n, 1, 18) and np.all(got["T_std"] > 0)
    within(reference(sw.w, LJ, None, got["Xi"]), got["T_std"], 1, "chains: T_std")
    assert same_bits(got["T_std"], chan["chan_std"])
