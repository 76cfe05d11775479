"""Bridle mooring lines on the device (include/raftx_mooring.h) through the C-ABI: raftx_mooring_lines on the cases of
tests/mooring_bridle_cases.py against the longdouble all-points reference of tests/mooring_bridle_reference.py under the gate
|x - ref| <= C eps Ek (C = 8, from the fp64 model on the CPU, whose worst is 1.79; every case prints its own), the
coincident-legs and mirror identities, the flag cases, a bridle across the workgroup boundary, bridles beside chains and single
lines, the record errors, the mooring program, the mean pose and one crossing of each rider."""
import numpy as np
import pytest

from raft_amd import geometry as G
from raft_amd._abi import RaftxError
from raft_amd.mooring import MooringProgram
from tests import mean_pose_cases as cs
from tests import mean_pose_reference as mpr
from tests import mooring_bridle_cases as bc
from tests import mooring_bridle_reference as br
from tests import mooring_cases as mc
from tests.test_mooring_bridles import _coincident, _mirror, reference, worst_multiples

pytestmark = pytest.mark.gpu
KEYS = ("C", "F", "T", "J", "line_out", "flags")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def device(ctx):
    return lambda lines, pose, depth: ctx.mooring_lines(lines, depth, pose=pose)


def test_cases_against_the_reference(hip_ctx):
    worst = 0.0
    for (depth, nrow), group in bc.accuracy_batch().items():
        lines = np.array([g[2] for g in group])
        pose = np.array([g[3] for g in group])
        res = hip_ctx.mooring_lines(lines, depth, pose=pose)
        assert not res["flags"].any(), res["flags"]
        for i, (name, ip, rows, _) in enumerate(group):
            ref = reference(name, ip)
            one = {k: res[k][i:i + 1] for k in KEYS}
            w = worst_multiples(one, ref)
            print("%-18s pose %d  worst multiples of eps Ek: %s" % (name, ip, {k: round(v, 3) for k, v in w.items()}))
            assert max(w.values()) <= br.GATE_C, (name, ip, w)
            worst = max(worst, max(w.values()))
            lo, lr = one["line_out"][0], np.asarray(ref["line_out"][0], dtype=float)
            assert np.array_equal(lo[:, 6], lr[:, 6]), name                                    # the branch
            assert np.all(lo[:, 5] == lo[0, 5]) and 1 <= lo[0, 5] < 60 and np.all(lo[:, 7] == 0), (name, lo[:, 5])
            ns = int(np.sum(rows[:, bc.ML_LEG] == 0))
            assert np.all(lo[ns:, 4] == 0)                                                     # a leg never rests
            LB = lr[0, 4]
            assert abs(lo[0, 4] - LB) * rows[0, 8] <= br.GATE_C * br.EPS * float(np.asarray(ref["ET"][0]).max()), name
    print("worst multiple over all cases: %.3g (gate %d)" % (worst, br.GATE_C))


def test_coincident_legs_identity(hip_ctx):
    for m in _coincident(device(hip_ctx)):
        print({k: "%.3g" % v for k, v in m.items()})
        assert max(m.values()) <= br.GATE_C, m


def test_mirror_identity(hip_ctx):
    _mirror(device(hip_ctx), br.GATE_C)


def test_flag_cases_poison_only_their_design(hip_ctx):
    good = bc.ACCURACY["symmetric_200"][0]
    for name, (rows, depth, pose, flag) in bc.FLAGS.items():
        if depth != 200.0:
            res = hip_ctx.mooring_lines(rows[None], depth, pose=pose[None])
            assert list(res["flags"]) == [flag], (name, res["flags"])
            assert all(np.all(np.isnan(res[k][0])) for k in ("C", "F", "T", "J", "line_out")), name
            continue
        lines = np.stack([good, rows, good])
        poses = np.stack([bc.POSES[1], pose, bc.POSES[0]])
        res = hip_ctx.mooring_lines(lines, depth, pose=poses)
        assert list(res["flags"]) == [0, flag, 0], (name, res["flags"])
        for i in (0, 2):
            alone = hip_ctx.mooring_lines(lines[i:i + 1], depth, pose=poses[i:i + 1])
            assert all(same_bits(alone[k][0], res[k][i]) for k in KEYS), (name, i)
        for k in ("C", "F", "T", "J", "line_out"):
            assert np.all(np.isnan(res[k][1])), (name, k)


def test_a_bridle_across_the_workgroup_boundary(hip_ctx):
    """52 designs x 5 rows = 260 lanes of 256-lane workgroups: design 51 has its stem's head row in lane 255 and its legs in
    the next workgroup.  Every design's bits are those it has alone."""
    base, depth = bc.bridle_two_singles()
    other = np.vstack([base[3:], base[:3]])                         # the bridle last: its rows at another offset in the workgroup
    lines = np.array([other if i % 4 == 1 else base for i in range(52)])
    assert 51 * 5 == 255 and lines[51, 0, bc.ML_LEG] == 0 and np.all(lines[51, 1:3, bc.ML_LEG] == 1)
    pose = np.array([bc.POSES[1] * (0.2 + 0.015 * i) for i in range(52)])
    full = hip_ctx.mooring_lines(lines, depth, pose=pose)
    assert not full["flags"].any()
    for i in (0, 1, 2, 50, 51):
        one = hip_ctx.mooring_lines(lines[i:i + 1], depth, pose=pose[i:i + 1])
        assert all(same_bits(one[k][0], full[k][i]) for k in KEYS), i


def test_bridles_beside_chains_and_single_lines(hip_ctx):
    """One batch with a bridle + chain + single design beside a design of chains and single lines and one of single lines
    only, six rows each: the designs without a leg row give, bit for bit, what a batch without any leg row gives them."""
    mixed, depth = bc.mixed_design()
    plain = np.vstack([mixed[3:], bc.turned(mixed[3:], 60.0)])      # chain + single, twice: six rows, no leg row
    singles = np.vstack([bc.turned(bc.single(bc.A200, (-40.0, 0.0, -14.0), 850.0, *bc.CHAIN), a) for a in (0, 60, 120, 180, 240, 300)])
    without = np.array([plain, singles])
    pose = np.array([bc.POSES[1], bc.POSES[1] * 0.5])
    want = hip_ctx.mooring_lines(without, depth, pose=pose)
    assert not want["flags"].any()
    both = hip_ctx.mooring_lines(np.array([mixed, plain, singles]), depth, pose=np.array([bc.POSES[1], pose[0], pose[1]]))
    assert not both["flags"].any()
    assert all(same_bits(both[k][1:], want[k]) for k in KEYS)
    ref = br.evaluate(mixed[None], bc.POSES[1][None], depth)
    w = worst_multiples({k: both[k][:1] for k in KEYS}, ref)
    assert max(w.values()) <= br.GATE_C, w


def test_record_errors_before_any_launch(hip_ctx):
    rows, depth = bc.ACCURACY["symmetric_200"]
    def refused(r, match):
        with pytest.raises(RaftxError, match=match):
            hip_ctx.mooring_lines(np.asarray(r)[None], depth)
    refused(rows[1:], "leg row that follows no head row")
    refused(rows[:2], "exactly one leg")
    refused(np.vstack([rows[:2], bc.single(bc.A200, bc.FL, 850.0, *bc.CHAIN)]), "exactly one leg")
    refused(np.vstack([rows, rows[1:], ]), "more than 3 legs")
    head = rows.copy()
    head[0, 3:6] = (-40.0, 0.0, -14.0)
    refused(head, "heads a bridle and has a fairlead")
    cb = rows.copy()
    cb[2, 9] = 0.5
    refused(cb, "CB = 0.5")
    five = bc.bridle(bc.A200, [(150.0,) + bc.CHAIN + (0.0,)] * 5, [(bc.FL, 110.0) + bc.CHAIN, (bc.FR, 110.0) + bc.CHAIN])
    refused(five, "more than 4 rows")
    both = rows.copy()
    both[1, bc.ML_CONT] = 1.0
    refused(both, "leg row and as a continuation row")
    # the second design's error names the second design
    with pytest.raises(RaftxError, match="design 1"):
        hip_ctx.mooring_lines(np.array([rows, np.vstack([rows[:2], rows[:1]])]), depth)


def _reference_pose(lines_d, depth, K_hs, F0, F_env):
    """The reference's own Newton solve of Y(x) = F0 + F_env - K_hs x + F_moor(x) = 0 (tests/mean_pose_reference.py's iteration
    with the bridle reference in place of the single-line one): the root, and the bound |K^-1| E_F of its components."""
    T = np.longdouble
    x, last = np.zeros(6), np.inf
    for it in range(40):
        m = br.evaluate(lines_d[None], x[None], depth)
        assert not m["flags"][0]
        Y = F0.astype(T) + F_env.astype(T) - K_hs.astype(T) @ x.astype(T) + m["F"][0]
        K = K_hs.astype(T) + m["C"][0]
        dX = mpr._solve(K, Y)
        size = float(np.max(np.abs(dX)))
        if size >= last or size == 0.0:
            break
        x, last = (x.astype(T) + dX).astype(np.float64), size
    E_F = np.abs(F0) + np.abs(F_env) + np.abs(K_hs) @ np.abs(x) + np.asarray(m["EF"][0])
    return dict(x=x.astype(T) + dX, bound=np.abs(np.linalg.inv(K.astype(np.float64))).astype(T) @ E_F)


def test_mean_pose(hip_ctx):
    """Bridle + 2 single lines (nLine = 5, a group of 8 lanes): the pose against the reference's own Newton solve, within the
    bridle gate of eps |K^-1| E_F (the pose error is K^-1 times the force error, which the gate bounds by C eps E_F), and
    C_moor, F_moor, T, J bit for bit those of raftx_mooring_lines at the returned pose.  Tolerances below the rounding floor,
    as in tests/test_hip_mooring_chains.py."""
    rows, depth = bc.bridle_two_singles()
    F_at_0 = br.evaluate(rows[None], None, depth)["F"][0].astype(np.float64)
    n = 5
    F0 = np.array([-(0.9 + 0.04 * i) * F_at_0 for i in range(n)])
    F_env = np.array([i * 0.02 * cs.thrust_load() for i in range(n)])
    lines = np.broadcast_to(rows, (n,) + rows.shape).copy()
    K = np.broadcast_to(cs.synthetic_K(), (n, 6, 6)).copy()
    tol = (1e-12, 1e-12)
    res = hip_ctx.mean_pose(K, F0, depth, lines=lines, F_env=F_env, x_ref=np.zeros((n, 6)), tol=tol)
    assert not res["flags"].any(), res["flags"]
    assert np.all(res["iterations"] >= 2)
    for i in (0, n - 1):
        ref = _reference_pose(rows, depth, K[i], F0[i], F_env[i])
        m = mpr._multiples(res["pose"][i], ref["x"], ref["bound"])
        print("design %d: %d steps, pose within %.3g eps |K^-1| E_F" % (i, res["iterations"][i], m.max()))
        assert m.max() <= br.GATE_C, (i, m)
    at = hip_ctx.mooring_lines(lines, depth, pose=res["pose"], want=("C", "F", "T", "J"))
    assert not at["flags"].any()
    for k in ("C", "F", "T", "J"):
        assert same_bits(res[k], at[k]), k
    one = hip_ctx.mean_pose(K[3:4], F0[3:4], depth, lines=lines[3:4], F_env=F_env[3:4], x_ref=np.zeros((1, 6)), tol=tol)
    assert all(same_bits(one[k][0], res[k][3]) for k in ("pose", "C", "F", "T", "J", "F_res", "iterations", "flags"))


def _c3_program():
    import json
    from raft_amd import snapshot as standin
    return G.volturnus_program(json.loads(standin.load_fixture("geom_units.npz")["c3_base_json"]))


def test_program_with_leg_row_edits(hip_ctx):
    hip_ctx.variant_program(_c3_program())
    rows = np.vstack([bc.ACCURACY["chain_rope_600"][0], bc.turned(bc.single(bc.A600, (-40.0, 0.0, -14.0), 1750.0, *bc.ROPE), 120.0)])
    rng = np.random.default_rng(11)
    prog = MooringProgram(rows, 5)

    def coef(l, fields):
        c = np.zeros((6, 6))
        c[:, 0] = rows[l, :6]
        c[fields, 1:] = rng.normal(size=(len(fields), 5)) * 0.5
        return c
    c = coef(0, [0, 1])
    prog.ends(0, c[:3], None)                                        # the bridle's anchor moves
    for l in (2, 3):
        c = coef(l, [3, 4])
        prog.ends(l, None, c[3:])                                    # the legs' fairleads follow the columns
    c = coef(4, [0, 1, 3, 4])
    prog.ends(4, c[:3], c[3:])
    hip_ctx.mooring_program(prog)
    params = rng.uniform(-1, 1, (65, 5))
    got = hip_ctx.mooring_expand(params)
    assert same_bits(got, prog.expand(params))
    assert same_bits(got[:, 1], np.broadcast_to(rows[1], (65, 16)).copy())
    assert np.all(got[:, 0, 3:6] == 0) and np.all(got[:, 2:4, 0:3] == 0) and np.all(got[:, 2:4, bc.ML_LEG] == 1)
    res = hip_ctx.mooring_lines(got[:4], 600.0)
    ref = br.evaluate(got[:4], None, 600.0)
    assert not res["flags"].any() and max(worst_multiples(res, ref).values()) <= br.GATE_C
    # an edit of fields 0-2 of a leg row, of fields 3-5 of a bridle's head row
    bad = MooringProgram(rows, 5)
    bad.edit[2] = 1
    bad.coef[2, 1, 0] = 3.0
    with pytest.raises(RaftxError, match="row 2, a leg row of a bridle, has a coefficient for field 1"):
        hip_ctx.mooring_program(bad)
    bad = MooringProgram(rows, 5)
    bad.edit[0] = 1
    bad.coef[0, :3, 0] = rows[0, :3]
    bad.coef[0, 4, 2] = 0.1
    with pytest.raises(RaftxError, match="row 0, the head row of a bridle, has a coefficient for field 4"):
        hip_ctx.mooring_program(bad)
    with pytest.raises(RaftxError, match="exactly one leg"):
        hip_ctx.mooring_program(MooringProgram(rows[[0, 1, 2, 4]], 5))
    hip_ctx.mooring_program(None)


def _crossing_lines(n):
    g = mc.golden()["VolturnUS-S"]
    rows = bc.deck_bridles(g["lines"])                               # 3 bridles x 3 rows
    lines = np.broadcast_to(rows, (n,) + rows.shape).copy()
    lines[:, 1, bc.ML_WJOINT] = np.linspace(0.0, 1.0e5, n)           # a clump of its own at each design's first junction
    return lines


def test_one_crossing_with_bridles(hip_ctx):
    """Three C3 variants and the fixture's sea state with every line of the deck ending in a two-leg bridle: add_stiffness is bit
    for bit the crossing fed C0 + C_moor, and T_std is the channel kernel on J (as test_one_crossing_with_chains)."""
    from tests.test_hip_modal import _variant_sweep
    from tests.test_hip_sweep_channels import reference as chan_reference, within
    from tests.test_hip_sweep_mooring import BITS, DEPTH, run
    n = 3
    lines = _crossing_lines(n)
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
    within(chan_reference(sw.w, LJ, None, got["Xi"]), got["T_std"], 1, "bridles: T_std")
    assert same_bits(got["T_std"], chan["chan_std"])


def test_one_mean_pose_crossing_with_bridles(hip_ctx):
    """... and the crossing at every design's mean pose: the stand-alone composition (resident build, hydrostatics,
    raftx_mean_pose, the crossing with pose=) bit for bit, as tests/test_hip_sweep_mean_pose.py checks single lines."""
    from tests.test_hip_modal import _variant_sweep
    from tests.test_hip_sweep_mean_pose import assert_composition, host_route, request
    n = 3
    lines = _crossing_lines(n)
    sw = _variant_sweep(n)
    res, want = host_route(hip_ctx, sw, lines)
    got = sw.wait_crossing(hip_ctx, sw.submit_crossing(hip_ctx, 0, n_chunk=1, want_Xi=True, modal=True, mean_pose=request(dict(lines=lines), n)))
    assert_composition(got, res, want, "bridles")
