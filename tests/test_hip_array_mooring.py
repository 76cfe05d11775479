"""Arrays with shared lines on the device (include/raftx_array_mooring.h) through the C-ABI: raftx_array_mooring_lines and
raftx_array_mean_pose on the cases of tests/array_mooring_cases.py against the longdouble reference of
tests/array_mooring_reference.py under its gates (GATE_C = 8 for C / F / T / J, from the fp64 model's worst 1.18 on the CPU;
GATE_POSE = 0.5 for the pose and the residual, from its worst 0.082; every case prints its own), the step counts against the
fp64 model, the outputs of the pose solve against raftx_array_mooring_lines bit for bit, nUnit = 1 and arrays without shared
rows against raftx_mooring_lines bit for bit, batch shapes and positions, flags, the errors raised before any launch and the farm
sweep with its own mooring system.  (The scratch of the new kernels: tests/test_array_mooring_code_object.py.)"""
import functools

import numpy as np
import pytest

from raft_amd import statics
from raft_amd._abi import RaftxError
from tests import array_mooring_cases as ac
from tests import array_mooring_device_model as adm
from tests import array_mooring_reference as ar
from tests import mean_pose_cases as mpc
from tests import mean_pose_reference as mpr
from tests import mooring_bridle_cases as bc
from tests import mooring_chain_cases as cc

pytestmark = pytest.mark.gpu
OUT = ("pose", "C", "F", "T", "J", "F_res", "iterations", "flags")
PAIRS = ("pair", "pair_thrust", "pair_yaw_pitch", "pair_shared_first")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def solve(ctx, b, **kw):
    return ctx.array_mean_pose(b["K_hs"], b["F0"], b["x_ref"], b["depth"], b["lines"], F_env=b["F_env"], **kw)


@functools.lru_cache(maxsize=None)
def model_iterations(name):
    c = ac.cases()[name]
    m = adm.solve(c["lines"], c["depth"], c["K_hs"], c["F0"], c["F_env"], c["x_ref"])
    assert m["flags"] == 0
    return m["iterations"]


@pytest.mark.parametrize("name", ac.NAMES)
def test_cases_against_the_reference(hip_ctx, name):
    """Measured on the MI355X, worst over the nine cases: C 1.09 and J 1.18 of eps E (square4 at x_ref: the model's own worst), T
    0.53, F 0.11; pose 0.082 of eps |K^-1| E_F and residual 0.051 of eps |E_F| (pair_thrust); the model's step count on every
    case; C, F, T, J of the pose solve equal to raftx_array_mooring_lines at the returned pose in every bit."""
    c = ac.cases()[name]
    b = ac.batch([name])
    ref = ac.reference(name)
    # the lines at the start pose
    at0 = hip_ctx.array_mooring_lines(b["lines"], b["x_ref"], b["depth"])
    assert at0["flags"][0] == 0
    w0 = ar.worst_multiples({k: at0[k][0] for k in "CFTJ"}, ar.evaluate(c["lines"], c["x_ref"], c["depth"]))
    # the pose
    res = solve(hip_ctx, b)
    assert res["flags"][0] == 0
    pm = float(ar.multiples(res["pose"][0].reshape(-1), ref["x"], ref["bound"]).max())
    rn = float(np.linalg.norm(res["F_res"][0]) / (ar.EPS * np.linalg.norm(ref["E_F"].astype(np.float64))))
    w1 = ar.worst_multiples({k: res[k][0] for k in "CFTJ"}, ar.evaluate(c["lines"], res["pose"][0], c["depth"]))
    print("%-18s C/F/T/J multiples of eps E: at x_ref %s, at the pose %s; pose %.3g of eps |K^-1| E_F; residual %.3g of eps |E_F|; "
          "%d steps (model %d)" % (name, {k: round(v, 2) for k, v in w0.items()}, {k: round(v, 2) for k, v in w1.items()}, pm, rn,
                                   res["iterations"][0], model_iterations(name)))
    assert max(w0.values()) <= ar.GATE_C and max(w1.values()) <= ar.GATE_C
    assert pm <= ar.GATE_POSE and rn <= ar.GATE_POSE
    assert res["iterations"][0] <= model_iterations(name) + 1
    # the outputs at the returned pose are those of raftx_array_mooring_lines there
    at = hip_ctx.array_mooring_lines(b["lines"], res["pose"], b["depth"], want=("C", "F", "T", "J"))
    assert at["flags"][0] == 0
    differ = [k for k in "CFTJ" if not same_bits(res[k], at[k])]
    assert not differ, (name, differ)


def test_single_unit_is_the_single_unit_path(hip_ctx):
    """nUnit = 1: raftx_array_mooring_lines has the bits of raftx_mooring_lines; raftx_array_mean_pose lies within the gate of
    raftx_mean_pose's reference and takes raftx_mean_pose's step count."""
    names = ["VolturnUS-S/unloaded", "VolturnUS-S/current", "VolturnUS-S/thrust"]
    b = mpc.batch(names)
    pose = np.array([np.zeros(6), [9.0, -6.0, 0.8, 0.02, -0.03, 0.17], [-4.0, 11.0, -0.5, -0.01, 0.02, -0.2]])
    one = hip_ctx.mooring_lines(b["lines"], b["depth"], pose=pose)
    arr = hip_ctx.array_mooring_lines(b["lines"], pose[:, None, :], b["depth"])
    assert not one["flags"].any()
    for k in ("C", "F", "T", "J", "line_out", "flags"):
        assert same_bits(one[k], arr[k]), k
    mp = hip_ctx.mean_pose(b["K_hs"], b["F0"], b["depth"], lines=b["lines"], F_env=b["F_env"], x_ref=b["x_ref"])
    res = hip_ctx.array_mean_pose(b["K_hs"][:, None], b["F0"][:, None], b["x_ref"][:, None], b["depth"], b["lines"], F_env=b["F_env"][:, None])
    assert not res["flags"].any() and np.array_equal(res["iterations"], mp["iterations"])
    for i, name in enumerate(names):
        ref = mpc.reference(name)
        mult = mpr.pose_multiples(res["pose"][i, 0], ref)
        print("%-28s nUnit = 1: pose multiples of eps |K^-1| E_F: worst %.3g (raftx_mean_pose %.3g)" % (
            name, mult.max(), mpr.pose_multiples(mp["pose"][i], ref).max()))
        assert np.all(mult <= mpr.GATE)


def _unshared_array(kind):
    """(rows of one unit, depth, poses [3,6]) for an array of three units without shared rows."""
    poses = np.array([[0.0, 0, 0, 0, 0, 0], [9.0, -6.0, 0.8, 0.02, -0.03, 0.17], [-5.0, 4.0, -0.4, -0.01, 0.02, -0.1]])
    if kind == "single":
        return mpc.decks()["VolturnUS-S"]["lines"], 200.0, poses
    if kind == "chains":
        return np.vstack([cc.crc(180.0), cc.crc(60.0), cc.single(300.0)]), cc.DEEP, poses
    rows, depth = bc.mixed_design()
    return rows, depth, poses


@pytest.mark.parametrize("kind", ["single", "chains", "bridles"])
def test_array_without_shared_rows(hip_ctx, kind):
    """... has the bits of raftx_mooring_lines per unit in its diagonal blocks and exact zeros off them (single rows, composite
    lines and bridles: the three instantiations of the kernels)."""
    from raft_amd import mooring
    rows, depth, poses = _unshared_array(kind)
    loc = np.array([[0.0, 0.0], [1600.0, 0.0], [800.0, 1400.0]])
    lines = mooring.array_lines([rows] * 3, loc)[None]
    x = poses.copy()
    x[:, :2] += loc
    arr = hip_ctx.array_mooring_lines(lines, x[None], depth)
    assert arr["flags"][0] == 0
    nR = len(rows)
    C = arr["C"][0].reshape(3, 6, 3, 6)
    for u in range(3):
        shifted = rows.copy()
        head = (rows[:, 15] == 0) & (rows[:, 14] == 0)
        shifted[head, 0:2] += loc[u]
        one = hip_ctx.mooring_lines(shifted[None], depth, pose=x[u][None])
        assert one["flags"][0] == 0
        assert same_bits(C[u, :, u, :], one["C"][0]) and same_bits(arr["F"][0, 6 * u:6 * u + 6], one["F"][0])
        for e in range(2):
            sl = slice(e * 3 * nR + u * nR, e * 3 * nR + (u + 1) * nR)
            assert same_bits(arr["T"][0, sl], one["T"][0, e * nR:(e + 1) * nR])
            assert same_bits(arr["J"][0, sl, 6 * u:6 * u + 6], one["J"][0, e * nR:(e + 1) * nR])
            for v in range(3):
                if v != u:
                    assert not arr["J"][0, sl, 6 * v:6 * v + 6].any()
        assert same_bits(arr["line_out"][0, u * nR:(u + 1) * nR], one["line_out"][0])
        for v in range(3):
            if v != u:
                assert not C[u, :, v, :].any() and not np.signbit(C[u, :, v, :]).any()


@pytest.mark.parametrize("kind", ["chains", "bridles"])
def test_shared_rows_beside_composite_lines_and_bridles(hip_ctx, kind):
    """The CHAINS and BRIDLES instantiations with a shared row among the rows: the pose solve's outputs are those of
    raftx_array_mooring_lines at the returned pose, bit for bit, and the shared row's blocks are those it has between single lines."""
    from raft_amd import mooring
    rows, depth, _ = _unshared_array(kind)
    d = mpc.decks()["VolturnUS-S"]
    loc = [(0.0, 0.0), (1600.0, 0.0)]
    sh = [dict(unitA=0, rA=(58.0, 0.0, -14.0), unitB=1, rB=(-58.0, 0.0, -14.0), **ac.SHARED)]
    lines = mooring.array_lines([rows, rows], loc, [0.0, 180.0], sh)[None]
    K_hs, F0 = np.broadcast_to(d["K_hs"], (1, 2, 6, 6)), np.broadcast_to(d["F0"], (1, 2, 6))
    r = statics.array_mean_pose(hip_ctx, K_hs, F0, lines, loc, depth, tol=(1e3, 1e3))      # one Newton step, then the outputs
    assert r.ok.all() and r.describe_flags(0) == [] and r.iterations[0] == 1 and np.abs(r.pose[0, :, :2] - np.asarray(loc)).max() > 0.1
    at = hip_ctx.array_mooring_lines(lines, r.pose, depth, want=("C", "F", "T", "J"))
    for k, v in (("C", r.C), ("F", r.F), ("T", r.T), ("J", r.J)):
        assert same_bits(v, at[k]), (kind, k)
    # the shared row's off-diagonal blocks against the same row alone at the same poses (the default instantiations: another
    # copy of the body, so to rounding)
    alone = mooring.array_lines([np.zeros((0, 16))] * 2, loc, shared=sh)[None]
    ref = hip_ctx.array_mooring_lines(alone, r.pose, depth, want=("C",))
    for blk in ((slice(0, 6), slice(6, 12)), (slice(6, 12), slice(0, 6))):
        assert np.allclose(at["C"][0][blk], ref["C"][0][blk], rtol=1e-10, atol=1e-10 * np.abs(ref["C"][0]).max())


def _nan_record_array():
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ac.cases()["pair"].items()}
    c["lines"][6, 6] = np.nan                                    # the shared row's length
    return c


def test_batch_shapes_positions_and_flags(hip_ctx):
    """nArray = 1, 2, 63, 65 of the pair-shaped cases: an array's bits are the same alone, at any position and beside flagged
    neighbours -- one pair_grounded array (GROUNDED rises mid-iteration) and one array with a NaN record stand among the good
    ones; only their own outputs are NaN, only their own flags are set, and iterations stays a count."""
    pool = [ac.cases()[n] for n in PAIRS]
    stack = lambda cs: dict({k: np.ascontiguousarray([c[k] for c in cs]) for k in ("lines", "K_hs", "F0", "F_env", "x_ref")}, depth=ac.DEPTH)
    alone = [solve(hip_ctx, stack([c])) for c in pool]
    alone_l = [hip_ctx.array_mooring_lines(c["lines"][None], a["pose"], ac.DEPTH) for c, a in zip(pool, alone)]
    assert not any(a["flags"][0] for a in alone)
    grounded, nanrec = ac.cases()["pair_grounded"], _nan_record_array()
    g_alone, n_alone = solve(hip_ctx, stack([grounded])), solve(hip_ctx, stack([nanrec]))
    assert g_alone["flags"][0] == 64 and g_alone["iterations"][0] >= 1
    assert n_alone["flags"][0] == 1 and n_alone["iterations"][0] == 0
    first = hip_ctx.array_mooring_lines(grounded["lines"][None], grounded["x_ref"][None], ac.DEPTH)
    assert first["flags"][0] == 0                                 # (unflagged at the start pose: the flag rises on the way)
    for n in (1, 2, 63, 65):
        for shift, special in ((0, {}), (1, {0: (grounded, g_alone), n // 2: (nanrec, n_alone)} if n > 1 else {0: (grounded, g_alone)})):
            idx = [(i + shift) % len(pool) for i in range(n)]
            cs = [special[i][0] if i in special else pool[idx[i]] for i in range(n)]
            res = solve(hip_ctx, stack(cs))
            for i in range(n):
                want = special[i][1] if i in special else alone[idx[i]]
                for k in OUT:
                    assert same_bits(res[k][i], want[k][0]), (n, shift, i, k)
            for i in special:
                assert all(np.all(np.isnan(res[k][i])) for k in ("pose", "C", "F", "T", "J", "F_res")) and res["iterations"][i] >= 0
            # the stand-alone evaluation at the solved poses, the flagged arrays at their start poses
            poses = np.array([cs[i]["x_ref"] if i in special else res["pose"][i] for i in range(n)])
            ev = hip_ctx.array_mooring_lines(stack(cs)["lines"], poses, ac.DEPTH)
            for i in range(n):
                if i in special:
                    if special[i][0] is nanrec:
                        assert ev["flags"][i] == 1 and all(np.all(np.isnan(ev[k][i])) for k in ("C", "F", "T", "J", "line_out"))
                    continue
                for k in ("C", "F", "T", "J", "line_out", "flags"):
                    assert same_bits(ev[k][i], alone_l[idx[i]][k][0]), (n, shift, i, k)


def test_null_outputs_and_tolerances(hip_ctx):
    b = ac.batch(["pair", "pair_thrust"])
    full = solve(hip_ctx, b)
    assert all(same_bits(solve(hip_ctx, b, tol=(1e-9, 1e-10), max_iter=40)[k], full[k]) for k in OUT)
    for k in OUT[:-1]:
        part = solve(hip_ctx, b, want=(k,))
        assert set(part) == {k, "flags"} and same_bits(part[k], full[k])
    capped = solve(hip_ctx, b, max_iter=2)
    assert np.all(capped["flags"] == statics.FLAG_POSE_CAP) and np.all(capped["iterations"] == 2) and np.all(np.isnan(capped["pose"]))
    lines = hip_ctx.array_mooring_lines(b["lines"], b["x_ref"], b["depth"])
    for k in ("C", "F", "T", "J", "line_out"):
        part = hip_ctx.array_mooring_lines(b["lines"], b["x_ref"], b["depth"], want=(k,))
        assert set(part) == {k, "flags"} and same_bits(part[k], lines[k])


def test_errors_before_any_launch(hip_ctx):
    b = ac.batch(["pair", "pair_thrust"])

    def edited(l, f, v):
        e = dict(b, lines=b["lines"].copy())
        e["lines"][1, l, f] = v
        return e

    for e, msg in ((edited(6, 12, 2.0), "both ends on unit"), (edited(6, 11, 2.0), "unit B = 2"), (edited(6, 11, 0.5), "unit B = 0.5"),
                   (edited(6, 12, 3.0), "unit A = 3"), (edited(6, 12, np.nan), "unit A"), (edited(2, 11, -1.0), "unit B = -1"),
                   (edited(6, 15, 1.0), "continues a shared row|continuation"), (edited(6, 14, 1.0), "bridle|leg"),
                   (edited(6, 10, 5.0), "joint weight"), (edited(6, 9, 0.3), "CB = 0.3"), (edited(1, 9, 0.3), "CB = 0.3")):
        for call in (lambda q: solve(hip_ctx, q), lambda q: hip_ctx.array_mooring_lines(q["lines"], q["x_ref"], q["depth"])):
            with pytest.raises(RaftxError, match=msg):
                call(e)
    cont_after_shared = dict(b, lines=np.concatenate([b["lines"], np.zeros((2, 1, 16))], axis=1))
    cont_after_shared["lines"][:, 7, 6:9] = (10.0, 1e8, 100.0)
    cont_after_shared["lines"][:, 7, 15], cont_after_shared["lines"][:, 7, 11] = 1.0, 1.0
    with pytest.raises(RaftxError, match="continues a shared row"):
        solve(hip_ctx, cont_after_shared)
    for depth in (-1.0, 0.0, np.nan, np.inf):
        with pytest.raises(RaftxError, match="depth"):
            solve(hip_ctx, dict(b, depth=depth))
    for tol in ((-1e-9, 1e-10), (1e-9, np.nan)):
        with pytest.raises(RaftxError, match="tolerances"):
            solve(hip_ctx, b, tol=tol)
    L = hip_ctx.rlib.lib
    ptr = lambda a: a.ctypes.data
    fl = np.zeros(2, dtype=np.int32)
    K, F0, xr, ln = b["K_hs"], b["F0"], b["x_ref"], b["lines"]

    def pose_call(nU=2, lines=ptr(ln), K=ptr(K), F=ptr(F0), x=ptr(xr), flags=ptr(fl), nA=2):
        return L.raftx_array_mean_pose(hip_ctx._h, nA, nU, 7, lines, 200.0, K, F, None, x, None, 0, None, None, None, None, None, None, None, flags)

    for kw in (dict(lines=None), dict(K=None), dict(F=None), dict(x=None), dict(flags=None)):
        assert pose_call(**kw) != 0 and b"required" in L.raftx_last_error(hip_ctx._h)
    for nU in (0, 7):
        assert pose_call(nU=nU) != 0 and b"nUnit must be 1 to 6" in L.raftx_last_error(hip_ctx._h)
    assert pose_call(nA=-1) != 0 and pose_call(nA=0) == 0
    assert pose_call() == 0 and not fl.any()

    def lines_call(lines=ptr(ln), pose=ptr(xr), flags=ptr(fl), nU=2):
        return L.raftx_array_mooring_lines(hip_ctx._h, 2, nU, 7, lines, pose, 200.0, None, None, None, None, None, flags)

    for kw in (dict(lines=None), dict(pose=None), dict(flags=None)):
        assert lines_call(**kw) != 0 and b"required" in L.raftx_last_error(hip_ctx._h)
    assert lines_call(nU=7) != 0 and lines_call() == 0


def test_farm_sweep_with_its_own_mooring(hip_ctx):
    """Sweep.run_farm(array_mooring=...) on two 2-unit farms with tiny tables: Xi is run_farm(Cc=C) bit for bit with C from the
    stand-alone entry, T_mean its T, T_std raftx_response_stats of J Xi; a caller's Cc is added."""
    from raft_amd.sweep import Sweep
    from tests.util import random_matrices, random_strips, synthetic_cases
    rng = np.random.default_rng(2024)
    nG, n_unit, nw = 2, 2, 96
    tables = [random_strips(rng, 8, nw, 0.0) for _ in range(nG * n_unit)]
    M0, B0, C0, _ = random_matrices(rng, nG * n_unit, nw, False)
    w, k, zeta, beta = synthetic_cases(rng, 2, 1, nw)
    off = np.concatenate([[0], np.cumsum([len(t.strips) for t in tables])]).astype(np.int64)
    sweep = Sweep(off, np.concatenate([t.strips for t in tables]), M0, B0, C0, w, k, 200.0, zeta, beta, 5, 0.1)
    b = ac.batch(["pair", "pair_thrust"])
    pose = solve(hip_ctx, b, want=("pose",))["pose"]
    moor = dict(lines=b["lines"], pose=pose, depth=b["depth"])
    out = sweep.run_farm(hip_ctx, n_unit, array_mooring=moor)
    at = hip_ctx.array_mooring_lines(b["lines"], pose, b["depth"])
    assert not out["moor_flags"].any() and same_bits(out["C_moor"], at["C"]) and same_bits(out["T_mean"], at["T"])
    ref = sweep.run_farm(hip_ctx, n_unit, Cc=at["C"])
    assert same_bits(out["Xi"], ref["Xi"]) and np.all(np.isfinite(out["Xi"].view(np.float64)))
    dw = float(w[1] - w[0])
    for g in range(nG):
        L = np.zeros((14, 3, 12))
        L[:, 0, :] = at["J"][g]
        for c in range(2):
            assert same_bits(out["T_std"][g, c], hip_ctx.response_stats(w, L, out["Xi"][g, c], dw)[0])
    assert out["T_std"].shape == (nG, 2, 14) and np.all(out["T_std"] > 0)
    extra = 1e4 * np.eye(12)[None]
    both = sweep.run_farm(hip_ctx, n_unit, Cc=extra, array_mooring=moor)
    assert same_bits(both["Xi"], sweep.run_farm(hip_ctx, n_unit, Cc=extra + at["C"])["Xi"]) and not same_bits(both["Xi"], out["Xi"])
