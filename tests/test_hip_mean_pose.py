"""The mean equilibrium pose on the device (include/raftx_statics.h) through the C-ABI: raftx_mean_pose on the cases of
tests/mean_pose_cases.py against the longdouble root of tests/mean_pose_reference.py under the gate
|x - x*|_i <= GATE eps (|K^-1| E_F)_i (GATE = 2, from the fp64 model on the CPU, whose worst is 0.26; worst measured on the
MI355X 0.28, worst residual 0.20 eps |E_F|; every case prints its own), iteration counts against the fp64 model, the residual, the outputs at the returned pose against
raftx_mooring_lines bit for bit, batch shapes and positions, the mooring program, flags, and the errors raised before any
launch."""
import functools
import json

import numpy as np
import pytest

from raft_amd import geometry as G
from raft_amd import snapshot as standin
from raft_amd import statics
from raft_amd._abi import RaftxError
from tests import mean_pose_cases as cs
from tests import mean_pose_device_model as mdm
from tests import mean_pose_reference as mpr
from tests import mooring_cases as mc
from tests import mooring_reference as mr

pytestmark = pytest.mark.gpu
OUT = ("pose", "C", "F", "T", "J", "F_res", "iterations", "flags")
SIZES = (1, 63, 65, 257)
DECKS_200 = [d + "/" + f for d in ("VolturnUS-S", "VolturnUS-S-pointInertia", "OC4semi-WAMIT_Coefs") for f in ("unloaded", "current", "thrust")]
GROUPS = {"decks, 200 m": DECKS_200, "OC3spar": ["OC3spar/" + f for f in ("unloaded", "current", "thrust")],
          "single lines": ["single/" + n for n in cs.SINGLE], "x_ref": ["x_ref"], "four lines": ["four_lines"]}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def run(ctx, b, **kw):
    return ctx.mean_pose(b["K_hs"], b["F0"], b["depth"], lines=b["lines"], F_env=b["F_env"], x_ref=b["x_ref"], **kw)


@functools.lru_cache(maxsize=None)
def model_iterations(name):
    c = cs.cases()[name]
    m = mdm.solve(c["lines"], c["depth"], c["K_hs"], c["F0"], c["F_env"], c["x_ref"])
    assert m["flags"] == 0
    return m["iterations"]


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_cases_against_the_reference(hip_ctx, group):
    """Measured on the MI355X: worst pose multiple 0.281 (surge of VolturnUS-S, unloaded), worst residual 0.201 eps |E_F|
    (OC3spar under the thrust-like load), the model's step count on every case."""
    names = GROUPS[group]
    b = cs.batch(names)
    res = run(hip_ctx, b)
    assert not res["flags"].any(), res["flags"]
    worst = 0.0
    for i, name in enumerate(names):
        ref = cs.reference(name)
        mult = mpr.pose_multiples(res["pose"][i], ref)
        rn = float(np.linalg.norm(res["F_res"][i]) / (mpr.EPS * np.linalg.norm(ref["E_F"].astype(np.float64))))
        print("%-36s pose multiples of eps |K^-1| E_F: worst %.3g; residual %.3g of eps |E_F|; %d steps (model %d)"
              % (name, mult.max(), rn, res["iterations"][i], model_iterations(name)))
        assert np.all(mult <= mpr.GATE), (name, mult)
        assert rn <= mpr.GATE, (name, rn)
        assert res["iterations"][i] <= model_iterations(name) + 1, name
        worst = max(worst, float(mult.max()))
    print("%s: worst pose multiple %.3g (gate %d)" % (group, worst, mpr.GATE))
    # the outputs at the returned pose are those of raftx_mooring_lines there
    at = hip_ctx.mooring_lines(b["lines"], b["depth"], pose=res["pose"], want=("C", "F", "T", "J"))
    assert not at["flags"].any()
    for k in ("C", "F", "T", "J"):
        assert same_bits(res[k], at[k]), (group, k)


def _slack_design(n_line):
    """A design whose first line goes slack mid-iteration (tests/test_mean_pose.py): flag 4 after some steps."""
    rec, depth = mc.single_lines()["contact"]
    other = mc.single_lines()["no_contact"][0]
    lines = np.array([rec] + [other] * (n_line - 1))
    return dict(lines=lines, K_hs=cs.synthetic_K(), F0=np.array([-4.0e7, 0, 0, 0, 0, 0]), F_env=np.zeros(6), x_ref=np.zeros(6))


def _pool(n_line):
    """Designs of n_line lines at 200 m depth: the cases of that line count and copies of them under other loads."""
    names = {1: GROUPS["single lines"], 3: DECKS_200 + ["x_ref"], 4: ["four_lines"]}[n_line]
    pool = [cs.cases()[n] for n in names]
    for c in list(pool[:3]):
        for s in (0.5, -0.7):
            e = dict(c)
            e["F_env"] = c["F_env"] + s * cs.thrust_load() * (0.02 if n_line == 1 else 1.0)
            pool.append(e)
    return pool


@pytest.mark.parametrize("n_line", [1, 3, 4])
def test_batch_sizes_and_positions(hip_ctx, n_line):
    """A design's bits are the same alone, at any position of any batch size, and beside a flagged neighbour."""
    pool = _pool(n_line)
    stack = lambda ds: dict({k: np.ascontiguousarray([d[k] for d in ds]) for k in ("lines", "K_hs", "F0", "F_env", "x_ref")}, depth=200.0)
    alone = [run(hip_ctx, stack([d])) for d in pool]
    assert not any(a["flags"][0] for a in alone)
    assert len({int(a["iterations"][0]) for a in alone}) > 1        # designs of one wavefront finish at different steps
    bad = _slack_design(n_line)
    bad_alone = run(hip_ctx, stack([bad]))
    assert bad_alone["flags"][0] == 4 and bad_alone["iterations"][0] >= 2
    for n in SIZES:
        for shift, flagged in ((0, ()), (1, (0, n // 2, n - 1))):
            idx = [(i + shift) % len(pool) for i in range(n)]
            ds = [bad if i in flagged else pool[idx[i]] for i in range(n)]
            res = run(hip_ctx, stack(ds))
            for i in range(n):
                want = bad_alone if i in flagged else alone[idx[i]]
                for k in OUT:
                    assert same_bits(res[k][i], want[k][0]), (n, shift, i, k)
            for i in flagged:
                assert all(np.all(np.isnan(res[k][i])) for k in ("pose", "C", "F", "T", "J", "F_res"))


def _programs():
    base = json.loads(standin.load_fixture("geom_units.npz")["c3_base_json"])
    moor = mc.golden()["VolturnUS-S"]["design"]
    return G.volturnus_program(base), G.volturnus_mooring_program(moor)


def test_mooring_program_gives_the_bits_of_the_explicit_records(hip_ctx):
    vp, mp = _programs()
    hip_ctx.variant_program(vp)
    hip_ctx.mooring_program(mp)
    n = 65
    params = np.ascontiguousarray(G.volturnus_params(np.random.default_rng(5).uniform(0.75, 1.25, (n, 5))), dtype=float)
    d = cs.decks()["VolturnUS-S"]
    K_hs, F0 = np.broadcast_to(d["K_hs"], (n, 6, 6)).copy(), np.broadcast_to(d["F0"], (n, 6)).copy()
    F_env = np.broadcast_to(cs.thrust_load(), (n, 6)) * np.linspace(0.2, 1.0, n)[:, None]
    lines = hip_ctx.mooring_expand(params)
    a = hip_ctx.mean_pose(K_hs, F0, 200.0, lines=lines, F_env=F_env)
    b = hip_ctx.mean_pose(K_hs, F0, 200.0, params=params, F_env=F_env)
    assert not a["flags"].any() and np.ptp(a["pose"][:, 0]) > 1.0
    assert all(same_bits(a[k], b[k]) for k in OUT)
    r = statics.mean_pose(hip_ctx, K_hs, F0, depth=200.0, program=mp, params=params, F_env=F_env)
    assert same_bits(r.pose, a["pose"]) and same_bits(r.T, a["T"]) and r.ok.all()
    with pytest.raises(RaftxError, match="nLine=2"):
        L = hip_ctx.rlib.lib
        ptr = lambda x: x.ctypes.data
        fl = np.zeros(n, dtype=np.int32)
        hip_ctx._check(L.raftx_mean_pose(hip_ctx._h, n, 2, None, ptr(params), 200.0, ptr(K_hs), ptr(F0), None, None, None, 0,
                                         None, None, None, None, None, None, None, ptr(fl)), "raftx_mean_pose")
    hip_ctx.mooring_program(None)
    with pytest.raises(RaftxError, match="no program"):
        hip_ctx.mean_pose(K_hs, F0, 200.0, params=params)


def test_hydrostatics_helper_feeds_the_solve(hip_ctx):
    """raft_amd.statics.hydrostatics on a resident set of six variants: K_hs and F0 are the fetched statics plus the
    caller's terms, ``current=`` is raftx_current_loads of that one current; the solve on them balances the loads."""
    from tests.test_hip_modal import _variant_sweep
    n = 6
    sw = _variant_sweep(n)
    sw.upload(hip_ctx)
    st = hip_ctx.fetch_statics()
    C_extra, F_extra = np.diag([0, 0, 0, 2.0e9, 2.0e9, 0.0]), np.array([0, 0, -1.0e5, 0, 0, 0])
    cur = dict(speed=0.6, heading=15.0, depth=sw.depth)
    K_hs, F0, F_env = statics.hydrostatics(hip_ctx, C_extra=C_extra, F_extra=F_extra, current=cur)
    assert same_bits(K_hs, st["C_struc"] + st["C_hydro"] + C_extra) and same_bits(F0, st["W_struc"] + st["W_hydro"] + F_extra)
    assert same_bits(F_env, hip_ctx.current_loads([0.6], [15.0], sw.depth)[:, 0, :]) and np.all(F_env[:, 0] > 0)
    assert statics.hydrostatics(hip_ctx)[2] is None
    vp, mp = _programs()
    r = statics.mean_pose(hip_ctx, K_hs, F0, depth=sw.depth, program=mp, params=sw.params, F_env=F_env)
    assert r.ok.all() and np.all(r.pose[:, 0] > 0) and r.describe_flags(0) == []
    lines = hip_ctx.mooring_expand(sw.params)
    ref = mr.evaluate(lines, r.pose, sw.depth)                       # the envelope of the residual's addends at the returned poses
    E_F = np.abs(F0) + np.abs(F_env) + np.einsum("dij,dj->di", np.abs(K_hs), np.abs(r.pose)) + ref["EF"].astype(np.float64)
    # What Newton leaves at the returned pose is the error of evaluating Y there -- F_moor is held to GATE_C eps EF by the
    # mooring gate, the other addends round within eps of their magnitudes -- plus K times the pose's own error, which
    # the pose gate bounds by GATE eps |K^-1| E_F: component by component |Y| <= eps (GATE_C E_F + GATE |K| |K^-1| E_F).
    # (Norm-wise these variants reach 3.8 eps |E_F|, the cases of test_cases_against_the_reference 0.20.)
    K = K_hs + r.C_moor
    spread = np.einsum("dij,dj->di", np.abs(K), np.einsum("dij,dj->di", np.abs(np.linalg.inv(K)), E_F))
    rn = np.abs(r.F_res) / (mpr.EPS * (mr.GATE_C * E_F + mpr.GATE * spread))
    print("residual of the six variants: worst %s of the bound; %s of eps |E_F| norm-wise" % (
        np.array2string(rn.max(axis=1), precision=3),
        np.array2string(np.linalg.norm(r.F_res, axis=1) / (mpr.EPS * np.linalg.norm(E_F, axis=1)), precision=3)))
    assert np.all(rn <= 1.0)
    assert mc.worst_multiples(dict(C=r.C_moor, F=r.F_moor, T=r.T, J=r.J), ref)["F"] <= mr.GATE_C
    assert same_bits(statics.mean_pose(hip_ctx, K_hs, F0, lines=lines, depth=sw.depth, F_env=F_env).pose, r.pose)


def test_null_arguments(hip_ctx):
    """NULL F_env / x_ref are zeros, NULL tol the defaults, max_iter <= 0 is 40; every output but flags may be NULL."""
    b = cs.batch(DECKS_200[:3])
    full = run(hip_ctx, b)
    z = dict(b, F_env=None, x_ref=None)
    unloaded = cs.batch([DECKS_200[0]] * 3)
    assert all(same_bits(run(hip_ctx, z)[k], run(hip_ctx, unloaded)[k]) for k in OUT)
    assert all(same_bits(run(hip_ctx, b, tol=(1e-9, 1e-10), max_iter=40)[k], full[k]) for k in OUT)
    for k in OUT[:-1]:
        part = run(hip_ctx, b, want=(k,))
        assert set(part) == {k, "flags"} and same_bits(part[k], full[k])
    only = run(hip_ctx, b, want=())
    assert set(only) == {"flags"} and not only["flags"].any()


def test_flags_poison_only_their_design(hip_ctx):
    n, mid = 7, 3
    names = [DECKS_200[i % len(DECKS_200)] for i in range(n)]
    b = cs.batch(names)
    good = run(hip_ctx, b)
    assert not good["flags"].any()
    keep = np.arange(n) != mid

    def check(res, flag, steps=None):
        want = np.zeros(n, dtype=np.int32)
        want[mid] = flag
        assert np.array_equal(res["flags"], want), (flag, res["flags"])
        for k in ("pose", "C", "F", "T", "J", "F_res"):
            assert np.all(np.isnan(res[k][mid])), (flag, k)
            assert same_bits(res[k][keep], good[k][keep]), (flag, k)
        assert same_bits(res["iterations"][keep], good["iterations"][keep])
        if steps is not None:
            assert res["iterations"][mid] == steps

    def edited(key, edit):
        e = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in b.items()}
        edit(e[key][mid])
        return e

    check(run(hip_ctx, edited("K_hs", lambda a: a.__setitem__((2, 2), np.nan))), statics.FLAG_SINGULAR, 0)
    check(run(hip_ctx, edited("F0", lambda a: a.__setitem__(0, np.inf))), statics.FLAG_SINGULAR, 0)
    check(run(hip_ctx, edited("x_ref", lambda a: a.__setitem__(4, np.nan))), 1, 0)                    # a bad pose is a bad line
    check(run(hip_ctx, edited("lines", lambda a: a.__setitem__((1, 6), 5000.0))), 4, 0)              # slack at the start
    check(run(hip_ctx, edited("F_env", lambda a: a.__setitem__(0, -6.0e7))), 4)                      # ... and on the way
    # the cap: two steps do not suffice for the loaded designs; the unloaded ones that need more are flagged too
    res = run(hip_ctx, b, max_iter=2)
    capped = good["iterations"] > 2
    assert capped.any() and np.array_equal(res["flags"], np.where(capped, statics.FLAG_POSE_CAP, 0))
    assert np.all(res["iterations"][capped] == 2) and np.all(np.isnan(res["pose"][capped]))
    assert same_bits(res["pose"][~capped], good["pose"][~capped])


def test_safeguards_on_the_device(hip_ctx):
    """A 5e6 N surge load: the first steps are capped at 30 m (the count says so) and the root is still reached; a zero
    yaw diagonal (one line through the axis, no hydrostatic yaw stiffness) takes the mean diagonal."""
    c = cs.cases()["VolturnUS-S/unloaded"]
    F_env = np.array([5.0e6, 0, 0, 0, 0, 0])
    res = hip_ctx.mean_pose(c["K_hs"][None], c["F0"][None], c["depth"], lines=c["lines"][None], F_env=F_env[None])
    m = mdm.solve(c["lines"], c["depth"], c["K_hs"], c["F0"], F_env)
    assert res["flags"][0] == m["flags"]
    if m["flags"] == 0:
        assert abs(res["iterations"][0] - m["iterations"]) <= 1 and np.allclose(res["pose"][0], m["pose"], rtol=0, atol=1e-8)
    one = hip_ctx.mean_pose(c["K_hs"][None], c["F0"][None], c["depth"], lines=c["lines"][None], F_env=F_env[None], max_iter=1,
                            tol=(1e3, 1e3))
    assert one["flags"][0] == 0 and one["iterations"][0] == 1
    assert np.all(np.abs(one["pose"][0]) <= np.array(mdm.CAPS) * (1 + 4 * mpr.EPS)) and np.isclose(np.abs(one["pose"][0] / mdm.CAPS).max(), 1.0)
    lines = mc.record([-837.0, 0, -200.0], [0.0, 0, -14.0], 870.0, 3.27e9, 6000.0)[None]      # the fairlead on the yaw axis
    K = np.diag(np.diag(cs.synthetic_K()))
    K[5, 5] = 0.0
    F0 = np.array([3.0e5, 0, 8.0e5, 0, 0, 0])
    log = []
    mod = mdm.solve(lines, 200.0, K, F0, log=log)
    assert mod["flags"] == 0 and ("zero_diagonal", 5) in log                            # (without the repair: a zero column)
    dev = hip_ctx.mean_pose(K[None], F0[None], 200.0, lines=lines[None])
    assert dev["flags"][0] == 0 and abs(dev["iterations"][0] - mod["iterations"]) <= 1
    assert np.allclose(dev["pose"][0], mod["pose"], rtol=0, atol=1e-8) and abs(dev["pose"][0][5]) <= 1e-12


def test_errors_before_any_launch(hip_ctx):
    b = cs.batch(DECKS_200[:2])
    fr = dict(b, lines=b["lines"].copy())
    fr["lines"][1, 2, 9] = 0.3
    with pytest.raises(RaftxError, match="CB = 0.3"):
        run(hip_ctx, fr)
    for depth in (-1.0, 0.0, np.nan, np.inf):
        with pytest.raises(RaftxError, match="depth"):
            run(hip_ctx, dict(b, depth=depth))
    for tol in ((-1e-9, 1e-10), (1e-9, np.nan), (np.inf, 1e-10)):
        with pytest.raises(RaftxError, match="tolerances"):
            run(hip_ctx, b, tol=tol)
    with pytest.raises(RaftxError, match="nLine must be positive"):
        hip_ctx.mean_pose(b["K_hs"], b["F0"], 200.0, lines=np.zeros((2, 0, 16)))
    with pytest.raises(RaftxError, match="no program"):
        hip_ctx.mean_pose(b["K_hs"], b["F0"], 200.0, params=np.zeros((2, 5)))
    L = hip_ctx.rlib.lib
    ptr = lambda a: a.ctypes.data
    flags = np.zeros(2, dtype=np.int32)
    args = lambda K, F, fl, n=2: (hip_ctx._h, n, 3, ptr(b["lines"]), None, 200.0, K, F, None, None, None, 0,
                                  None, None, None, None, None, None, None, fl)
    assert L.raftx_mean_pose(*args(None, ptr(b["F0"]), ptr(flags))) != 0
    assert b"required" in L.raftx_last_error(hip_ctx._h)
    assert L.raftx_mean_pose(*args(ptr(b["K_hs"]), None, ptr(flags))) != 0
    assert L.raftx_mean_pose(*args(ptr(b["K_hs"]), ptr(b["F0"]), None)) != 0
    assert L.raftx_mean_pose(*args(ptr(b["K_hs"]), ptr(b["F0"]), ptr(flags), n=-1)) != 0
    assert L.raftx_mean_pose(*args(ptr(b["K_hs"]), ptr(b["F0"]), ptr(flags), n=0)) == 0
    assert L.raftx_mean_pose(*args(ptr(b["K_hs"]), ptr(b["F0"]), ptr(flags))) == 0 and not flags.any()
    # lines == NULL: the program, its line count and params
    nul = (hip_ctx._h, 2, 3, None, None, 200.0, ptr(b["K_hs"]), ptr(b["F0"]), None, None, None, 0, None, None, None, None, None, None,
           None, ptr(flags))
    assert L.raftx_mean_pose(*nul) != 0 and b"without a mooring program" in L.raftx_last_error(hip_ctx._h)
    vp, mp = _programs()
    hip_ctx.variant_program(vp)
    hip_ctx.mooring_program(mp)
    assert L.raftx_mean_pose(*nul) != 0 and b"params" in L.raftx_last_error(hip_ctx._h)
    with pytest.raises(ValueError):
        hip_ctx.mean_pose(b["K_hs"], b["F0"], 200.0, params=np.zeros((2, 4)))
    with pytest.raises(ValueError):
        statics.mean_pose(hip_ctx, b["K_hs"], b["F0"], lines=b["lines"], depth=200.0, params=np.zeros((2, 5)))
