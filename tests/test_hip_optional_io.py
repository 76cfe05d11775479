"""The optional arrays of the stand-alone entry points (-m gpu), through the raw C-ABI with every output pre-filled.

Each call is made with every optional array present, then with each one absent (NULL) in turn:
* an absent optional OUTPUT leaves its array as pre-filled and every other output with the bits of the full call;
* an absent optional INPUT gives the values of the same call with that input present and all zero (the neutral value of
  each of them: an added matrix, an added force, a heading offset, a reference point at the origin) -- x + 0 * y is x in
  IEEE arithmetic, fused or not, except that -0 + 0 is +0: every element compares equal, whatever the kernel does
  with a pointer it has;
* a call whose outer count is zero returns 0 and writes nothing.
The decks are the smallest the parity tests build (2 designs x 2 sea states x 1-2 headings) with nw = 64 and 65 bins:
the two sides of the boundary between 64 and 128 threads per row of the statistics and BEM kernels."""
import numpy as np
import pytest

from raft_amd import snapshot as standin
from raft_amd._abi import _ptr
from tests.util import random_strips, random_matrices, synthetic_cases

pytestmark = pytest.mark.gpu
CASES = [(64, 1), (65, 2)]                       # (nw, nHead)
ND, NC = 2, 2
SENT = {np.dtype(np.float64): 7.25, np.dtype(np.complex128): 7.25 - 3.5j, np.dtype(np.int32): -77}


def filled(shape, dtype=np.float64):
    return np.full(shape, SENT[np.dtype(dtype)], dtype=dtype)


def untouched(a):
    return bool(np.all(a == SENT[a.dtype]))


def written(a):
    return bool(np.all(np.isfinite(a.view(np.float64) if a.dtype.kind in "fc" else a)) and not np.any(a == SENT[a.dtype]))


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def equal(a, b):                                 # element by element (a NaN equals nothing; -0 equals +0)
    return a.shape == b.shape and bool(np.all(a == b))


def call(ctx, name, *args):
    rc = getattr(ctx.rlib.lib, "raftx_" + name)(ctx._h, *[_ptr(a) if isinstance(a, np.ndarray) else a for a in args])
    assert rc == 0, (name, rc, ctx.rlib.lib.raftx_last_error(ctx._h))


class Pick:
    """An optional array of one call: absent -> None, zero -> zeros, else the array itself."""

    def __init__(self, absent=(), zero=()):
        self.absent, self.zero = set(absent), set(zero)

    def __call__(self, name, a):
        return None if name in self.absent else (np.zeros_like(a) if name in self.zero else a)


def each_absent(run, outs=(), ins=()):
    """run(pick) -> {name: output array (pre-filled where the call was not given it)}"""
    ref = run(Pick())
    for k, v in ref.items():
        assert written(v), k
    for o in outs:
        got = run(Pick(absent=[o]))
        assert untouched(got[o]), o
        for k in ref:
            assert k == o or same(got[k], ref[k]), (o, k)
    for i in ins:
        got, zero = run(Pick(absent=[i])), run(Pick(zero=[i]))
        for k in ref:
            assert equal(got[k], zero[k]), (i, k)
        assert not all(equal(got[k], ref[k]) for k in ref), i             # (the input matters: the full call differs)
    return ref


def cnormal(rng, shape, scale=1.0):
    return scale * (rng.normal(size=shape) + 1j * rng.normal(size=shape))


def deck(ctx, nw, nH):
    rng = np.random.default_rng(4100 + nw)
    tables = [random_strips(rng, S, nw) for S in (5, 9)]
    M0, B0, C0, MBw = random_matrices(rng, ND, nw)
    w, k, zeta, beta = synthetic_cases(rng, NC, nH, nw)
    ctx.upload_designs(tables, M0, B0, C0, nw, MBw)
    ctx.upload_cases(w, k, 200.0, 1025.0, 9.81, zeta, beta)
    return rng, w


@pytest.mark.parametrize("nw,nH", CASES)
def test_statistics_of_the_resident_responses(hip_ctx, nw, nH):
    rng, w = deck(hip_ctx, nw, nH)
    hip_ctx.solve_dynamics_device(3, 0.01, 0.1)
    dw, nCh = float(w[1] - w[0]), 3

    def motion(pick):
        sd, psd = filled((ND, NC, 6)), filled((ND, NC, 6, nw))
        call(hip_ctx, "motion_stats", dw, sd, pick("psd", psd))
        return dict(sd=sd, psd=psd)
    each_absent(motion, outs=["psd"])

    L, pw = rng.normal(size=(ND, nCh, 6)), np.array([0, 2, 1], dtype=np.int32)

    def channel(pick, n=nCh):
        sd, psd = filled((ND, NC, nCh)), filled((ND, NC, nCh, nw))
        call(hip_ctx, "channel_stats", n, L, pw, dw, sd, pick("psd", psd))
        return dict(sd=sd, psd=psd)
    each_absent(channel, outs=["psd"])
    assert all(untouched(v) for v in channel(Pick(), n=0).values())

    Lp, Gw = rng.normal(size=(ND, nCh, 3, 6)), cnormal(rng, (ND, nCh, 6, nw))

    def poly(pick, n=nCh):
        sd, psd = filled((ND, NC, nCh)), filled((ND, NC, nCh, nw))
        call(hip_ctx, "channel_stats_poly", n, Lp, pick("Gw", Gw), dw, sd, pick("psd", psd))
        return dict(sd=sd, psd=psd)
    each_absent(poly, outs=["psd"], ins=["Gw"])
    assert all(untouched(v) for v in poly(Pick(), n=0).values())


@pytest.mark.parametrize("nw", [64, 65])
def test_statistics_of_a_caller_held_response(hip_ctx, nw):
    rng = np.random.default_rng(4200 + nw)
    nCh, nDof, nResp = 3, 8, 2
    w = np.linspace(0.05, 2.0, nw)
    L, Gw, Xi = rng.normal(size=(nCh, 3, nDof)), cnormal(rng, (nCh, nDof, nw)), cnormal(rng, (nResp, nDof, nw))

    def run(pick, n=nCh):
        sd, psd = filled((nCh,)), filled((nCh, nw))
        call(hip_ctx, "response_stats", n, nDof, nResp, nw, w, L, pick("Gw", Gw), Xi, float(w[1] - w[0]), sd, pick("psd", psd))
        return dict(sd=sd, psd=psd)
    each_absent(run, outs=["psd"], ins=["Gw"])
    assert all(untouched(v) for v in run(Pick(), n=0).values())


@pytest.mark.parametrize("nw,nH", CASES)
def test_first_order_strip_calls(hip_ctx, nw, nH):
    rng, w = deck(hip_ctx, nw, nH)
    Xi = cnormal(rng, (ND, NC, 6, nw), 0.3)
    Xi[:, :, 3:] *= 0.02

    def linearize(pick):
        B, F = filled((ND, NC, 6, 6)), filled((ND, NC, nH, 6, nw), np.complex128)
        call(hip_ctx, "linearize", Xi, pick("B_drag", B), pick("F_drag", F))
        return dict(B_drag=B, F_drag=F)
    each_absent(linearize, outs=["B_drag", "F_drag"])

    S = 9                                            # the strips of design 1

    def kinematics(pick):
        u, ud, p = (filled((nH, S, 3, nw), np.complex128), filled((nH, S, 3, nw), np.complex128), filled((nH, S, nw), np.complex128))
        call(hip_ctx, "strip_kinematics", 1, 1, pick("u", u), pick("ud", ud), pick("pDyn", p))
        return dict(u=u, ud=ud, pDyn=p)
    each_absent(kinematics, outs=["u", "ud", "pDyn"])

    def drag(pick):
        B, F = filled((S, 3, 3)), filled((S, 3, nw), np.complex128)
        call(hip_ctx, "strip_drag", 1, 1, np.ascontiguousarray(Xi[1, 1]), nH - 1, pick("Bmat", B), pick("F_exc_drag", F))
        return dict(Bmat=B, F_exc_drag=F)
    each_absent(drag, outs=["Bmat", "F_exc_drag"])


@pytest.mark.parametrize("nw,nH", CASES)
def test_bem_excitation(hip_ctx, nw, nH):
    rng, w = deck(hip_ctx, nw, nH)
    heads = np.array([0.0, 90.0, 200.0])
    X = cnormal(rng, (ND, len(heads), 6, nw), 1e5)
    adjust, xy, Fadd = rng.uniform(-20, 20, size=ND), rng.uniform(-50, 50, size=(ND, 2)), cnormal(rng, (ND, NC, nH, 6, nw), 1e4)

    def run(pick):
        F = filled((ND, NC, nH, 6, nw), np.complex128)
        call(hip_ctx, "bem_excitation", len(heads), heads, X, pick("heading_adjust", adjust), pick("xy_ref", xy), pick("F_add", Fadd),
             pick("F_out", F))
        return dict(F_out=F)
    each_absent(run, outs=["F_out"], ins=["heading_adjust", "xy_ref", "F_add"])


@pytest.mark.parametrize("nUnit", [1, 2])            # the LDS-resident kernel | the register-resident one
@pytest.mark.parametrize("nw", [64, 65])
def test_solve_system(hip_ctx, nw, nUnit):
    rng = np.random.default_rng(4300 + nw + nUnit)
    nSys, nRhs, n = 2, 2, 6 * nUnit
    w = np.linspace(0.05, 2.0, nw)
    Z = cnormal(rng, (nSys, nUnit, 6, 6, nw)) + (10.0 * np.eye(6))[None, None, :, :, None]
    F = cnormal(rng, (nSys, nRhs, n, nw))
    Mc, Bc, Cc = (s * rng.normal(size=(nSys, n, n)) for s in (0.5, 0.3, 0.7))

    def run(pick, ns=nSys):
        Xi = filled((nSys, nRhs, n, nw), np.complex128)
        call(hip_ctx, "solve_system", ns, nUnit, nRhs, nw, w, Z, pick("Mc", Mc), pick("Bc", Bc), pick("Cc", Cc), F, Xi)
        return dict(Xi=Xi)
    each_absent(run, ins=["Mc", "Bc", "Cc"])
    assert untouched(run(Pick(), ns=0)["Xi"])


@pytest.mark.parametrize("nw", [64, 65])
def test_dense_solvers(hip_ctx, nw):
    rng = np.random.default_rng(4400 + nw)
    nSys, nRhs, n = 2, 2, 8
    w = np.linspace(0.05, 2.0, nw)
    M = rng.normal(size=(nSys, n, n)) + 20.0 * np.eye(n)
    B = rng.normal(size=(nSys, n, n)) + 5.0 * np.eye(n)
    Cm = rng.normal(size=(nSys, n, n)) + 40.0 * np.eye(n)
    F = cnormal(rng, (nSys, nRhs, n, nw))

    def one(pick):
        Xi, Z = filled((nRhs, n, nw), np.complex128), filled((n, n, nw), np.complex128)
        call(hip_ctx, "solve_dense", n, nRhs, nw, w, M[0], B[0], Cm[0], 0, F[0], Xi, pick("Z", Z))
        return dict(Xi=Xi, Z=Z)
    each_absent(one, outs=["Z"])

    def batch(pick, ns=nSys):
        Xi, Z = filled((nSys, nRhs, n, nw), np.complex128), filled((nSys, n, n, nw), np.complex128)
        call(hip_ctx, "solve_dense_batch", ns, n, nRhs, nw, w, M, B, Cm, 0, F, Xi, pick("Z", Z))
        return dict(Xi=Xi, Z=Z)
    ref = each_absent(batch, outs=["Z"])
    assert all(untouched(v) for v in batch(Pick(), ns=0).values())

    hip_ctx.dense_resident(w, M, B, Cm)
    Badd = 0.4 * rng.normal(size=(nSys, n, n))

    def resident(pick):
        Xi, Z = filled((nSys, nRhs, n, nw), np.complex128), filled((nSys, n, n, nw), np.complex128)
        call(hip_ctx, "solve_dense_resident", 1, pick("Badd", Badd), nRhs, F, Xi, pick("Z", Z))
        return dict(Xi=Xi, Z=Z)
    each_absent(resident, outs=["Z"], ins=["Badd"])
    got = resident(Pick(absent=["Badd"]))
    assert equal(got["Xi"], ref["Xi"]) and equal(got["Z"], ref["Z"])
    hip_ctx.dense_resident(None, None, None, None)


def test_kim_yue_table_fetched_or_left_resident(hip_ctx):
    """kay_out of raftx_qtf_kay: the table the call leaves resident for the next raftx_qtf_slender is the one it hands out."""
    from raft_amd import qtf as rq, waves
    f = standin.build_model(standin.load_fixture("c5_oc4semi_qtf.npz")["model"]).fowtList[0]
    tab = rq.pack_qtf(f)
    nw2 = 12
    w2 = np.arange(1, nw2 + 1) * 0.04 * 2 * np.pi
    k2 = np.array([waves.wave_number(x, f.depth) for x in w2])
    beta = np.array([np.deg2rad(30.0)])
    args = ([tab], beta, w2, k2, f.depth, f.rho_water, f.g)
    table = hip_ctx.qtf_kay(*args, fetch=True)
    assert np.all(np.isfinite(table.view(float))) and np.any(table != 0)
    assert same(hip_ctx.qtf_kay(*args, fetch=True), table)
    Xi = cnormal(np.random.default_rng(4500), (1, 6, nw2), 0.2)
    Ms = f.M_struc[None]
    fed = hip_ctx.qtf_slender([tab], Xi, beta, w2, k2, f.depth, f.rho_water, f.g, Ms, table)
    assert hip_ctx.qtf_kay(*args, fetch=False) is None
    assert same(hip_ctx.qtf_slender([tab], Xi, beta, w2, k2, f.depth, f.rho_water, f.g, Ms, None), fed)
    assert not same(hip_ctx.qtf_slender([tab], Xi, beta, w2, k2, f.depth, f.rho_water, f.g, Ms, None), fed)      # one-shot: gone


def test_second_order_calls_without_sets(hip_ctx):
    nw2, nw = 4, 5
    w2, k2, w = np.linspace(0.2, 0.8, nw2), np.linspace(0.01, 0.07, nw2), np.linspace(0.1, 1.0, nw)
    off0, one = np.zeros(1, dtype=np.int64), np.ones(36)
    out = filled((1, nw2, nw2, 6), np.complex128)
    call(hip_ctx, "qtf_kay", 0, nw2, w2, k2, 200.0, 1025.0, 9.81, off0, None, one, 4, out)
    assert untouched(out)
    call(hip_ctx, "qtf_slender", 0, nw2, w2, k2, 200.0, 1025.0, 9.81, off0, None, off0, None, out, one, one, None, out)
    assert untouched(out)
    fm, f2 = filled((1, 6)), filled((1, 6, nw))
    call(hip_ctx, "qtf_force", 0, nw2, w2, out, nw, w, 0.1, one, fm, f2)
    assert untouched(fm) and untouched(f2) and untouched(out)


def test_modal_calls(hip_ctx):
    from tests.test_hip_modal import _variant_sweep
    n = 2
    sw = _variant_sweep(n)
    sw.upload(hip_ctx)
    rng = np.random.default_rng(4600)
    dM, dC = 1e5 * np.abs(rng.normal(size=(n, 6, 6))) * np.eye(6), 1e4 * np.abs(rng.normal(size=(n, 6, 6))) * np.eye(6)

    def resident(pick):
        fn, modes, flags, props = filled((n, 6)), filled((n, 6, 6)), filled((n,), np.int32), filled((n, 12))
        call(hip_ctx, "modal_resident", pick("dM", dM), pick("dC", dC), fn, modes, flags, pick("props", props))
        return dict(fn=fn, modes=modes, flags=flags, props=props)
    each_absent(resident, outs=["props"], ins=["dM", "dC"])

    M, Cm = np.repeat((1e6 * np.eye(6))[None], n, axis=0), np.repeat((1e5 * np.diag([1.0, 2, 3, 4, 5, 6]))[None], n, axis=0)

    def batch(count):
        fn, modes, flags = filled((n, 6)), filled((n, 6, 6)), filled((n,), np.int32)
        call(hip_ctx, "modal_batch", count, M, Cm, fn, modes, flags)
        return fn, modes, flags
    assert all(written(a) for a in batch(n))
    assert all(untouched(a) for a in batch(0))
