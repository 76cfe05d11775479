"""The four statistics entries (raftx_motion_stats, raftx_channel_stats, raftx_channel_stats_poly, raftx_response_stats)
against tests/stats_reference.py: the formulas of include/raftx.h evaluated independently in numpy.longdouble, with the
derived forward-error bound of an fp64 evaluation as the ONLY tolerance (see that module).  Every check is written once as
_check_*(ctx) and runs on the CPU oracle (default selection) and on the HIP library (-m gpu).

The shapes put the frequency axis on both sides of every launch shape of the kernels (64, 128 or 256 lanes striding the
bins: 1..64 | 65..128 | 129..256 | more than one trip), on wave and block boundaries, and pair nHead = 1 with them; the
designs of the resident batch carry rows of L and Gw that differ by orders of magnitude, so that a wrong design index
cannot pass.  Every input set is also evaluated in plain complex128 NumPy, which has to stay inside the same bound: the
bound itself can then never be what is wrong."""
import numpy as np
import pytest

from raft_amd._abi import RaftxError
from tests import stats_reference as R
from tests.util import random_strips, random_matrices, synthetic_cases


def _within(ref, std, psd, nDof, nResp, what, factor=1.0, mask=None):
    f_psd, f_var = R.used(ref, std, psd, nDof, nResp, mask)
    print("%s: uses %.3g of the psd bound, %.3g of the variance bound" % (what, f_psd, f_var))
    assert f_psd <= factor and f_var <= factor, (what, f_psd, f_var)


def _numpy_within(ref, coef, Xi, dw, nDof, nResp, what, want_psd=True):
    """complex128 NumPy of the same formula on the same inputs sits inside the bound."""
    std, psd = R.numpy_c128(coef, Xi, dw)
    _within(ref, std, psd if want_psd else None, nDof, nResp, what + " [complex128 NumPy]")


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ------------------------------------------------------------------ raftx_response_stats: every input is the test's own
RESPONSE_SHAPES = [(1, 1, 1, 1), (2, 6, 1, 2), (63, 6, 2, 1), (64, 7, 1, 3), (65, 7, 3, 5), (128, 6, 1, 2), (129, 150, 1, 4),
                   (255, 6, 2, 2), (256, 6, 1, 1), (257, 150, 2, 3), (513, 12, 1, 2), (700, 240, 3, 2)]      # (nw, nDof, nResp, nChan)


def _axis(nw):
    w = np.linspace(0.0, 2.5, nw) if nw > 1 else np.array([0.7])           # one bin at w = 0
    return w, (w[1] - w[0] if nw > 1 else 0.1)


def _rows(rng, nChan, nDof, nw):
    """L with its displacement / velocity / acceleration blocks near 1, 10 and 100 (a lost power of w cannot hide), Gw"""
    L = rng.normal(size=(nChan, 3, nDof)) * np.array([1.0, 10.0, 100.0])[None, :, None]
    Gw = 5.0 * (rng.normal(size=(nChan, nDof, nw)) + 1j * rng.normal(size=(nChan, nDof, nw)))
    return L, Gw


def _response_case(ctx, w, dw, L, Gw, Xi, what):
    """One input set: with and without psd (std bit-identical), against the reference; returns (ref, std, psd)."""
    nResp, nDof, nw = Xi.shape
    coef = R.poly_coef(w, L, Gw)
    ref = R.stats(coef, Xi, dw)
    std, psd = ctx.response_stats(w, L, Xi, dw, Gw=Gw, want_psd=True)
    std_only, none = ctx.response_stats(w, L, Xi, dw, Gw=Gw)
    assert none is None and _same_bits(std_only, std), what
    return coef, ref, std, psd


def _check_response_stats(ctx, nw, nDof, nResp, nChan):
    rng = np.random.default_rng([nw, nDof, nResp, nChan])
    w, dw = _axis(nw)
    L, Gw = _rows(rng, nChan, nDof, nw)
    # (a) seeded normal Xi, L, Gw
    Xi = rng.normal(size=(nResp, nDof, nw)) + 1j * rng.normal(size=(nResp, nDof, nw))
    for g in (Gw, None):
        what = "normal, %s Gw" % ("with" if g is not None else "no")
        coef, ref, std, psd = _response_case(ctx, w, dw, L, g, Xi, what)
        _numpy_within(ref, coef, Xi, dw, nDof, nResp, what)
        _within(ref, std, psd, nDof, nResp, what)
    # (b) one-hot Xi in the last bin and in the first: zero -- exactly -- in every other bin (strides, tail bins, waves
    # that hold no bin)
    h0, j0 = nResp - 1, nDof // 2
    for i0 in (nw - 1, 0):
        X1 = np.zeros((nResp, nDof, nw), dtype=complex)
        X1[h0, j0, i0] = 0.75 - 1.25j
        for g in (Gw, None):
            what = "one-hot at bin %d, %s Gw" % (i0, "with" if g is not None else "no")
            coef, ref, std, psd = _response_case(ctx, w, dw, L, g, X1, what)
            _numpy_within(ref, coef, X1, dw, nDof, nResp, what)
            other = np.arange(nw) != i0
            assert np.all(psd[:, other] == 0.0), what
            assert np.all(ref.psd[:, i0] > 0) and np.all(psd[:, i0] > 0), what
            _within(ref, std, psd, nDof, nResp, what)
    # (c) a cancelling channel: Xi[h,j,w] = a_j g[h,w] (1 + 1e-9 r[h,j,w]) and L[0,0,:] orthogonal to a, so that
    # sum_j L_j Xi_j is ~1e-9 of its envelope in every bin -- the bound, not a relative error, is what is asserted
    a = rng.uniform(0.5, 2.0, size=nDof) * rng.choice([-1.0, 1.0], size=nDof)
    gsh = rng.normal(size=(nResp, 1, nw)) + 1j * rng.normal(size=(nResp, 1, nw))
    Xc = a[None, :, None] * gsh * (1.0 + 1e-9 * rng.uniform(-1.0, 1.0, size=(nResp, nDof, nw)))
    Lc = np.zeros((nChan, 3, nDof))
    Lc[:, 0] = rng.normal(size=(nChan, nDof))
    if nDof > 1:
        Lc[0, 0] -= (Lc[0, 0] @ a) / (a @ a) * a
    coef, ref, std, psd = _response_case(ctx, w, dw, Lc, None, Xc, "cancelling")
    if nDof > 1:
        ratio = ref.psd[0] / ref.env_psd[0]
        assert np.all(ratio < 1e-14), float(ratio.max())                     # |y| <~ 1e-8 of the envelope in every bin
    _numpy_within(ref, coef, Xc, dw, nDof, nResp, "cancelling")
    _within(ref, std, psd, nDof, nResp, "cancelling")
    # (d) one NaN in one bin of response 0: std of every channel is NaN, psd is NaN in exactly that bin
    if (nw, nDof, nResp, nChan) == (257, 150, 2, 3):
        Xn = Xi.copy()
        Xn[0, 77, 130] = np.nan
        for g in (Gw, None):
            coef, ref, std, psd = _response_case(ctx, w, dw, L, g, Xn, "NaN")
            other = np.arange(nw) != 130
            assert np.all(np.isnan(std)) and np.all(np.isnan(psd[:, 130])) and np.all(np.isfinite(psd[:, other]))
            f_psd, _ = R.used(ref, std, psd, nDof, nResp, mask=other)
            f_np, _ = R.used(ref, *R.numpy_c128(coef, Xn, dw), nDof, nResp, mask=other)
            assert f_psd <= 1.0 and f_np <= 1.0, (f_psd, f_np)


@pytest.mark.parametrize("nw,nDof,nResp,nChan", RESPONSE_SHAPES)
def test_oracle_response_stats_against_extended_reference(oracle_ctx, nw, nDof, nResp, nChan):
    _check_response_stats(oracle_ctx, nw, nDof, nResp, nChan)


# ------------------------------------------------------------------ the kernels of the resident responses
RESIDENT_SHAPES = [(8, 3), (64, 1), (65, 1), (65, 3), (128, 3), (129, 1), (257, 1), (257, 3), (700, 3)]      # (nw, nHead)
N_DESIGN, N_CASE, STRIPS = 3, 2, (9, 5, 12)
# The bound models fp64 ROUNDING, not underflow: synthetic_cases' default axis starts at 0.05 rad/s, where its JONSWAP
# amplitudes are ~1e-150 and |Xi|^2 is subnormal or zero in fp64 (plain complex128 NumPy then misses the bound as well).
# From 0.3 rad/s on every |Xi| of these sea states stays far above sqrt(DBL_MIN); _resident asserts it.
W_MIN, XI_FLOOR = 0.3, 1e-100


def _resident(ctx, nw, nHead, strips=STRIPS, singular=None, keep=None):
    """A real solve whose responses stay resident; the reference is evaluated on the FETCHED Xi, so it owes nothing to
    the solver.  singular: index of a design replaced by the all-zero, no-strip design under a unit force (flag 2,
    non-finite Xi); keep: the designs of the batch to upload (default all).  Returns (w, dw, Xi, flags)."""
    rng = np.random.default_rng([nw, nHead])
    tables = [random_strips(rng, S) for S in strips]
    M0, B0, C0, _ = random_matrices(rng, len(strips))
    w, k, zeta, beta = synthetic_cases(rng, N_CASE, nHead, nw, wmin=W_MIN)
    Fe = None
    if singular is not None:
        tables[singular] = random_strips(rng, 0)
        M0[singular] = B0[singular] = C0[singular] = 0.0
        Fe = np.ones((len(strips), N_CASE, nHead, 6, nw), dtype=complex)
    if keep is not None:
        tables, M0, B0, C0 = [tables[d] for d in keep], M0[keep], B0[keep], C0[keep]
        Fe = None if Fe is None else np.ascontiguousarray(Fe[keep])
    ctx.upload_designs(tables, M0, B0, C0, nw)
    ctx.upload_cases(w, k, 200.0, 1025.0, 9.81, zeta, beta)
    ctx.solve_dynamics_device(2, 0.01, 0.1, F_extra=Fe)
    out = ctx.fetch_results(want_Xi=True)
    mag = np.abs(out["Xi"][np.isfinite(out["Xi"])])
    assert mag.size and mag.min() > XI_FLOOR, "a response so small that its square leaves fp64's normal range"
    return w, w[1] - w[0], out["Xi"], out["flags"]


def _psd_sums_to_variance(ref, std, psd, dw, nHead, what):
    """std^2 against sum_w psd dw: both sit within their bound of the reference, so within twice the variance bound."""
    _, Kv = R.bound_factors(6, nHead, psd.shape[-1])
    var = np.asarray(std, dtype=R.LD) ** 2
    err = np.abs(var - (np.asarray(psd, dtype=R.LD) * R.LD(dw)).sum(axis=-1))
    assert np.all(err <= 2 * Kv * ref.env_var), (what, float(np.max(err / (Kv * ref.env_var))))


def _check_motion_stats(ctx, nw, nHead):
    w, dw, Xi, _ = _resident(ctx, nw, nHead)
    coef = R.motion_coef(nw)
    ref = R.stats(coef, Xi, dw)
    std, psd = ctx.motion_stats(dw, want_psd=True)
    std_only, none = ctx.motion_stats(dw)
    assert none is None and _same_bits(std_only, std)
    _numpy_within(ref, coef, Xi, dw, 6, nHead, "motions")
    _within(ref, std, psd, 6, nHead, "motions")
    _psd_sums_to_variance(ref, std, psd, dw, nHead, "motions")


def _channel_rows(rng):
    """Five channels, one per power; design 1's rows are 1000 times design 0's: a wrong design index shows at once."""
    L = rng.normal(size=(N_DESIGN, 5, 6)) * np.array([1, 1, 1, 50, 50, 50])
    L[1] = 1000.0 * L[0]
    return L, [0, 1, 2, 3, 4]


def _check_channel_stats(ctx, nw, nHead):
    w, dw, Xi, _ = _resident(ctx, nw, nHead)
    L, pw = _channel_rows(np.random.default_rng([11, nw, nHead]))
    coef = R.power_coef(w, L, pw)[:, None]                                    # [d,1,c,j,w] against Xi [d,case,h,j,w]
    ref = R.stats(coef, Xi, dw)
    std, psd = ctx.channel_stats(L, pw, dw, want_psd=True)
    std_only, none = ctx.channel_stats(L, pw, dw)
    assert none is None and _same_bits(std_only, std)
    _numpy_within(ref, coef, Xi, dw, 6, nHead, "channels")
    _within(ref, std, psd, 6, nHead, "channels")
    _psd_sums_to_variance(ref, std, psd, dw, nHead, "channels")


def _poly_rows(rng, nw):
    """Four channels with all three powers populated; L and Gw differ per design by orders of magnitude."""
    L = rng.normal(size=(N_DESIGN, 4, 3, 6)) * np.array([1, 1, 1, 50, 50, 50]) * np.array([1.0, 10.0, 100.0])[:, None]
    Gw = 5.0 * (rng.normal(size=(N_DESIGN, 4, 6, nw)) + 1j * rng.normal(size=(N_DESIGN, 4, 6, nw)))
    scale = np.array([1.0, 1000.0, 1e-3])
    return L * scale[:, None, None, None], Gw * scale[:, None, None, None]


def _check_channel_stats_poly(ctx, nw, nHead):
    w, dw, Xi, _ = _resident(ctx, nw, nHead)
    L, Gw = _poly_rows(np.random.default_rng([12, nw, nHead]), nw)
    for g in (Gw, None):
        what = "poly channels, %s Gw" % ("with" if g is not None else "no")
        coef = R.poly_coef(w, L, g)[:, None]
        ref = R.stats(coef, Xi, dw)
        std, psd = ctx.channel_stats_poly(L, dw, Gw=g, want_psd=True)
        std_only, none = ctx.channel_stats_poly(L, dw, Gw=g)
        assert none is None and _same_bits(std_only, std), what
        _numpy_within(ref, coef, Xi, dw, 6, nHead, what)
        _within(ref, std, psd, 6, nHead, what)
        _psd_sums_to_variance(ref, std, psd, dw, nHead, what)
        # raftx_response_stats fed pair (d, c)'s fetched Xi, row L[d] and Gw[d] gives that pair's result: both within
        # the bound of one reference, so within twice the bound of each other
        for d in range(N_DESIGN):
            for c in range(N_CASE):
                pair = R.Stats(ref.std[d, c], ref.psd[d, c], ref.env_psd[d, c], ref.env_var[d, c])
                s1, p1 = ctx.response_stats(w, L[d], Xi[d, c], dw, Gw=None if g is None else g[d], want_psd=True)
                _within(pair, s1, p1, 6, nHead, "%s: response_stats of pair (%d, %d)" % (what, d, c))
                Kp, Kv = R.bound_factors(6, nHead, nw)
                assert np.all(np.abs(p1.astype(R.LD) - psd[d, c].astype(R.LD)) <= 2 * Kp * pair.env_psd)
                assert np.all(np.abs(s1.astype(R.LD) ** 2 - std[d, c].astype(R.LD) ** 2) <= 2 * Kv * pair.env_var)


@pytest.mark.parametrize("nw,nHead", RESIDENT_SHAPES)
def test_oracle_motion_stats_against_extended_reference(oracle_ctx, nw, nHead):
    _check_motion_stats(oracle_ctx, nw, nHead)


@pytest.mark.parametrize("nw,nHead", RESIDENT_SHAPES)
def test_oracle_channel_stats_against_extended_reference(oracle_ctx, nw, nHead):
    _check_channel_stats(oracle_ctx, nw, nHead)


@pytest.mark.parametrize("nw,nHead", RESIDENT_SHAPES)
def test_oracle_channel_stats_poly_against_extended_reference(oracle_ctx, nw, nHead):
    _check_channel_stats_poly(oracle_ctx, nw, nHead)


def _all_resident_stats(ctx, w, dw, nw):
    """(coef, nDof-6 stats call) of the three resident entries with the rows of the tests above"""
    L5, pw = _channel_rows(np.random.default_rng(21))
    L4, Gw = _poly_rows(np.random.default_rng(22), nw)
    return [("motions", lambda keep: R.motion_coef(nw), lambda keep: ctx.motion_stats(dw, want_psd=True)),
            ("channels", lambda keep: R.power_coef(w, L5[keep], pw)[:, None],
             lambda keep: ctx.channel_stats(L5[keep], pw, dw, want_psd=True)),
            ("poly channels", lambda keep: R.poly_coef(w, L4[keep], Gw[keep])[:, None],
             lambda keep: ctx.channel_stats_poly(L4[keep], dw, Gw=Gw[keep], want_psd=True))]


def _check_singular_pair_in_the_batch(ctx):
    """The middle design is the all-zero, no-strip design of test_singular_system_is_flagged_not_hidden (flag 2,
    non-finite Xi): its statistics are non-finite, and its neighbours' are untouched -- within the bound of their own
    reference and bit-identical to a batch without it."""
    nw, nHead, good = 65, 3, [0, 2]
    w, dw, Xi, flags = _resident(ctx, nw, nHead, singular=1)
    assert np.all(flags[1] & 2) and not np.any(flags[good] & 2)
    assert not np.any(np.isfinite(Xi[1])) and np.all(np.isfinite(Xi[good]))
    every = list(range(N_DESIGN))
    with_it = [(name, coef(good), run(every)) for name, coef, run in _all_resident_stats(ctx, w, dw, nw)]
    w2, dw2, Xi2, flags2 = _resident(ctx, nw, nHead, singular=1, keep=good)
    assert _same_bits(Xi2, Xi[good]) and np.array_equal(flags2, flags[good])
    without = [run(good) for _, _, run in _all_resident_stats(ctx, w2, dw2, nw)]
    for (name, coef, (std, psd)), (std2, psd2) in zip(with_it, without):
        assert not np.any(np.isfinite(std[1])) and not np.any(np.isfinite(psd[1])), name
        ref = R.stats(coef, Xi[good], dw)
        _numpy_within(ref, coef, Xi[good], dw, 6, nHead, name)
        _within(ref, std[good], psd[good], 6, nHead, name + " next to a singular design")
        assert _same_bits(std[good], std2) and _same_bits(psd[good], psd2), name


def test_oracle_singular_pair_leaves_its_neighbours_statistics_alone(oracle_ctx):
    _check_singular_pair_in_the_batch(oracle_ctx)


def _check_crossing_statistics(ctx):
    """raftx_sweep_stats (the statistics kernel in its crossing form, which also carries niter / flags) on five C3
    variants: its std against the reference on its own returned Xi.  (std only, as the crossing returns: the first bins
    of this sea state carry amplitudes whose squares leave fp64's normal range, which the variance does not notice.)"""
    from tests.test_geometry import C3, _c3_crossing_inputs
    D, M0, B0, C0 = _c3_crossing_inputs(5)
    zeta2 = np.stack([np.asarray(C3["zeta"]), 0.5 * np.asarray(C3["zeta"])])
    beta2 = np.stack([np.asarray(C3["beta"]), np.asarray(C3["beta"]) + 0.4])
    w = np.asarray(C3["w"])
    got = ctx.sweep_stats(D, M0, B0, C0, w, C3["k"], float(C3["depth"]), zeta2, beta2, int(C3["nIter"]), 0.01,
                          float(C3["XiStart"]), want_Xi=True)
    assert got["Xi"].shape[:2] == (5, 2) and np.all(got["niter"] > 0) and not np.any(got["flags"] & 2)
    dw = w[1] - w[0]
    coef = R.motion_coef(len(w))
    ref = R.stats(coef, got["Xi"], dw)
    nHead = got["Xi"].shape[2]
    _numpy_within(ref, coef, got["Xi"], dw, 6, nHead, "crossing", want_psd=False)
    _within(ref, got["std"], None, 6, nHead, "crossing")


def test_oracle_crossing_statistics_against_extended_reference(oracle_ctx):
    _check_crossing_statistics(oracle_ctx)


def _check_dw_must_be_positive(ctx):
    """All four entries refuse a dw that is not > 0 (zero, negative, NaN) instead of returning infinite spectra."""
    w, dw, Xi, _ = _resident(ctx, 8, 1)
    L5, pw = _channel_rows(np.random.default_rng(31))
    L4, Gw = _poly_rows(np.random.default_rng(32), 8)
    calls = [lambda x: ctx.motion_stats(x, want_psd=True), lambda x: ctx.channel_stats(L5, pw, x, want_psd=True),
             lambda x: ctx.channel_stats_poly(L4, x, Gw=Gw, want_psd=True),
             lambda x: ctx.response_stats(w, L4[0], Xi[0, 0], x, Gw=Gw[0], want_psd=True)]
    for call in calls:
        call(dw)                                                             # the call itself is a good one
        for bad in (0.0, -1.0, float("nan")):
            with pytest.raises(RaftxError, match="dw must be positive"):
                call(bad)


def test_oracle_statistics_refuse_a_dw_that_is_not_positive(oracle_ctx):
    _check_dw_must_be_positive(oracle_ctx)


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("nw,nDof,nResp,nChan", RESPONSE_SHAPES)
def test_hip_response_stats_against_extended_reference(hip_ctx, nw, nDof, nResp, nChan):
    _check_response_stats(hip_ctx, nw, nDof, nResp, nChan)


@pytest.mark.gpu
@pytest.mark.parametrize("nw,nHead", RESIDENT_SHAPES)
def test_hip_motion_stats_against_extended_reference(hip_ctx, nw, nHead):
    _check_motion_stats(hip_ctx, nw, nHead)


@pytest.mark.gpu
@pytest.mark.parametrize("nw,nHead", RESIDENT_SHAPES)
def test_hip_channel_stats_against_extended_reference(hip_ctx, nw, nHead):
    _check_channel_stats(hip_ctx, nw, nHead)


@pytest.mark.gpu
@pytest.mark.parametrize("nw,nHead", RESIDENT_SHAPES)
def test_hip_channel_stats_poly_against_extended_reference(hip_ctx, nw, nHead):
    _check_channel_stats_poly(hip_ctx, nw, nHead)


@pytest.mark.gpu
def test_hip_singular_pair_leaves_its_neighbours_statistics_alone(hip_ctx):
    _check_singular_pair_in_the_batch(hip_ctx)


@pytest.mark.gpu
def test_hip_crossing_statistics_against_extended_reference(hip_ctx):
    _check_crossing_statistics(hip_ctx)


@pytest.mark.gpu
def test_hip_statistics_refuse_a_dw_that_is_not_positive(hip_ctx):
    _check_dw_must_be_positive(hip_ctx)
