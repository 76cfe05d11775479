"""The second-order entries (raftx_qtf_slender, raftx_qtf_slender_rows, raftx_qtf_kay, raftx_qtf_force) against
tests/qtf_reference.py: the same operations in numpy.clongdouble with the non-cancelling envelope E of what they sum.
EVERY entry and DOF is compared, |x - ref| <= C eps E with eps = 2^-52; where E == 0 the result has to be exactly 0.

The constants.  One entry is too many operations for a clean forward-error derivation, so C is measured -- against the
reference, never against the device: the worst envelope-scaled error of the complex128 HOST implementations
(oracle/qtf_oracle.py, tests/qtf_device_model.py, raft_amd.qtf.kay_correction) over every input set of this file, times
16, rounded up to a power of two.  The 16 covers what the device legitimately does differently: the strip-frame rotation
(two more 3-term dot products per vector), FMA contraction, tabulated exponential products instead of sinh / cosh,
another summation order over strips and orders.  The host implementations are asserted to stay inside C / 4.
    slender body   host worst 54.5 eps E (tests/qtf_device_model.py; the oracle itself 35.9)  ->  C = 1024;
                   k_qtf_pairs on the MI355X: worst 26.1 eps E = 0.026 of C (nw2 = 64, nSet = 3, set 0)
    Kim & Yue      host worst 74.5 eps E (kay_correction)  ->  C = 2048;
                   k_kay_pairs on the MI355X: worst 6.34 eps E = 0.0031 of C (nw2 = 128 and 129, Nm = 0, heading 0)
The kernels sit below the host figures themselves, so the margin of 16 is not drawn on.  (Every test prints its own
figure.)  k_qtf_force on the MI355X: f at most 8.6 eps of its bound 272.5 (nw = 513), f_mean at most 1.5 eps of 273.
raftx_qtf_force has derived bounds instead: f is a sum of non-negative terms, relative error <= (nw/2 + 16) eps;
f_mean <= (nw + 16) eps of its envelope 2 dw sum |S_i| |Re q_ii|.

The shapes sit on every launch edge of raft_amd/csrc/raftx_qtf.h: 64 / 128 threads of k_qtf_pairs and k_kay_pairs at
nw2 <= 64, 128 / 256 threads of k_qtf_tables at nw2 > 128, a second stride trip (129, 257), nSet * nrow not a multiple of
the 8 slabs of k_qtf_pairs (3 x 65, 1 x 1, ...), 256-lane strides and the LDS table of k_qtf_force (nw 255 .. 513)."""
import functools

import numpy as np
import pytest

from oracle import qtf_oracle
from raft_amd import qtf as rq
from raft_amd import waves
from raft_amd._abi import RaftxError
from tests import qtf_reference as R

# measured on the CPU (test_host_* print them): worst |x - ref| / (eps E) of the complex128 host implementations
HOST_SLENDER, C_SLENDER = 54.5, 1024.0           # 16 x 54.5 = 872 (54.5: tests/qtf_device_model.py; the oracle: 35.9)
HOST_KAY, C_KAY = 74.5, 2048.0                   # 16 x 74.5 = 1192
RHO, G = 1025.0, 9.81
TINY = 1e-250                                          # nothing compared may come near the subnormal range


def _check(x, ref, env, C, what, factor=1.0):
    u = R.used(x, ref, env)
    print("%s: %.3g eps E, %.3g of C = %g" % (what, u, u / C, C))
    assert u <= factor * C, (what, u, C)
    return u


# ------------------------------------------------------------------------------------------------ synthetic tables
def _triad(rng):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 2] *= -1
    return Q[:, 0], Q[:, 1], Q[:, 2]


def _strip(rng, r, q, p1, p2, rect, sign):
    """QS_N record from strip dimensions, as raft_amd.qtf.pack_qtf fills it (circular or rectangular section)"""
    rec = np.zeros(rq.QS_N)
    dl = rng.uniform(1.0, 4.0)
    if rect:
        d, dr = rng.uniform(2.0, 6.0, size=2), sign * rng.uniform(0.1, 0.5, size=2)
        v_i = d[0] * d[1] * dl
        v_e = np.pi / 12.0 * ((np.mean(d + dr)) ** 3 - (np.mean(d - dr)) ** 3)
        a_i = (d[0] + dr[0]) * (d[1] + dr[1]) - (d[0] - dr[0]) * (d[1] - dr[1])
    else:
        d, dr = rng.uniform(2.0, 9.0), sign * rng.uniform(0.1, 0.5)
        v_i = 0.25 * np.pi * d ** 2 * dl
        v_e = np.pi / 12.0 * abs((d + dr) ** 3 - (d - dr) ** 3)
        a_i = np.pi * d * dr
    if r[2] + 0.5 * dl > 0:
        v_i = v_i * (0.5 * dl - r[2]) / dl
    rec[0:3], rec[3:6], rec[6:9], rec[9:12] = r, q, p1, p2
    rec[12:18] = [rng.uniform(0.6, 1.1), rng.uniform(0.6, 1.1), rng.uniform(0.4, 0.8), v_i, v_e, a_i]
    return rec


def _member(rng, p1, p2, crosses, reach):
    m = np.zeros(rq.QM_N)
    if crosses:
        m[0] = 1.0
        m[1:4] = [rng.uniform(-reach, reach), rng.uniform(-reach, reach), 0.0]
        m[4] = rng.uniform(10.0, 60.0)
        m[5:7] = rng.uniform(0.6, 1.1, size=2)
    m[7:10], m[10:13] = p1, p2
    return m


def _table(seed, zs, crossing, reach=40.0):
    """Hand-made QtfTable: strips at the depths zs IN THIS ORDER (equal consecutive depths get different x, y), a random
    orthonormal triad per member, circular and rectangular sections, a_i of both signs; members per ``crossing``."""
    rng = np.random.default_rng(seed)
    triads = [_triad(rng) for _ in range(max(1, len(crossing)))]
    strips = []
    for i, z in enumerate(zs):
        q, p1, p2 = triads[i % len(triads)]
        r = np.array([rng.uniform(-reach, reach), rng.uniform(-reach, reach), z])
        s = _strip(rng, r, q, p1, p2, rect=(i % 3 == 1), sign=(-1.0 if i % 2 else 1.0))
        s[18] = i % len(triads)
        strips.append(s)
    members = [_member(rng, t[1], t[2], c, reach) for t, c in zip(triads, crossing)]
    tab = rq.QtfTable(np.array(strips) if strips else np.zeros((0, rq.QS_N)),
                      np.array(members) if members else np.zeros((0, rq.QM_N)), [])
    if len(zs):
        assert np.any(tab.strips[:, 17] > 0) and np.any(tab.strips[:, 17] < 0)
    return tab


def _tables():
    return dict(
        cache=_table(1, [-5.0, -5.0, -12.0, -5.0, -20.0], [True, False]),      # same z twice in a row; z back to -5 after -12
        none=_table(2, [], [True]),                                            # no strip at all, one waterline member
        three=_table(3, [-0.4, -7.5, -7.5], [True]),                           # a strip cut by the waterline
        six=_table(4, [-3.0, -30.0, -3.0, -11.0, -11.0, -1.0], [False, True, True]),
        near=_table(5, [-4.0, -9.0, -4.0, -15.0], [True], reach=3.0))          # resident-path force test only: close to the origin, a smooth QTF


def _grid(nw2, kind):
    """deep: h = 200 m, 0.3 .. 2.2 rad/s, k h from 1.9 to 99 (both sides of the k h >= 10 switch of the gradients);
    shallow: h = 30 m, 0.3 .. 1.5 rad/s, k h < 10 throughout"""
    h, wmax = (200.0, 2.2) if kind == "deep" else (30.0, 1.5)
    w = np.linspace(0.3, wmax, nw2) if nw2 > 1 else np.array([0.3 if kind == "shallow" else 0.9])
    k = np.array([waves.wave_number(x, h) for x in w])
    if kind == "deep" and nw2 > 1:
        assert np.any(k * h >= 10) and np.any(k * h < 10)
    if kind == "shallow":
        assert np.all(k * h < 10)
    return w, k, h


def _motions(rng, w):
    amp = np.array([1.0, 0.3, 0.7, 0.01, 0.02, 0.004])[:, None] / (1.0 + (w[None, :] / 0.6) ** 2)
    return amp * np.exp(1j * (rng.uniform(0, 6, 6)[:, None] + 1.5 * w[None, :]))


def _mstruc(rng):
    m = rng.uniform(1.5e7, 3e7)
    M = np.diag([m, m, m, m * 1500, m * 1500, m * 900])
    M[0, 4] = M[4, 0] = -m * 8.0
    M[1, 3] = M[3, 1] = m * 8.0
    return M


# (nw2, nSet, grid, host kay table)
SLENDER_CASES = [(1, 1, "deep", False), (2, 3, "shallow", True), (63, 1, "deep", True), (64, 3, "deep", False),
                 (65, 3, "shallow", True), (128, 1, "shallow", False), (129, 3, "deep", True), (257, 3, "deep", False)]
SLENDER_IDS = ["nw2=%d-nSet=%d-%s-%s" % (a, b, c, "kay" if d else "nokay") for a, b, c, d in SLENDER_CASES]


@functools.lru_cache(maxsize=None)
def _slender_case(nw2, nSet, kind, with_kay):
    """Inputs and the extended reference of one case (computed once per session, shared by the CPU and GPU tests)."""
    T = _tables()
    rng = np.random.default_rng([nw2, nSet])
    w, k, h = _grid(nw2, kind)
    if nSet == 1:
        tabs, betas, moving = [T["six"]], [0.7], [True]
    else:
        tabs, betas, moving = [T["cache"], T["none"], T["three"]], [0.6, 0.0, -1.1], [True, True, False]
    Xi = np.array([_motions(rng, w) if mv else np.zeros((6, nw2), dtype=complex) for mv in moving])
    Ms = np.array([_mstruc(rng) for _ in tabs])
    kay = None
    if with_kay:
        kay = 1e5 * (rng.normal(size=(nSet, nw2, nw2, 6)) + 1j * rng.normal(size=(nSet, nw2, nw2, 6)))
        kay *= (np.arange(nw2)[None, :] >= np.arange(nw2)[:, None])[None, :, :, None]
    ref = [R.qtf_slender_ref(tabs[s], Xi[s], betas[s], w, k, h, RHO, G, Ms[s], None if kay is None else kay[s])
           for s in range(nSet)]
    E = np.array([e for _, e in ref])
    assert E[E > 0].min() > TINY
    return dict(tabs=tabs, betas=betas, w=w, k=k, h=h, Xi=Xi, Ms=Ms, kay=kay, ref=np.array([q for q, _ in ref]), E=E)


def _device_slender(ctx, c, **kw):
    return ctx.qtf_slender(c["tabs"], c["Xi"], c["betas"], c["w"], c["k"], c["h"], RHO, G, c["Ms"], c["kay"], **kw)


@pytest.mark.parametrize("nw2,nSet,kind,with_kay", SLENDER_CASES, ids=SLENDER_IDS)
def test_host_oracle_against_extended_reference(nw2, nSet, kind, with_kay):
    c = _slender_case(nw2, nSet, kind, with_kay)
    for s in range(nSet):
        q = qtf_oracle.qtf_slender_body(c["tabs"][s], c["Xi"][s], c["betas"][s], c["w"], c["k"], c["h"], RHO, G, c["Ms"][s],
                                        None if c["kay"] is None else c["kay"][s])
        _check(q, c["ref"][s], c["E"][s], C_SLENDER, "complex128 oracle, set %d" % s, factor=0.25)


def test_device_model_against_extended_reference():
    """tests/qtf_device_model.py (the strip-frame formulation of k_qtf_pairs in complex128 NumPy): strip terms alone,
    i.e. the reference with no member, no Pinkster term (M_struc = 0) and the lower triangle left empty."""
    from tests import qtf_device_model as dm
    tab = _tables()["cache"]
    bare = rq.QtfTable(tab.strips, np.zeros((0, rq.QM_N)), [])
    w, k, h = _grid(65, "deep")
    Xi = _motions(np.random.default_rng(8), w)
    ref, E = R.qtf_slender_ref(bare, Xi, 0.6, w, k, h, RHO, G, np.zeros((6, 6)))
    up = (w[None, :] >= w[:, None])[:, :, None]
    q = np.transpose(dm.qtf_strips(bare, Xi, 0.6, w, k, h, RHO, G), (1, 2, 0))
    _check(q, np.where(up, ref, 0), np.where(up, E, 0), C_SLENDER, "device model", factor=0.25)


@pytest.mark.gpu
@pytest.mark.parametrize("nw2,nSet,kind,with_kay", SLENDER_CASES, ids=SLENDER_IDS)
def test_hip_qtf_slender_against_extended_reference(hip_ctx, nw2, nSet, kind, with_kay):
    c = _slender_case(nw2, nSet, kind, with_kay)
    q = _device_slender(hip_ctx, c)
    assert q.shape == c["ref"].shape                    # every set, entry and DOF is compared: nothing is masked out
    for s in range(nSet):
        _check(q[s], c["ref"][s], c["E"][s], C_SLENDER, "k_qtf_pairs, set %d" % s)
        off = ~np.eye(nw2, dtype=bool)
        assert np.array_equal(q[s][off], np.conj(np.transpose(q[s], (1, 0, 2)))[off])


@pytest.mark.gpu
@pytest.mark.parametrize("case,world", [(SLENDER_CASES[4], 3), (SLENDER_CASES[1], 5)], ids=["nw2=65-world=3", "nw2=2-world=5"])
def test_hip_qtf_slender_rows_sum_to_the_full_matrix(hip_ctx, case, world):
    c = _slender_case(*case)
    full = _device_slender(hip_ctx, c)
    parts = [_device_slender(hip_ctx, c, rows=(r, world)) for r in range(world)]
    total = parts[0]
    for p in parts[1:]:
        assert not np.any((np.abs(total) > 0) & (np.abs(p) > 0))               # disjoint support: the sum is exact
        total = total + p
    assert np.array_equal(total.view(np.float64), full.view(np.float64))
    for s in range(case[1]):
        _check(full[s], c["ref"][s], c["E"][s], C_SLENDER, "rows, set %d" % s)


# ------------------------------------------------------------------------------------------------ Kim & Yue
KAY_NW = [1, 64, 65, 128, 129]
KAY_SETS = [("two", 0.4), ("none", 0.0), ("two", 0.0)]                        # two members in one set; a set with no item


@functools.lru_cache(maxsize=None)
def _kay_case(nw2, sets, Nm):
    w, k = R.kay_grid(nw2)
    geoms = [R.kay_geometry(name) for name, _ in sets]
    betas = np.array([b for _, b in sets])
    x = np.concatenate([k * Rr for Rr in R.KAY_R])
    assert x.min() <= 1.001e-3 or nw2 == 1
    ref = [R.kay_ref(rq.kay_items(gm, b), w, k, b, R.KAY_DEPTH, RHO, G, Nm) for gm, b in zip(geoms, betas)]
    E = np.array([e for _, e in ref])
    assert not np.any(E) or E[E > 0].min() > TINY
    return dict(w=w, k=k, geoms=geoms, betas=betas, ref=np.array([q for q, _ in ref]), E=E)


def _kay_tabs(c):
    return [rq.QtfTable(np.zeros((0, rq.QS_N)), np.zeros((0, rq.QM_N)), gm) for gm in c["geoms"]]


def test_kay_grid_reaches_the_branch_points_of_the_device_bessel_functions():
    """x = k R runs from 1e-3 to 12 and holds 1, 2, 3, 5, 8, 10, 12 exactly (order above, at and below the argument;
    libm's switches at 2 and 8); the arguments one ulp either side of 2 and 8 (and next to 1 and 12) come with radii one ulp off 4."""
    _, k = R.kay_grid(129)
    x = np.concatenate([k * Rr for Rr in R.KAY_R])
    assert x.min() == 1e-3 and x.max() == 12.0 and set(R.KAY_X_SPECIAL) <= set(x)
    for n in (64, 65, 128):
        assert set(R.KAY_X_SPECIAL) <= set(R.kay_grid(n)[1] * R.KAY_R[0])
    lo, hi = R.KAY_BRANCH_K * np.nextafter(4.0, 0.0), R.KAY_BRANCH_K * np.nextafter(4.0, 8.0)
    for xs, lo_, hi_ in zip((1.0, 2.0, 8.0, 12.0), lo, hi):
        assert lo_ < xs < hi_ and hi_ - lo_ <= 3 * np.spacing(xs)
        if xs in (2.0, 8.0):                                                    # exactly the neighbours of libm's switches
            assert lo_ == np.nextafter(xs, 0.0) and hi_ == np.nextafter(xs, 100.0)


def test_bessel_fixture_against_mpmath():
    """a sample of tests/golden/kay_hankel_ref.npz regenerated (oracle/make_kay_hankel.py); the fixture holds exactly the
    arguments of the tests"""
    pytest.importorskip("mpmath", reason="mpmath is not installed: the committed fixture cannot be regenerated here")
    from oracle import make_kay_hankel as mk
    xs = R.kay_fixture_arguments()
    with np.load(R.GOLDEN) as z:
        assert np.array_equal(z["x"].view(np.uint64), xs.view(np.uint64))
        pick = np.unique(np.concatenate([np.arange(0, len(xs), 23), [len(xs) - 1], np.nonzero(np.isin(xs, [2.0, 8.0]))[0]]))
        v = mk.values(xs[pick])
        for i, name in enumerate(("J_hi", "J_lo", "Y_hi", "Y_lo")):
            assert np.array_equal(z[name][pick], v[i]), name
        assert np.all(np.abs(z["J_lo"]) <= np.abs(z["J_hi"]) * 2.0 ** -52)
    J, Y = R.bessel(np.array([2.0]))
    assert abs(float(J[0, 0]) - 0.22389077914123567) < 1e-16 and abs(float(Y[0, 1]) + 0.10703243154093755) < 1e-16


@pytest.mark.parametrize("nw2", KAY_NW)
def test_host_kay_correction_against_extended_reference(nw2):
    c = _kay_case(nw2, tuple(KAY_SETS), 10)
    for s, (gm, b) in enumerate(zip(c["geoms"], c["betas"])):
        host = rq.kay_correction(gm, c["w"], c["k"], b, R.KAY_DEPTH, rho=RHO, g=G, Nm=10)
        _check(host, c["ref"][s], c["E"][s], C_KAY, "kay_correction, set %d" % s, factor=0.25)


@pytest.mark.parametrize("Nm", [0, 10])
def test_host_kay_single_waterline_and_branch_points(Nm):
    for sets in ((("wl", 0.3),), (("below", 0.0), ("mid", 0.0), ("above", 0.0))):
        c = _kay_branch_case(sets, Nm)
        for s, (gm, b) in enumerate(zip(c["geoms"], c["betas"])):
            host = rq.kay_correction(gm, c["w"], c["k"], b, R.KAY_DEPTH, rho=RHO, g=G, Nm=Nm)
            _check(host, c["ref"][s], c["E"][s], C_KAY, "kay_correction %s Nm=%d" % (sets[s][0], Nm), factor=0.25)


@functools.lru_cache(maxsize=None)
def _kay_branch_case(sets, Nm):
    """the four wave numbers that put k R within one ulp of 1, 2, 8 and 12, for radii 4 -+ 1 ulp"""
    k = R.KAY_BRANCH_K
    w = np.sqrt(G * k * np.tanh(k * R.KAY_DEPTH))
    geoms = [R.kay_geometry(name) for name, _ in sets]
    betas = np.array([b for _, b in sets])
    ref = [R.kay_ref(rq.kay_items(gm, b), w, k, b, R.KAY_DEPTH, RHO, G, Nm) for gm, b in zip(geoms, betas)]
    E = np.array([e for _, e in ref])
    assert E[E > 0].min() > TINY
    return dict(w=w, k=k, geoms=geoms, betas=betas, ref=np.array([q for q, _ in ref]), E=E)


def _device_kay(ctx, c, Nm):
    return ctx.qtf_kay(_kay_tabs(c), c["betas"], c["w"], c["k"], R.KAY_DEPTH, RHO, G, Nm=Nm, fetch=True)


@pytest.mark.gpu
@pytest.mark.parametrize("Nm", [0, 10])
@pytest.mark.parametrize("nw2", KAY_NW)
def test_hip_qtf_kay_against_extended_reference(hip_ctx, nw2, Nm):
    c = _kay_case(nw2, tuple(KAY_SETS), Nm)
    dev = _device_kay(hip_ctx, c, Nm)
    for s in range(len(KAY_SETS)):
        _check(dev[s], c["ref"][s], c["E"][s], C_KAY, "k_kay_pairs, set %d" % s)
    assert not np.any(dev[1])                                                   # the set without items
    assert np.any(c["ref"][0][..., 3:]) and np.any(c["ref"][0][..., :3])


@pytest.mark.gpu
@pytest.mark.parametrize("Nm", [0, 10])
def test_hip_qtf_kay_single_waterline_item_and_branch_points(hip_ctx, Nm):
    """Nm = 0 with one waterline item leaves Omega_0 alone, 1 / (H'_1 conj H'_0) - 1 / (H'_0 conj H'_1): a wrong row of
    the device table 1 / H'_n cannot hide in a sum.  The three-set batch walks x within one ulp of 1, 2, 8, 12."""
    for sets in ((("wl", 0.3),), (("below", 0.0), ("mid", 0.0), ("above", 0.0))):
        c = _kay_branch_case(sets, Nm)
        assert len(rq.kay_items(c["geoms"][0], 0.0)) == (1 if sets[0][0] == "wl" else 2)
        dev = _device_kay(hip_ctx, c, Nm)
        for s in range(len(sets)):
            _check(dev[s], c["ref"][s], c["E"][s], C_KAY, "k_kay_pairs %s Nm=%d" % (sets[s][0], Nm))


# ------------------------------------------------------------------------------------------------ second-order force
# (nw, nw2, nSet)
FORCE_CASES = [(1, 2, 1), (2, 3, 3), (63, 50, 1), (64, 2, 3), (65, 3, 1), (255, 50, 3), (256, 2, 1), (257, 3, 3), (513, 50, 3)]
S0_SCALE = (1.0, 1e-6, 1e5)


def _force_grids(nw, nw2):
    """a non-uniform second-order grid from 0.3 rad/s and first-order bins below it, ON w2[0], on interior grid points,
    ON w2[-1] and above it (as many of these as nw allows)"""
    rng = np.random.default_rng([nw, nw2])
    w2 = 0.3 + np.concatenate([[0.0], np.cumsum(rng.uniform(0.6, 1.4, nw2 - 1))]) * (2.0 / (nw2 - 1))
    must = [w2[0], w2[-1]] + list(w2[1:-1][:: max(1, (nw2 - 2) // 5)])
    if nw == 1:
        return w2, np.array([w2[0]])
    if nw == 2:
        return w2, np.array([w2[0], w2[-1]])
    fill = np.linspace(0.5 * w2[0], 1.15 * w2[-1], nw)
    w = np.unique(np.concatenate([must, fill]))
    while len(w) > nw:                                                          # drop fill points, never the ones that must stay
        i = next(j for j in range(1, len(w) - 1) if w[j] not in must)
        w = np.delete(w, i)
    assert len(w) == nw and w[0] < w2[0] and w[-1] > w2[-1] and np.all(np.isin(must, w))
    return w2, w


def _smooth_qtf(w2, seed):
    """Hermitian, every DOF at its own scale and sign, phase turning slowly between grid points"""
    rng = np.random.default_rng(seed)
    c = 0.3 * np.arange(1, 7) / np.max(np.diff(w2))
    A = rng.choice([-1.0, 1.0], 6) * 10.0 ** np.arange(6)
    g = 1.0 / (1.0 + w2 ** 2)
    d = w2[:, None] - w2[None, :]
    return A * (g[:, None] * g[None, :])[:, :, None] * np.exp(-1j * c * d[:, :, None])


@functools.lru_cache(maxsize=None)
def _force_case(nw, nw2, nSet):
    w2, w = _force_grids(nw, nw2)
    dw = 0.01
    S0 = np.array([S0_SCALE[s] * (0.5 + np.sin(3.0 * w + s) ** 2) * np.exp(-w) for s in range(nSet)])
    qtf = np.array([_smooth_qtf(w2, [nw, s]) for s in range(nSet)])
    ref = [R.qtf_force_ref(qtf[s], w2, w, dw, S0[s]) for s in range(nSet)]
    return dict(w2=w2, w=w, dw=dw, S0=S0, qtf=qtf, ref=ref)


def _check_force(fm, f, ref, nw, what, factor=1.0):
    f_ref, m_ref, m_env = ref
    f, fm = np.asarray(f, dtype=R.LD), np.asarray(fm, dtype=R.LD)
    zero = f_ref == 0
    assert np.all(f[zero] == 0), what
    assert np.all(f_ref[~zero] > TINY) and np.all(m_env[m_env > 0] > TINY)
    rel = float(np.max(np.abs(f - f_ref)[~zero] / f_ref[~zero])) / R.EPS if np.any(~zero) else 0.0
    um = R.used(fm, m_ref, m_env)
    print("%s: f %.3g eps of %.1f, f_mean %.3g eps of %.1f" % (what, rel, nw / 2 + 16, um, nw + 16))
    assert rel <= factor * (nw / 2 + 16) and um <= factor * (nw + 16), (what, rel, um)


@pytest.mark.parametrize("nw,nw2,nSet", FORCE_CASES)
def test_host_hydro_force_2nd_against_extended_reference(nw, nw2, nSet):
    """SciPy's RegularGridInterpolator (raft_amd.qtf.hydro_force_2nd) against the interpolation rules written out"""
    c = _force_case(nw, nw2, nSet)
    for s in range(nSet):
        fm, f = rq.hydro_force_2nd(c["qtf"][s], c["w2"], c["w"], c["dw"], c["S0"][s])
        _check_force(fm, f, c["ref"][s], nw, "hydro_force_2nd set %d" % s, factor=0.25)


@pytest.mark.gpu
@pytest.mark.parametrize("nw,nw2,nSet", FORCE_CASES)
def test_hip_qtf_force_against_extended_reference(hip_ctx, nw, nw2, nSet):
    c = _force_case(nw, nw2, nSet)
    fm, f = hip_ctx.qtf_force(c["w2"], c["w"], c["dw"], c["S0"], qtf=c["qtf"])
    for s in range(nSet):
        _check_force(fm[s], f[s], c["ref"][s], nw, "k_qtf_force set %d" % s)


@pytest.mark.gpu
@pytest.mark.parametrize("nw,nw2,nSet", [(65, 3, 1), (255, 50, 3)])
def test_hip_qtf_force_resident_path(hip_ctx, nw, nw2, nSet):
    """the QTFs raftx_qtf_slender leaves on the device: same bits as the host-QTF path fed with the fetched copy, and
    inside the bounds against the reference evaluated on that copy"""
    tab = _tables()["near"]
    rng = np.random.default_rng([nw, nw2, 7])
    w2, w = _force_grids(nw, nw2)
    w2 = 0.3 + (w2 - 0.3) * 0.35                                                # 0.3 .. 1.0 rad/s: k x stays below one radian
    w = 0.3 + (w - 0.3) * 0.35
    k2 = np.array([waves.wave_number(x, 200.0) for x in w2])
    Xi = np.array([_motions(rng, w2) for _ in range(nSet)])
    Ms = np.array([_mstruc(rng) for _ in range(nSet)])
    S0 = np.array([S0_SCALE[s] * (0.5 + np.sin(3.0 * w + s) ** 2) * np.exp(-w) for s in range(nSet)])
    q = hip_ctx.qtf_slender([tab] * nSet, Xi, [0.2 * s for s in range(nSet)], w2, k2, 200.0, RHO, G, Ms)
    fm_r, f_r = hip_ctx.qtf_force(w2, w, 0.01, S0, qtf=None, n_set=nSet)
    fm_h, f_h = hip_ctx.qtf_force(w2, w, 0.01, S0, qtf=q)
    assert np.array_equal(fm_r.view(np.uint64), fm_h.view(np.uint64)) and np.array_equal(f_r.view(np.uint64), f_h.view(np.uint64))
    for s in range(nSet):
        _check_force(fm_r[s], f_r[s], R.qtf_force_ref(q[s], w2, w, 0.01, S0[s]), nw, "resident set %d" % s)


@pytest.mark.gpu
def test_hip_qtf_force_refuses_bad_shapes(hip_ctx):
    """nw2 = 1 has no interval to interpolate in; nw = 5457 asks for 8 (nw + (nw+1)/2 + 8) = 65552 bytes of LDS, more than
    the 64 KB of a workgroup: both are refused with a message, before any launch (5456, the largest that fits, is not
    launched here either: only the refusal is tested)"""
    with pytest.raises(RaftxError, match="bad arguments"):
        hip_ctx.qtf_force(np.array([0.5]), np.array([0.5, 0.6]), 0.1, np.ones((1, 2)), qtf=np.ones((1, 1, 1, 6), dtype=complex))
    nw = 5457
    assert 8 * (nw + (nw + 1) // 2 + 8) > 65536 >= 8 * (nw - 1 + nw // 2 + 8)
    w2 = np.array([0.3, 1.0, 2.0])
    with pytest.raises(RaftxError, match="LDS"):
        hip_ctx.qtf_force(w2, np.linspace(0.2, 2.1, nw), 0.01, np.ones((1, nw)), qtf=_smooth_qtf(w2, 1)[None])
