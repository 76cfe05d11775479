"""The linear solvers against tests/linear_solve_reference.py -- the contract of include/raftx.h in long double and the normwise
backward error of a solution, one GATE for everything -- on the inputs of tests/linear_solve_cases.py.  This file is the CPU
half: the inputs keep what their families promise (so that a later change of seed cannot hollow them out), LAPACK, the fp64
model of the kernels' elimination and the CPU oracle sit inside GATE on every input, every seeded fault of the model is
thrown out by the same checker, and a NaN or an exactly singular system stays in its own (system, bin).  The checkers are
written once and run on the HIP library in tests/test_hip_linear_solve.py.

The oracle's coupled solve multiplies by an explicit inverse (as the reference does): its backward error grows with the
condition number, which is why every input is asserted to have cond_inf <= 1e4."""
import functools

import numpy as np
import pytest

from raft_amd._abi import RaftxError, WANT_BDRAG, WANT_FWAVE, WANT_Z
from tests import linear_solve_cases as K
from tests import linear_solve_reference as R
from tests.util import random_matrices, random_strips, synthetic_cases

COND_MAX = 1e4


def used(A, absA, X, F, what, mask=None):
    """Prints the fraction of GATE the solution uses (worst (system, bin) of mask) and asserts that it is within it."""
    om = R.omega(A, absA, X, F)
    worst = float(om[mask].max() if mask is not None else om.max())
    print("%s: uses %.3g of the gate" % (what, worst / R.GATE))
    assert worst <= R.GATE, (what, worst)
    return worst


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ------------------------------------------------------------------ the inputs with their references (computed once)
@functools.lru_cache(maxsize=16)
def coupled_input(family, nUnit, nRhs, nw):
    c = K.coupled(family, nUnit, nRhs, nw)
    A, absA = R.assemble(c["w"], 6 * nUnit, blocks=c["Zblk"], M=c["Mc"], B=c["Bc"], C=c["Cc"])
    for v in list(c.values()) + [A, absA]:
        v.flags.writeable = False
    return c, A, absA


@functools.lru_cache(maxsize=4)
def dense_input(family, n, nRhs, freq_M=False):
    c = K.dense(family, n, nRhs, freq_M=freq_M)
    A, absA = R.assemble(c["w"], n, M=c["M"], B=c["B"], C=c["C"])
    for v in list(c.values()) + [A, absA]:
        v.flags.writeable = False
    return c, A, absA


def _coupled_model_args(c):
    return dict(blocks=c["Zblk"], M=c["Mc"], B=c["Bc"], C=c["Cc"])


def _dense_model_args(c):
    return dict(M=c["M"], B=c["B"], C=c["C"])


COUPLED_PARAMS = [(f, nu, nr) for f in K.FAMILIES for nu, nr, _ in K.COUPLED_SHAPES]
COUPLED_NW = {(nu, nr): nws for nu, nr, nws in K.COUPLED_SHAPES}
DENSE_PARAMS = [(f, n, nr) for f in K.DENSE_FAMILIES for n, nr in K.DENSE_SHAPES + [K.DENSE_L2_SHAPE]]


def _dense_case(family, n, nRhs):
    return dense_input(family, n, nRhs, freq_M=(n, nRhs) == K.DENSE_L2_SHAPE)


# ------------------------------------------------------------------ checkers shared with the device tests
def check_coupled(ctx, family, nUnit, nRhs):
    worst = 0.0
    for nw in COUPLED_NW[nUnit, nRhs]:
        c, A, absA = coupled_input(family, nUnit, nRhs, nw)
        X = ctx.solve_system(c["w"], c["Zblk"], c["F"], c["Mc"], c["Bc"], c["Cc"])
        worst = max(worst, used(A, absA, X, c["F"], "%s (%d units, %d rhs, %d bins)" % (family, nUnit, nRhs, nw)))
    return worst


def check_dense(ctx, family, n, nRhs):
    c, A, absA = _dense_case(family, n, nRhs)
    X = ctx.solve_dense_batch(c["w"], c["M"], c["B"], c["C"], c["F"])
    return used(A, absA, X, c["F"], "dense %s (n = %d, %d rhs)" % (family, n, nRhs))


def check_dense_resident(ctx):
    c = K.dense_resident()
    n = c["C"].shape[-1]
    rep = lambda a: np.repeat(a, 2, axis=0)                                  # system s takes the matrices of set s // 2
    A, absA = R.assemble(c["w"], n, M=rep(c["M"]), B=rep(c["B"]), C=rep(c["C"]), Badd=c["Badd"])
    assert float(R.cond_inf(A).max()) <= COND_MAX
    ctx.dense_resident(c["w"], c["M"], c["B"], c["C"])
    try:
        X = ctx.solve_dense_resident(c["F"], Badd=c["Badd"])
    finally:
        ctx.dense_resident(None, None, None, None)
    used(A, absA, R.lapack(A, c["F"]), c["F"], "dense resident [LAPACK]")
    return used(A, absA, X, c["F"], "dense resident with Badd")


def check_refused(ctx):
    """Shapes beyond 150 KiB of LDS are refused with the entry's error, before any launch."""
    for nUnit, nRhs in K.REFUSED_SHAPES:
        c = K.coupled("dominant", nUnit, nRhs, 2)
        with pytest.raises(RaftxError, match="does not fit the LDS-resident solver"):
            ctx.solve_system(c["w"], c["Zblk"], c["F"], c["Mc"], c["Bc"], c["Cc"])


def check_containment(ctx, nUnit, nRhs, nw, iw, kind, family="permuted"):
    """kind "nan": one NaN in a unit block of (system 1, bin iw); "singular": column 7 % n of that (system, bin) is zero in
    every addend (the coupling's column in all bins, the unit block's in bin iw).  Exactly that (system, bin) is non-finite,
    in every right-hand side; every other one stays within GATE of ITS reference."""
    c, _, _ = coupled_input(family, nUnit, nRhs, nw)
    c = {k: np.array(v) for k, v in c.items()}
    n, j = 6 * nUnit, 7 % (6 * nUnit)
    if kind == "nan":
        c["Zblk"][1, nUnit - 1, 2, 3, iw] = np.nan
    else:
        for a in ("Mc", "Bc", "Cc"):
            c[a][1, :, j] = 0.0
        c["Zblk"][1, j // 6, :, j % 6, iw] = 0.0
    X = ctx.solve_system(c["w"], c["Zblk"], c["F"], c["Mc"], c["Bc"], c["Cc"])
    bad = ~np.isfinite(X.real) | ~np.isfinite(X.imag)
    assert np.all(bad[1, :, :, iw].any(axis=-1)), "a right-hand side of the poisoned (system, bin) is finite"
    good = np.ones((K.N_SYS, nw), dtype=bool)
    good[1, iw] = False
    assert not bad[np.broadcast_to(good[:, None, None, :], bad.shape)].any(), "a non-finite value outside the poisoned (system, bin)"
    A, absA = R.assemble(c["w"], n, blocks=np.nan_to_num(c["Zblk"]), M=c["Mc"], B=c["Bc"], C=c["Cc"])
    used(A, absA, X, c["F"], "%s at bin %d of %d (%d units, %d rhs): the others" % (kind, iw, nw, nUnit, nRhs), mask=good)


def check_repeat(solve):
    """Two runs of one batch: the same bits (a race in a row buffer or a workspace would show)."""
    assert _same_bits(solve(), solve())


# ---- the resident coupled solve: fed from what a real fixed point left on the device
RESIDENT_PARAMS = [(nu, nh, mode) for nu in (2, 5, 6) for nh in (1, 3) for mode in ("Z", "BDRAG")]
N_GROUP, N_CASE = 2, 2


def check_resident(ctx, nUnit, nHead, mode):
    """solve_dynamics_device, then solve_system_resident with coupling of the forced kind (entries 1e6 times the largest
    |Z|, built after the fetch) and of the dominant kind.  The reference is evaluated on what the solve itself left: the
    fetched Z (mode "Z") or Z rebuilt in long double from M0, B0, C0 and the fetched B_drag (mode "BDRAG": the kernels
    assemble it on the fly), and the fetched F_wave -- it owes nothing to the fixed point."""
    n, nD = 6 * nUnit, N_GROUP * nUnit
    for nw in (5, 8):
        rng = np.random.default_rng([nUnit, nHead, nw])
        tables = [random_strips(rng, int(S)) for S in rng.integers(2, 6, size=nD)]
        M0, B0, C0, _ = random_matrices(rng, nD)
        w, k, zeta, beta = synthetic_cases(rng, N_CASE, nHead, nw, wmin=0.3)
        ctx.upload_designs(tables, M0, B0, C0, nw)
        ctx.upload_cases(w, k, 200.0, 1025.0, 9.81, zeta, beta)
        ctx.solve_dynamics_device(2, 0.01, 0.1, want_mask=(WANT_Z if mode == "Z" else WANT_BDRAG) | WANT_FWAVE)
        out = ctx.fetch_results(want_Xi=False, want_Z=mode == "Z", want_B=mode == "BDRAG", want_F=True)
        if mode == "Z":
            Z, absZ = out["Z"].astype(R.CLD), None
        else:
            wl = np.asarray(w, dtype=R.LD)
            m, b0, bd, c0 = (np.asarray(a, dtype=R.LD)[..., None] for a in (M0[:, None], B0[:, None], out["B_drag"], C0[:, None]))
            Z = (-wl * wl * m + c0) + 1j * (wl * (b0 + bd))
            absZ = wl * wl * np.abs(m) + np.abs(c0) + wl * (np.abs(b0) + np.abs(bd))
        # system (g, c): units g * nUnit + u of case c
        pick = lambda a: np.moveaxis(a.reshape((N_GROUP, nUnit) + a.shape[1:]), 2, 1).reshape((N_GROUP * N_CASE, nUnit) + a.shape[2:])
        blocks, abs_blocks = pick(Z), None if absZ is None else pick(absZ)
        F = np.moveaxis(pick(out["F_wave"]), 2, 1).reshape(N_GROUP * N_CASE, nHead, n, nw)   # [s,u,ih,6,w] -> [s,ih,(u,6),w]
        assert np.all(np.abs(F).max(axis=(2, 3)) > 0.0)
        zmax = float(np.abs(Z).max())
        sym = rng.normal(size=(N_GROUP, n, n)) * 1e5
        couplings = {"forced": K.forced_coupling(rng, N_GROUP, n, 1e6 * zmax),
                     "dominant": (1e4 * rng.normal(size=(N_GROUP, n, n)), 1e3 * rng.normal(size=(N_GROUP, n, n)),
                                  sym + np.transpose(sym, (0, 2, 1)))}
        for family, (Mc, Bc, Cc) in couplings.items():
            rep = lambda a: np.repeat(a, N_CASE, axis=0)
            A, absA = R.assemble(w, n, blocks=blocks, M=rep(Mc), B=rep(Bc), C=rep(Cc), abs_blocks=abs_blocks)
            X = ctx.solve_system_resident(nUnit, Mc, Bc, Cc).reshape(N_GROUP * N_CASE, nHead, n, nw)
            what = "resident %s from %s (%d units, %d headings, %d bins)" % (family, mode, nUnit, nHead, nw)
            used(A, absA, R.lapack(A, F), F, what + " [LAPACK]")
            used(A, absA, X, F, what)


# ------------------------------------------------------------------ the inputs keep their promises
def _traces(A64):
    """pivot traces of the model, per (system, bin)"""
    out = {}
    for s in range(A64.shape[0]):
        for i in range(A64.shape[1]):
            out[s, i] = []
            R.eliminate(A64[s, i], np.zeros((A64.shape[-1], 1)), trace=out[s, i])
    return out


def _check_promises(family, A, A64, n):
    cond = float(R.cond_inf(A).max())
    assert cond <= COND_MAX, cond
    if family == "forced":
        tr = _traces(A64)
        for (s, i), t in tr.items():
            assert all(mag >= 1e6 * other for _, mag, other, _ in t[:-1]), "a pivot of the forced family is not unique"
            rows = np.array([r for r, _, _, _ in t])
            assert sorted(rows) == list(range(n))
            if n > 16 and s < 2:
                assert (rows < 16).any() and (rows >= 16).any()
                if s == 1:                                 # consecutive pivots alternate between the lower and upper rows
                    assert np.all((rows[:-1] < n // 2) != (rows[1:] < n // 2))
    if family == "ties":
        tr = _traces(A64)
        for s in range(A64.shape[0]):
            assert max(cnt for i in range(A64.shape[1]) for _, _, _, cnt in tr[s, i]) >= 3, "no exact ties in system %d" % s
    return cond


@pytest.mark.parametrize("family,nUnit,nRhs", COUPLED_PARAMS)
def test_coupled_inputs_and_cpu_solvers(oracle_ctx, family, nUnit, nRhs):
    """The family's promises; LAPACK, the fp64 model and the oracle within GATE; every fault of the model outside it."""
    n = 6 * nUnit
    for nw in COUPLED_NW[nUnit, nRhs]:
        c, A, absA = coupled_input(family, nUnit, nRhs, nw)
        args = _coupled_model_args(c)
        cond = _check_promises(family, A, R.assemble_fp64(c["w"], n, **args), n)
        what = "%s (%d units, %d rhs, %d bins, cond %.3g)" % (family, nUnit, nRhs, nw, cond)
        used(A, absA, R.lapack(A, c["F"]), c["F"], what + " [LAPACK]")
        used(A, absA, R.model(c["w"], n, c["F"], **args), c["F"], what + " [model]")
    check_coupled(oracle_ctx, family, nUnit, nRhs)
    # the faults, at the shape's largest nw
    for fault in R.FAULTS:
        if not R.applies(fault, nUnit, nRhs, nw, n) or (fault in R.PIVOT_FAULTS and family != "forced"):
            continue
        om = float(R.omega(A, absA, R.model(c["w"], n, c["F"], fault=fault, **args), c["F"]).max())
        print("%s, fault %s: %.3g times the gate" % (what, fault, om / R.GATE))
        assert om > (100.0 if fault in R.PIVOT_FAULTS else 1.0) * R.GATE, (fault, om)


@pytest.mark.parametrize("family,n,nRhs", DENSE_PARAMS)
def test_dense_inputs_and_cpu_solvers(oracle_ctx, family, n, nRhs):
    c, A, absA = _dense_case(family, n, nRhs)
    args = _dense_model_args(c)
    cond = _check_promises(family, A, R.assemble_fp64(c["w"], n, **args), n)
    what = "dense %s (n = %d, %d rhs, cond %.3g)" % (family, n, nRhs, cond)
    used(A, absA, R.lapack(A, c["F"]), c["F"], what + " [LAPACK]")
    used(A, absA, R.model(c["w"], n, c["F"], **args), c["F"], what + " [model]")
    used(A, absA, R.model(c["w"], n, c["F"], jordan=True, **args), c["F"], what + " [model, Gauss-Jordan]")
    check_dense(oracle_ctx, family, n, nRhs)
    for fault in R.FAULTS:
        if not R.applies(fault, 0, nRhs, K.DENSE_NW, n) or (fault in R.PIVOT_FAULTS and family != "forced"):
            continue
        om = float(R.omega(A, absA, R.model(c["w"], n, c["F"], fault=fault, jordan=True, **args), c["F"]).max())
        print("%s, fault %s: %.3g times the gate" % (what, fault, om / R.GATE))
        assert om > (100.0 if fault in R.PIVOT_FAULTS else 1.0) * R.GATE, (fault, om)


def test_gate_follows_from_lapack():
    """GATE is eight times LAPACK's worst multiple of n u over ALL inputs, rounded up to a power of two."""
    worst = 0.0
    for family, nUnit, nRhs in COUPLED_PARAMS:
        for nw in COUPLED_NW[nUnit, nRhs]:
            c, A, absA = coupled_input(family, nUnit, nRhs, nw)
            worst = max(worst, float(R.omega(A, absA, R.lapack(A, c["F"]), c["F"]).max()))
    for family, n, nRhs in DENSE_PARAMS:
        c, A, absA = _dense_case(family, n, nRhs)
        worst = max(worst, float(R.omega(A, absA, R.lapack(A, c["F"]), c["F"]).max()))
    print("LAPACK's worst over all inputs: %.3g n u; GATE = %g" % (worst, R.gate_from(worst)))
    assert R.GATE == R.gate_from(worst)


def test_oracle_dense_resident(oracle_ctx):
    check_dense_resident(oracle_ctx)


def test_lds_shapes_sit_on_their_edges():
    """The refused shapes are beyond 150 KiB, the largest accepted one is exactly 150 KiB, (11,1) is the first over 64 KiB
    (the device half runs them), and the bins per workgroup are 4, 2 and 1 as the shape table says."""
    assert K.lds_bytes(16, 4) == (1, 150 * 1024) and K.lds_bytes(11, 1) == (1, 70752) and K.lds_bytes(10, 3) == (1, 60480)
    assert all(K.lds_bytes(nu, nr)[1] > 150 * 1024 for nu, nr in K.REFUSED_SHAPES)
    assert [K.lds_bytes(*s)[0] for s in K.LDS_SHAPES] == [4, 4, 2, 2, 1, 1, 1, 1]


CONTAINMENT = [(3, 2, 5, 2), (3, 2, 5, 4), (6, 1, 3, 2), (1, 1, 5, 2)]          # (nUnit, nRhs, nw, poisoned bin)


@pytest.mark.parametrize("kind", ["nan", "singular"])
@pytest.mark.parametrize("nUnit,nRhs,nw,iw", CONTAINMENT)
def test_oracle_contains_a_poisoned_bin(oracle_ctx, nUnit, nRhs, nw, iw, kind):
    check_containment(oracle_ctx, nUnit, nRhs, nw, iw, kind)


@pytest.mark.parametrize("nUnit,nHead,mode", RESIDENT_PARAMS)
def test_oracle_resident_coupled_solve(oracle_ctx, nUnit, nHead, mode):
    check_resident(oracle_ctx, nUnit, nHead, mode)
