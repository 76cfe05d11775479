"""What the linear solvers (raftx_solve_system[_resident], raftx_solve_dense[_batch|_resident]) are held to: the contract of
include/raftx.h assembled in numpy.clongdouble and the NORMWISE BACKWARD ERROR of a returned solution against it.

  assemble   A = blockdiag(blocks) - w^2 M + i w (B [+ Badd]) + C per (system, bin), and absA = |blocks| + w^2 |M| + w (|B| +
             |Badd|) + |C|: the kernels form fma(-w^2, m, k), so cancellation BETWEEN the addends is a perturbation of the
             data (each addend perturbed by one rounding), not an error of the solve.
  omega      max_r ||F_r - A X_r||_inf / (||absA||_inf ||X_r||_inf + ||F_r||_inf) per (system, bin), in long double, in
             units of n u (u = 2^-53); inf where the solution is not finite.  A solver is backward stable when this is a
             small constant -- whatever the condition number, whichever of several equally large pivots it took.
  model      Gaussian elimination in plain fp64 NumPy with the kernels' pivot rule (first largest |re| + |im|), and with
             seeded faults (FAULTS) that the CPU tests use to prove that the gate has teeth.

GATE is ONE constant for the device, LAPACK and the model, and is not tuned on the device: eight times the worst multiple of
n u that numpy.linalg.solve (complex128, zgesv) reaches over all committed inputs of tests/linear_solve_cases.py, rounded up
to a power of two.  The factor 8 covers what differs from zgesv in the kernels: complex products in four FMAs, a Newton
reciprocal instead of a division, implicit interchanges (and, in k_solve_dense_reg2, Gauss-Jordan instead of a back
substitution).  Measured on the CPU (tests/test_linear_solve.py prints them and asserts that GATE follows from the first):

    LAPACK zgesv, worst over all inputs          0.223 n u   (permuted, one unit, 5 bins: n = 6, where n u is smallest)
    fp64 model with the kernels' rule, worst     0.213 n u   (0.96 times LAPACK; as Gauss-Jordan on the dense inputs 0.058)
    the CPU oracle (explicit inverse), worst     0.388 n u
    GATE = 2^ceil(log2(8 * 0.223))               2     n u
"""
import numpy as np

LD, CLD = np.longdouble, np.clongdouble
U = 2.0 ** -53
GATE = 2.0

PIVOT_FAULTS = ("none", "second", "low16")
INDEX_FAULTS = ("rhs_swapped", "bin_off_by_one", "last_bin_cloned", "units_swapped")
FAULTS = PIVOT_FAULTS + INDEX_FAULTS


def gate_from(lapack_worst):
    """GATE as defined above, from the measured LAPACK value."""
    return 2.0 ** np.ceil(np.log2(8.0 * lapack_worst))


def _per_bin(a, nw, dtype):
    """[nSys,n,n] or [nSys,n,n,nw] -> [nSys,nw,n,n] in dtype (None: zeros are returned as None)"""
    a = np.asarray(a, dtype=dtype)
    if a.ndim == 3:
        return np.broadcast_to(a[:, None], (a.shape[0], nw) + a.shape[1:])
    return np.moveaxis(a, -1, 1)


def assemble(w, n, blocks=None, M=None, B=None, C=None, Badd=None, abs_blocks=None):
    """(A, absA) [nSys,nw,n,n] in clongdouble / longdouble.  blocks [nSys,nUnit,6,6,nw]: the units' impedances on the block
    diagonal (abs_blocks: their magnitude as a sum of addends, where the caller built them from addends; default |blocks|);
    M, B [nSys,n,n] or [nSys,n,n,nw], C, Badd [nSys,n,n]; any may be None."""
    w = np.asarray(w, dtype=LD)
    nw = len(w)
    nSys = next(np.shape(x)[0] for x in (blocks, M, B, C) if x is not None)
    A = np.zeros((nSys, nw, n, n), dtype=CLD)
    absA = np.zeros((nSys, nw, n, n), dtype=LD)
    wv = w[None, :, None, None]
    if blocks is not None:
        blocks = np.asarray(blocks, dtype=CLD)
        ab = np.abs(blocks) if abs_blocks is None else np.asarray(abs_blocks, dtype=LD)
        for u in range(blocks.shape[1]):
            A[:, :, 6 * u:6 * u + 6, 6 * u:6 * u + 6] += np.moveaxis(blocks[:, u], -1, 1)
            absA[:, :, 6 * u:6 * u + 6, 6 * u:6 * u + 6] += np.moveaxis(ab[:, u], -1, 1)
    if M is not None:
        m = _per_bin(M, nw, LD)
        A -= wv * wv * m
        absA += wv * wv * np.abs(m)
    for b in (B, Badd):
        if b is not None:
            b = _per_bin(b, nw, LD)
            A += 1j * (wv * b)
            absA += wv * np.abs(b)
    if C is not None:
        c = _per_bin(C, nw, LD)
        A += c
        absA += np.abs(c)
    return A, absA


def omega(A, absA, X, F):
    """Backward error [nSys,nw] of X, F [nSys,nRhs,n,nw] in units of n u, worst right-hand side; inf where X is not finite."""
    n = A.shape[-1]
    X = np.moveaxis(np.asarray(X), -1, 1)                                     # [nSys,nw,nRhs,n]
    F = np.moveaxis(np.asarray(F), -1, 1)
    finite = np.all(np.isfinite(X.real) & np.isfinite(X.imag), axis=(2, 3))
    Xl = np.where(finite[:, :, None, None], X, 0).astype(CLD)
    Fl = F.astype(CLD)
    res = np.abs(Fl - np.einsum("swij,swrj->swri", A, Xl)).max(axis=-1)     # [nSys,nw,nRhs]
    normA = absA.sum(axis=-1).max(axis=-1)[:, :, None]
    den = normA * np.abs(Xl).max(axis=-1) + np.abs(Fl).max(axis=-1)
    om = (res / den).max(axis=-1) / (LD(n) * LD(U))
    return np.where(finite, om, np.inf).astype(float)


def cond_inf(A):
    """kappa_inf of every (system, bin) of assemble()'s A, in complex128"""
    A = np.asarray(A, dtype=complex)
    return np.abs(A).sum(axis=-1).max(axis=-1) * np.abs(np.linalg.inv(A)).sum(axis=-1).max(axis=-1)


def lapack(A, F):
    """numpy.linalg.solve in complex128 on assemble()'s A rounded to fp64: X [nSys,nRhs,n,nw]"""
    X = np.linalg.solve(np.asarray(A, dtype=complex), np.moveaxis(np.asarray(F, dtype=complex), (1, 2, 3), (3, 2, 1)))
    return np.ascontiguousarray(np.moveaxis(X, (1, 2, 3), (3, 2, 1)))


# ------------------------------------------------------------------ the fp64 model of the elimination
def eliminate(A, F, fault="", jordan=False, trace=None):
    """One system in plain complex128: A [n,n], F [n,nRhs] -> X [n,nRhs].  Partial pivoting on |re| + |im|, first largest;
    multipliers as a product with conj(p) / |p|^2 (the kernels' reciprocal).  jordan: the rows above the pivot are
    eliminated too (k_solve_dense_reg2) instead of a back substitution.  fault: one of PIVOT_FAULTS.  trace: a list that
    receives (pivot's ORIGINAL row, its magnitude, the largest other candidate, number of candidates equal to the pivot)."""
    A = np.array(A, dtype=complex)
    F = np.array(F, dtype=complex)
    n = A.shape[0]
    rowid = np.arange(n)
    with np.errstate(all="ignore"):
        for k in range(n):
            mag = np.abs(A[k:, k].real) + np.abs(A[k:, k].imag)
            mag = np.where(mag >= 0.0, mag, 0.0)                              # NaN: comparable, as in the kernels
            key = np.lexsort((rowid[k:], -mag))                               # candidates, best first; ties to the lower row
            if fault == "none":
                j = 0                                                         # whichever row sits in place: no search at all
            elif fault == "second":
                j = int(key[1]) if len(key) > 1 else int(key[0])
            elif fault == "low16":
                low = [i for i in key if rowid[k + i] < 16]
                j = int(low[0]) if low else int(key[0])
            else:
                j = int(key[0])
            if trace is not None:
                others = np.delete(mag, j)
                trace.append((int(rowid[k + j]), float(mag[j]), float(others.max()) if others.size else 0.0,
                              int(np.sum(mag == mag[j]))))
            p = k + j
            if p != k:
                A[[k, p]] = A[[p, k]]
                F[[k, p]] = F[[p, k]]
                rowid[[k, p]] = rowid[[p, k]]
            pv = A[k, k]
            inv = np.conj(pv) / (pv.real * pv.real + pv.imag * pv.imag)
            rows = np.arange(n) != k if jordan else np.arange(n) > k
            l = A[rows, k] * inv
            A[rows, k + 1:] -= l[:, None] * A[k, k + 1:][None, :]
            F[rows] -= l[:, None] * F[k][None, :]
            A[rows, k] = 0.0 if jordan else l
            A[k, k] = inv                                                     # the reciprocal pivot
        if jordan:
            return F * np.diag(A)[:, None]
        for k in range(n - 1, -1, -1):
            F[k] = F[k] * A[k, k]
            F[:k] -= A[:k, k][:, None] * F[k][None, :]
    return F


def assemble_fp64(w, n, blocks=None, M=None, B=None, C=None, Badd=None):
    """The kernels' own assembly in fp64 (without the fused multiply-add: absA covers the difference): [nSys,nw,n,n]"""
    w = np.asarray(w, dtype=float)
    nw = len(w)
    nSys = next(np.shape(x)[0] for x in (blocks, M, B, C) if x is not None)
    A = np.zeros((nSys, nw, n, n), dtype=complex)
    wv = w[None, :, None, None]
    zero = np.zeros((nSys, n, n))
    Bsum = _per_bin(zero if B is None else B, nw, float) + (0.0 if Badd is None else _per_bin(Badd, nw, float))
    A.real = -(wv * wv) * _per_bin(zero if M is None else M, nw, float) + _per_bin(zero if C is None else C, nw, float)
    A.imag = wv * Bsum
    if blocks is not None:
        for u in range(np.shape(blocks)[1]):
            A[:, :, 6 * u:6 * u + 6, 6 * u:6 * u + 6] += np.moveaxis(np.asarray(blocks)[:, u], -1, 1)
    return A


def model(w, n, F, blocks=None, M=None, B=None, C=None, Badd=None, fault="", jordan=False):
    """The fp64 model on a whole batch: X [nSys,nRhs,n,nw].  fault: "" or one of FAULTS -- the pivot faults inside the
    elimination, the indexing faults as what a kernel with that fault would return:
      rhs_swapped      right-hand sides 0 and 1 exchanged on the way out
      bin_off_by_one   every bin holds the solution of its right neighbour (the last: of its left)
      last_bin_cloned  the last bin holds the solution of the one before it
      units_swapped    the diagonal blocks of units 0 and 1 exchanged"""
    if fault == "units_swapped":
        blocks = np.array(blocks)
        blocks[:, [0, 1]] = blocks[:, [1, 0]]
    A = assemble_fp64(w, n, blocks, M, B, C, Badd)
    F = np.asarray(F, dtype=complex)
    X = np.empty_like(F)
    for s in range(A.shape[0]):
        for i in range(A.shape[1]):
            X[s, :, :, i] = eliminate(A[s, i], F[s, :, :, i].T, fault if fault in PIVOT_FAULTS else "", jordan).T
    nw = X.shape[-1]
    if fault == "rhs_swapped":
        X[:, [0, 1]] = X[:, [1, 0]]
    elif fault == "bin_off_by_one":
        X = X[..., [i + 1 if i + 1 < nw else nw - 2 for i in range(nw)]]
    elif fault == "last_bin_cloned":
        X[..., nw - 1] = X[..., nw - 2]
    return np.ascontiguousarray(X)


def applies(fault, nUnit, nRhs, nw, n):
    """Does the fault change anything at this shape?  (units_swapped: coupled entries only, nUnit = 0 for the dense ones)"""
    return {"low16": n > 16, "rhs_swapped": nRhs >= 2, "bin_off_by_one": nw >= 2, "last_bin_cloned": nw >= 2,
            "units_swapped": nUnit >= 2}.get(fault, True)
