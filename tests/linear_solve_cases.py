"""Seeded, tiny inputs for the linear solvers: four families of matrices that the coupled (raftx_solve_system) and the dense
(raftx_solve_dense_batch) entries share, and the shapes -- each on a selection edge of the code -- at which they run.

  dominant   Zblk = N(0,1) + i N(0,1) + 8 I with symmetric coupling of order 1 (test_solve_system_parity's inputs, the
             coupling divided by sqrt(nUnit): its NORM stays of order 1 up to 16 units, where unscaled entries of order 1
             outweigh the 8 I and cond_inf passes 1e4 from 7 units on).  The largest entry of a column is on the diagonal or
             as good as it.  The baseline: a wrong pivot search still passes here.
  permuted   a well-conditioned dense matrix, 10 I + N(0,1), with its rows rolled by n // 3, carried by Cc (C); unit blocks,
             Mc and Bc of order 0.05.  Every pivot is off the diagonal, the other entries are not negligible.
  forced     one entry of magnitude 1 .. 10 per column in Cc AND in Bc (same permutation, random signs); everything else --
             Zblk and Mc included -- is dust, uniform in +-1e-7.  The elimination has exactly one acceptable pivot per step.
             System 0: the reversal; system 1: column j's entry in row (j - 1) / 2 for odd j and n / 2 + j / 2 for even j
             (the inverse of "odd rows first, then even": consecutive pivots alternate between the lower and the upper rows,
             across 16-lane rows and unit boundaries); system 2: a random permutation.
  ties       every non-zero entry has |re| + |im| = 1 at w = 1: unit blocks from {+-1, +-i, (+-1 +- i) / 2}, coupling entries
             (outside the unit blocks) from {-1, 0, 1}, each carried by ONE of Cc, Mc, Bc.  The frequencies are powers of
             two, so the assembly is exact and the other bins hold the magnitudes 1, w, w^2: every pivot search meets exact
             ties (tie rule, truncated keys).  Another winner is as valid: the criterion is backward error, not bits.

The dense entries take the same matrices without unit blocks (the ties family draws every entry, diagonal blocks included,
from the coupling's values and the unit blocks' values through C and B).  tests/test_linear_solve.py asserts what the
families promise (conditioning, unique pivots, pivots on both sides of row 16, exact ties)."""
import numpy as np

FAMILIES = ("dominant", "permuted", "forced", "ties")
N_SYS = 3
DUST = 1e-7

# ------------------------------------------------------------------ shapes
# register-resident rows kernel: every instantiation NU x NR (nRhs = 3 is padded to 4); nw 1, 2, 3, 5: a dead half-wave,
# a full pair, a cloned last bin
ROWS_SHAPES = [(nu, nr) for nu in (2, 3, 4, 5) for nr in (1, 2, 3, 4)]
ROWS_NW = (1, 2, 3, 5)
# LDS-resident solver: (nUnit, nRhs) -> the nw it runs with.  Bins per workgroup and dynamic LDS of solve_system_shape
# (16 n (n + nRhs) bytes per bin; 4 bins up to 16 KiB per bin, 2 up to 32 KiB, else 1):
LDS_SHAPES = {(1, 1): (1, 2, 3, 5),     # 4 bins, 2.6 KiB
              (4, 5): (1, 2, 3, 5),     # 4 bins, 43.5 KiB: nRhs > 4 leaves the rows kernel
              (5, 5): (1, 3),           # 2 bins, 32.8 KiB: n (n + r) = 1050 > 1024
              (6, 1): (1, 3),           # 2 bins, 41.6 KiB
              (7, 7): (2,),             # 1 bin, 32.2 KiB: 2058 > 2048
              (10, 3): (2,),            # 1 bin, 59.1 KiB
              (11, 1): (2,),            # 1 bin, 69.1 KiB: the first shape over 64 KiB (hipFuncSetAttribute)
              (16, 4): (2,)}            # 1 bin, exactly 150 KiB: the largest shape the entry accepts
REFUSED_SHAPES = [(17, 1), (16, 5)]
COUPLED_SHAPES = [(nu, nr, ROWS_NW) for nu, nr in ROWS_SHAPES] + [(nu, nr, nws) for (nu, nr), nws in LDS_SHAPES.items()]

# dense: n + nRhs on both sides of every instantiation edge of k_solve_dense_reg2 (32, 64, 96, 128, 160)
DENSE_FAMILIES = ("forced", "ties", "permuted")
DENSE_NSYS, DENSE_NW = 2, 3
DENSE_SHAPES = [(31, 1), (31, 2), (62, 2), (62, 3), (95, 1), (96, 1), (125, 3), (126, 3), (158, 2), (159, 2)]
DENSE_L2_SHAPE = (170, 1)               # n + nRhs > 160: k_solve_dense, run with a frequency-dependent M
DENSE_RESIDENT_SHAPE = (40, 2)          # (n, nRhs) of the raftx_dense_resident case: 2 sets x 2 systems each, with Badd


def lds_bytes(nUnit, nRhs):
    """(bins per workgroup, dynamic LDS in bytes) of k_solve_system, as solve_system_shape gives them"""
    per = 16 * 6 * nUnit * (6 * nUnit + nRhs)
    nbin = 4 if per * 4 <= 65536 else (2 if per * 2 <= 65536 else 1)
    return nbin, per * nbin


def axis(family, nw):
    """Distinct frequencies: neighbouring bins differ by O(1) of the entries.  ties: powers of two, 1 first (exact)."""
    if family == "ties":
        return np.array([1.0, 2.0, 0.5, 4.0, 0.25, 8.0, 0.125, 16.0][:nw])
    return np.linspace(0.4, 1.5, nw) if nw > 1 else np.array([0.9])


def forced_rows(rng, s, n):
    """row[j]: the row of column j's entry, for system s"""
    j = np.arange(n)
    if s == 0:
        return n - 1 - j
    if s == 1:
        return np.where(j % 2 == 1, (j - 1) // 2, n // 2 + j // 2)
    return rng.permutation(n)


def _dust(rng, shape):
    return rng.uniform(-DUST, DUST, size=shape)


TIE_VALUES = np.array([1, -1, 1j, -1j, 0.5 + 0.5j, 0.5 - 0.5j, -0.5 + 0.5j, -0.5 - 0.5j])


def matrices(family, rng, nSys, n, unit_blocks):
    """(M, B, C) [nSys,n,n] of a family.  unit_blocks: the 6 x 6 diagonal blocks are left to Zblk (coupled entries)."""
    if family == "dominant":
        C = rng.normal(size=(nSys, n, n))
        C = (C + np.transpose(C, (0, 2, 1))) / np.sqrt(n / 6.0)
        if not unit_blocks:
            C += 8.0 * np.eye(n)
        return 0.1 * rng.normal(size=(nSys, n, n)), 0.1 * rng.normal(size=(nSys, n, n)), C
    if family == "permuted":
        C = np.roll(10.0 * np.eye(n)[None] + rng.normal(size=(nSys, n, n)), n // 3, axis=1)
        return 0.05 * rng.normal(size=(nSys, n, n)), 0.05 * rng.normal(size=(nSys, n, n)), C
    if family == "forced":
        M, B, C = _dust(rng, (nSys, n, n)), _dust(rng, (nSys, n, n)), _dust(rng, (nSys, n, n))
        for s in range(nSys):
            rows, cols = forced_rows(rng, s, n), np.arange(n)
            C[s, rows, cols] = rng.uniform(1.0, 10.0, size=n) * rng.choice([-1.0, 1.0], size=n)
            B[s, rows, cols] = rng.uniform(1.0, 10.0, size=n) * rng.choice([-1.0, 1.0], size=n)
        return M, B, C
    # ties: each entry carried by one of C, M, B (value in {-1, 0, 1}); the dense entries also draw the unit blocks' values
    val = rng.choice([-1.0, 0.0, 1.0], size=(nSys, n, n))
    which = rng.integers(0, 3, size=(nSys, n, n))
    C, M, B = val * (which == 0), -val * (which == 1), val * (which == 2)
    blk = np.kron(np.eye(n // 6 + 1), np.ones((6, 6)))[:n, :n].astype(bool)
    if unit_blocks:
        C[:, blk] = M[:, blk] = B[:, blk] = 0.0
    else:
        z = rng.choice(TIE_VALUES, size=(nSys, n, n))
        C[:, blk], B[:, blk], M[:, blk] = z.real[:, blk], z.imag[:, blk], 0.0
    return M, B, C


def unit_blocks(family, rng, nSys, nUnit, nw):
    shape = (nSys, nUnit, 6, 6, nw)
    if family == "dominant":
        return rng.normal(size=shape) + 1j * rng.normal(size=shape) + 8.0 * np.eye(6)[None, None, :, :, None]
    if family == "permuted":
        return 0.05 * (rng.normal(size=shape) + 1j * rng.normal(size=shape))
    if family == "forced":
        return _dust(rng, shape) + 1j * _dust(rng, shape)
    return np.repeat(rng.choice(TIE_VALUES, size=shape[:-1])[..., None], nw, axis=-1)


def _rhs(rng, nSys, nRhs, n, nw):
    return rng.normal(size=(nSys, nRhs, n, nw)) + 1j * rng.normal(size=(nSys, nRhs, n, nw))


COND_DRAW = 8e3                         # a draw is kept if cond_inf <= this in every (system, bin): the tests assert 1e4


def _worst_cond(w, n, M, B, C, Zblk=None):
    worst = 0.0
    for i, wi in enumerate(w):
        A = -wi * wi * (M[..., i] if M.ndim == 4 else M) + 1j * wi * B + C
        if Zblk is not None:
            for u in range(Zblk.shape[1]):
                A[:, 6 * u:6 * u + 6, 6 * u:6 * u + 6] += Zblk[:, u, :, :, i]
        norm = lambda a: np.abs(a).sum(axis=-1).max(axis=-1)
        worst = max(worst, float((norm(A) * norm(np.linalg.inv(A))).max()))
    return worst


def coupled(family, nUnit, nRhs, nw, nSys=N_SYS):
    """dict w, Zblk, F, Mc, Bc, Cc of raftx_solve_system.  Random matrices of entries +-1 are now and then nearly singular:
    the first draw (salt 0, 1, ..) that is conditioned within COND_DRAW is the input."""
    n, w = 6 * nUnit, axis(family, nw)
    for salt in range(100):
        rng = np.random.default_rng([FAMILIES.index(family), nUnit, nRhs, nw, salt])
        Mc, Bc, Cc = matrices(family, rng, nSys, n, True)
        Zblk = unit_blocks(family, rng, nSys, nUnit, nw)
        if _worst_cond(w, n, Mc, Bc, Cc, Zblk) <= COND_DRAW:
            return dict(w=w, Zblk=Zblk, F=_rhs(rng, nSys, nRhs, n, nw), Mc=Mc, Bc=Bc, Cc=Cc)
    raise AssertionError("no well-conditioned draw")


def dense(family, n, nRhs, nw=DENSE_NW, nSys=DENSE_NSYS, freq_M=False):
    """dict w, M, B, C, F of raftx_solve_dense_batch (draws as in coupled).  freq_M: M [nSys,n,n,nw] -- the family's M in
    bin 0; in bin i fresh draws of its size (ties: M's rows rolled by i, the entries stay in {-1, 0, 1})."""
    w = axis(family, nw)
    for salt in range(100):
        rng = np.random.default_rng([100 + FAMILIES.index(family), n, nRhs, nw, salt])
        M, B, C = matrices(family, rng, nSys, n, False)
        if freq_M and family == "ties":
            M = np.stack([np.roll(M, i, axis=1) for i in range(nw)], axis=-1)
        elif freq_M:
            scale = {"forced": DUST, "permuted": 0.05, "dominant": 0.1}[family]
            M = np.stack([M] + [scale * rng.uniform(-1.0, 1.0, size=M.shape) for _ in range(nw - 1)], axis=-1)
        if _worst_cond(w, n, M, B, C) <= COND_DRAW:
            return dict(w=w, M=M, B=B, C=C, F=_rhs(rng, nSys, nRhs, n, nw))
    raise AssertionError("no well-conditioned draw")


def dense_resident():
    """The raftx_dense_resident case: forced matrices of 2 sets, 2 systems per set; the large damping entries travel in
    Badd [4,n,n] (different per system of a set), B itself is dust.  dict w, M, B, C [2,..], Badd [4,n,n], F [4,..]."""
    n, nRhs = DENSE_RESIDENT_SHAPE
    rng = np.random.default_rng([200, n, nRhs])
    M, B, C = matrices("forced", rng, 2, n, False)
    Badd = np.repeat(B, 2, axis=0)
    big = np.abs(Badd) > 0.5
    Badd[1::2][big[1::2]] *= -0.5                          # the second system of each set: other entries, same pattern
    Badd[~big] = _dust(rng, Badd.shape)[~big]
    return dict(w=axis("forced", DENSE_NW), M=M, B=_dust(rng, B.shape), C=C, Badd=Badd, F=_rhs(rng, 4, nRhs, n, DENSE_NW))


def forced_coupling(rng, nGroup, n, scale):
    """Coupling of the forced kind for the resident coupled solve: entries `scale` times 1 .. 10, dust `scale` * 1e-7"""
    M, B, C = matrices("forced", rng, nGroup, n, True)
    return scale * M, scale * B, scale * C
