"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/flex_modal_reference.npz, the extended-precision reference of the eigen
analysis of units with flexible members (include/raftx_flex_modal.h).  CPU only, mpmath at 50 digits, nothing from the
reference tree; one process per case:

    python scripts/make_flex_modal_golden.py [case ...]

Never imported by the tests; they read the committed .npz.  Cases and record: tests/flex_modal_cases.py.  The exact spectrum
comes from mpmath: where M and C are exactly symmetric, eigsy of L^-1 C L^-T with M = L L^T (orthonormal vectors, also of
exactly repeated eigenvalues), x = L^-T q; otherwise eig of M^-1 C.  The vectors of a cluster (a chain of relative gaps < 1e-6)
are orthonormalised at 50 digits before they are rounded, and the basis is checked to span an invariant subspace there.
s_j and the clusters' sigma_min(Y_c^H X_c) come from float64 scipy.linalg.eig(left=True): they only scale a bound.  LAPACK's
own figures with the reference's procedure, numpy.linalg.eig(numpy.linalg.solve(M, C)), are measured here and stored: its
multiple of the eigenvalue bound per case (g is the worst, G = 4 max(1, g)) and its worst mode angle per case.
"""
import multiprocessing
import os
import sys
import time

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from raft_amd import snapshot as standin                     # noqa: E402
from tests import flex_modal_cases as fmc                    # noqa: E402

OUT = os.path.join(standin.GOLDEN_DIR, "flex_modal_reference.npz")
DIGITS = 50
SEEDS = {"synth7": 7007, "synth37": 7037, "synth65": 7065}


def inputs(name):
    if name in fmc.SYNTH:
        M, C = fmc.synthetic(fmc.SYNTH[name], SEEDS[name])
        return M, C, None
    M, C = fmc.deck_matrices(fmc.DECKS[name])
    moor6 = None
    if name == "deck150_moor":
        moor6 = fmc.deck_moor_block()
        C = C.copy()
        C[:6, :6] += moor6
    return M, C, moor6


def exact(M, C):
    """Ascending eigenvalues and right vectors (mp) of the exact M^-1 C."""
    mp.mp.dps = DIGITS
    n = len(M)
    Mm, Cm = mp.matrix(M.tolist()), mp.matrix(C.tolist())
    if np.array_equal(M, M.T) and np.array_equal(C, C.T):
        L = mp.cholesky(Mm)
        Li = mp.inverse(L)
        E, Q = mp.eigsy(Li * Cm * Li.T)
        X = Li.T * Q
        lam = [E[k] for k in range(n)]
        apply_A = lambda q: Li.T * (Li * (Cm * q))               # noqa: E731
    else:
        A = mp.inverse(Mm) * Cm
        apply_A = lambda q: A * q                                # noqa: E731
        E, X = mp.eig(A)
        # (a deck whose M is symmetric only to an ulp has exact eigenvalues that leave the real axis by a hair inside its
        # clusters: such a pair counts with its real part and must lie inside a cluster, whose real span is what is recorded)
        assert all(abs(mp.im(e)) < fmc.GAP_TOL * abs(e) for e in E), "complex eigenvalues"
        lam = [mp.re(e) for e in E]
    order = sorted(range(n), key=lambda k: lam[k])
    cols = [[X[i, k] for i in range(n)] for k in order]
    return [lam[k] for k in order], [E[k] for k in order], cols, apply_A


def orthonormal(cols, want):
    """A real orthonormal basis of the span of the (complex) vectors: Gram-Schmidt, twice, at the working precision, over
    their real and imaginary parts; a part already in the span is dropped.  Exactly ``want`` vectors must remain."""
    out = []
    parts = [[mp.re(v) for v in x] for x in cols] + [[mp.im(v) for v in x] for x in cols]
    for x in parts:
        nx = mp.sqrt(sum(v * v for v in x))
        if nx < mp.mpf(10) ** -(DIGITS // 2):
            continue
        x = [v / nx for v in x]
        keep = True
        for _ in range(2):
            for q in out:
                d = sum(a * b for a, b in zip(q, x))
                x = [a - d * b for a, b in zip(x, q)]
            nx = mp.sqrt(sum(v * v for v in x))
            if nx < mp.mpf(10) ** -(DIGITS // 2):
                keep = False
                break
            x = [v / nx for v in x]
        if keep:
            out.append(x)
    assert len(out) == want, "a cluster's vectors span %d dimensions, not %d" % (len(out), want)
    return out


def real_unit(x):
    """A separated mode: the phase turned so that the largest component is real and positive; then it must be real."""
    n = len(x)
    big = max(range(n), key=lambda i: abs(x[i]))
    ph = x[big] / abs(x[big])
    x = [v / ph for v in x]
    nx = mp.sqrt(sum(abs(v) ** 2 for v in x))
    assert all(abs(mp.im(v)) < mp.mpf(10) ** -(DIGITS - 15) * nx for v in x), "a separated mode is not real"
    return [mp.re(v) / nx for v in x]


def invariance(apply_A, basis):
    """The largest part of A q outside span(Q) over the orthonormal basis Q, relative to |A q|."""
    n = len(basis[0])
    worst = mp.mpf(0)
    for q in basis:
        y = apply_A(mp.matrix(q))
        y = [y[i] for i in range(n)]
        ny = mp.sqrt(sum(v * v for v in y))
        for b in basis:
            d = sum(a * c for a, c in zip(b, y))
            y = [a - d * c for a, c in zip(y, b)]
        worst = max(worst, mp.sqrt(sum(v * v for v in y)) / ny)
    return float(worst)


def work(name):
    t0 = time.time()
    M, C, moor6 = inputs(name)
    n = len(M)
    lam_mp, lam_c, cols, apply_A = exact(M, C)
    lam = np.array([float(v) for v in lam_mp])
    assert np.all(lam > 0), name
    clusters = fmc.chains(lam)
    vec = np.zeros((n, n))
    inv = 0.0
    inside = set()
    for cl in clusters:
        basis = orthonormal([cols[k] for k in cl], len(cl))
        inv = max(inv, invariance(apply_A, basis))
        for k, q in zip(cl, basis):
            vec[:, k] = [float(v) for v in q]
        inside.update(cl)
    for k in range(n):
        if k in inside:
            continue
        assert mp.im(lam_c[k]) == 0 or abs(mp.im(lam_c[k])) < mp.mpf(10) ** -(DIGITS - 15) * abs(lam_c[k]), "a complex eigenvalue outside the clusters"
        vec[:, k] = [float(v) for v in real_unit(cols[k])]
    # float64: s_j and the clusters' sigma_min(Y_c^H X_c)
    s = fmc.float64_conditions(fmc.refined_A(M, C).astype(np.float64), clusters)
    rec = dict(name=name, lam=lam, vec=vec, s=s, clusters=[np.array(cl) for cl in clusters], cluster_invariance=inv,
               seconds=time.time() - t0)
    if name in fmc.SYNTH:
        rec["M"], rec["C"] = M, C
    if moor6 is not None:
        rec["moor6"] = moor6
    return rec


def lapack_figures(rec):
    """LAPACK with the reference's procedure on the case: its multiple of the eigenvalue bound and its worst mode angle."""
    name = rec["name"]
    M, C = fmc.matrices(name)
    lam_np, vec_np = np.linalg.eig(np.linalg.solve(M, C))
    assert np.all(np.isreal(lam_np)), name
    o = np.argsort(lam_np.real, kind="stable")
    lam_np, vec_np = lam_np.real[o], vec_np.real[:, o]
    mult = float(np.max(np.abs(lam_np - rec["lam"]) / fmc.lambda_bound(name)))
    angle = fmc.mode_angle(vec_np, rec["lam"], rec["vec"])
    res = float(np.max(fmc.residual_multiples(name, lam_np, vec_np)))
    return mult, angle, res


def main():
    names = sys.argv[1:] or list(fmc.CASES)
    with multiprocessing.Pool(min(len(names), os.cpu_count() or 1)) as pool:
        recs = pool.map(work, names, chunksize=1)
    # the gates read the golden through tests/flex_modal_cases.py: write it first without LAPACK's figures, then with them
    standin.save_fixture(OUT, {"config": "", "digits": DIGITS, "g": 0.0, "G": 4.0, "cases": recs})
    fmc.golden.cache_clear()
    g = 0.0
    for rec in recs:
        rec["lapack_multiple"], rec["lapack_angle"], rec["lapack_residual"] = lapack_figures(rec)
        g = max(g, rec["lapack_multiple"])
        n = len(rec["lam"])
        print("%-13s n %3d  fn %.5f .. %.3f Hz  clusters %2d (%3d eigenvalues, invariance %.1e)  s_min %.3f  LAPACK: multiple %.3f  "
              "residual multiple %.3f  angle %.2e  (%.0f s)"
              % (rec["name"], n, np.sqrt(rec["lam"][0]) / 2 / np.pi, np.sqrt(rec["lam"][-1]) / 2 / np.pi, len(rec["clusters"]),
                 sum(len(c) for c in rec["clusters"]), rec["cluster_invariance"], rec["s"].min(), rec["lapack_multiple"],
                 rec["lapack_residual"], rec["lapack_angle"], rec["seconds"]), flush=True)
    G = 4.0 * max(1.0, g)
    print("g = %.3f  G = %.3f" % (g, G))
    cfg = ("mpmath at %d digits: eigsy of L^-1 C L^-T (M, C exactly symmetric) or eig of M^-1 C; s and the clusters' sigma_min from "
           "float64 scipy.linalg.eig(left=True); LAPACK = numpy.linalg.eig(numpy.linalg.solve(M, C))" % DIGITS)
    standin.save_fixture(OUT, {"config": cfg, "digits": DIGITS, "g": float(g), "G": float(G), "cases": recs})
    fmc.golden.cache_clear()
    print("wrote %s (%d cases, %d bytes)" % (OUT, len(recs), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
