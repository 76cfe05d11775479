"""What the tests of the array eigen analysis share (tests/test_array_modal.py on the CPU, tests/test_hip_array_modal.py on the
GPU): the committed extended-precision reference tests/golden/array_modal_reference.npz (scripts/make_array_modal_golden.py),
the eigenvalue gate, the two mode measures and the DOF claim.

Eigenvalue gate, per eigenvalue j of a case with n DOFs:

    |lambda - lambda_ref| <= G n eps ||A_b||_F / s_j

A = M^-1 C from the golden, A_b its balanced form (scipy.linalg.matrix_balance), s_j = |y_j^H x_j| / (|y_j| |x_j|) from the
golden's exact vectors: the first-order perturbation bound of a backward-stable eigensolver on the balanced matrix.
G = 4 max(1, g), where g is the worst multiple of that bound that LAPACK itself reaches over the committed cases with the
reference's own procedure, numpy.linalg.eig(numpy.linalg.solve(M, C)); the factor 4 allows for a second backward-stable QR
(EISPACK's ordering against LAPACK's, with its own constants) and for the LU of M ahead of it.  Measured when the golden was
written: g = 0.516 (pair_thrust), so G = 4; LAPACK's own mode measures there are <= 3.4e-16 and <= 1.5e-8 (twins).  fn = sqrt(lambda) / 2 pi is held to half the relative lambda gate plus 2 eps.

Modes, the measures and numbers of check_modes of tests/test_hip_modal.py for n DOFs: where the relative gap to every other
eigenvalue is >= 1e-6, 1 - |<v, v_ref>| <= 1e-9; otherwise the largest principal angle between the clusters' spans <= 1e-7.
"""
import functools

import numpy as np

from raft_amd import snapshot as standin

EPS = 2.0 ** -52
FIRM = ("single_unit", "pair", "pair_thrust", "pair_yaw_pitch", "row3", "uncoupled_pair")   # their DOF claim is decided by >= 1e-3
LOOSE = ("square4", "ring6", "twins")                                                       # near-degenerate: spectra and subspaces only
FIRM_MARGIN = 1e-3


@functools.lru_cache(maxsize=None)
def golden():
    fx = standin.load_fixture("array_modal_reference.npz")
    return dict(g=float(fx["g"]), G=float(fx["G"]), cases={str(c["name"]): c for c in fx["cases"]})


def lambda_bound(rec):
    """n eps ||A_b||_F / s_j [n], for the ascending eigenvalues of the record."""
    from scipy.linalg import matrix_balance
    A = np.asarray(rec["A"])
    Ab, _ = matrix_balance(A)
    return len(A) * EPS * np.linalg.norm(Ab, "fro") / np.asarray(rec["s"])


def lambda_multiples(lam_sorted, rec):
    """|lambda - lambda_ref| over the bound, per eigenvalue (both ascending)."""
    return np.abs(np.asarray(lam_sorted) - np.asarray(rec["lam"])) / lambda_bound(rec)


def fn_ref(rec):
    return np.sqrt(np.asarray(rec["lam"])) / 2.0 / np.pi


def fn_gate(rec, G):
    """The relative gate of fn per ascending eigenvalue: half the relative lambda gate plus 2 eps."""
    return 0.5 * G * lambda_bound(rec) / np.asarray(rec["lam"]) + 2.0 * EPS


def mode_measures(vec_sorted, rec, gap_tol=1e-6):
    """(largest 1 - |<v, v_ref>| over the separated modes, largest principal angle over the clusters); columns ascending."""
    lam, ref = np.asarray(rec["lam"]), np.asarray(rec["vec"])
    n = len(lam)
    worst, angle = 0.0, 0.0
    for j in range(n):
        others = np.delete(np.arange(n), j)
        gap = np.min(np.abs(lam[others] - lam[j])) / abs(lam[j])
        if gap >= gap_tol:
            worst = max(worst, 1.0 - abs(float(np.dot(vec_sorted[:, j], ref[:, j]))))
        else:
            cl = [k for k in range(n) if abs(lam[k] - lam[j]) / abs(lam[j]) < gap_tol]
            qa, _ = np.linalg.qr(vec_sorted[:, cl])
            qb, _ = np.linalg.qr(ref[:, cl])
            sv = np.linalg.svd(qa.T @ qb, compute_uv=False)
            angle = max(angle, float(np.arccos(np.clip(sv.min(), -1, 1))))
    return worst, angle


def claim(vec):
    """The reference's DOF order on the columns of vec (raft_model.py:500-517): rows n-1 .. 0 each claim the unclaimed column
    of largest |v|, first on ties.  Returns (columns per DOF [n], the smallest relative lead of a winner over its runner-up)."""
    n = len(vec)
    taken, cols, margin = set(), [0] * n, np.inf
    for i in range(n - 1, -1, -1):
        free = [j for j in range(n) if j not in taken]
        a = np.abs(vec[i, free])
        k = int(np.argmax(a))
        if len(free) > 1:
            margin = min(margin, float((a[k] - np.max(np.delete(a, k))) / a[k]))
        taken.add(free[k])
        cols[i] = free[k]
    return cols, margin


def claim_margin(vec):
    return claim(vec)[1]


def check_system(name, fn, modes, rec, G, firm):
    """One device (or serial-core) result against the golden: the fn gate on the sorted spectrum, unit columns with the sign
    convention, the two mode measures, and for a firm case the column order itself.  Returns the figures for printing."""
    n = len(rec["lam"])
    fn, modes = np.asarray(fn), np.asarray(modes)
    assert np.all(np.isfinite(fn)) and np.all(np.isfinite(modes)), name
    order = np.argsort(fn, kind="stable")
    rel = np.abs(fn[order] - fn_ref(rec)) / fn_ref(rec)
    mult = lambda_multiples((2.0 * np.pi * fn[order]) ** 2, rec)
    for j in range(n):
        assert modes[int(np.argmax(np.abs(modes[:, j]))), j] > 0, (name, j)
        assert abs(np.linalg.norm(modes[:, j]) - 1.0) < 1e-12, (name, j)
    worst, angle = mode_measures(modes[:, order], rec)
    figures = dict(name=name, fn_rel=float(rel.max()), fn_gate_used=float(np.max(rel / fn_gate(rec, G))), lam_multiple=float(mult.max()),
                   mode=worst, angle=angle)
    print("%-15s n %2d  |dfn|/fn %.2e (%.3f of its gate)  lambda multiple %.3f of G = %.2f  1-|<v,v>| %.2e  angle %.2e"
          % (name, n, figures["fn_rel"], figures["fn_gate_used"], figures["lam_multiple"], G, worst, angle))
    assert np.all(rel <= fn_gate(rec, G)), (name, figures)
    assert worst <= 1e-9 and angle <= 1e-7, (name, figures)
    if firm:
        cols, margin = claim(np.asarray(rec["vec"]))
        assert margin >= FIRM_MARGIN, (name, margin)
        want = fn_ref(rec)[cols]
        assert np.all(np.abs(fn - want) / want <= fn_gate(rec, G)[cols]), (name, "column order")
        for i in range(n):
            assert 1.0 - abs(float(np.dot(modes[:, i], np.asarray(rec["vec"])[:, cols[i]]))) <= 1e-9, (name, i)
    return figures


def flag_seeds(M, C, unit):
    """Flagged variants of one system, each seeded in the block of ``unit``: name -> (M, C).  skew: a skew-dominated C
    (COMPLEX); indefinite: a negative heave stiffness (NONPOSITIVE, and SMALL_DIAG with it); small: a heave stiffness of 0.5
    uncoupled from the rest, still a well-posed problem (SMALL_DIAG alone, finite results); singular: a zero row and column
    of M (SINGULAR_M)."""
    M, C = np.asarray(M, dtype=float), np.asarray(C, dtype=float)
    o = 6 * unit
    out = {}
    Cs = C.copy()
    Cs[o + 0, o + 4] += 1e9
    Cs[o + 4, o + 0] -= 1e9
    Cs[o + 1, o + 3] += 1e9
    Cs[o + 3, o + 1] -= 1e9
    out["skew"] = (M, Cs)
    Ci = C.copy()
    Ci[o + 2, o + 2] = -abs(Ci[o + 2, o + 2])
    out["indefinite"] = (M, Ci)
    Cd, Md = C.copy(), M.copy()
    Cd[o + 2, :] = 0.0
    Cd[:, o + 2] = 0.0
    Cd[o + 2, o + 2] = 0.5
    d = Md[o + 2, o + 2]
    Md[o + 2, :] = 0.0
    Md[:, o + 2] = 0.0
    Md[o + 2, o + 2] = d
    out["small"] = (Md, Cd)
    Ms = M.copy()
    Ms[o + 5, :] = 0.0
    Ms[:, o + 5] = 0.0
    out["singular"] = (Ms, C)
    return out


def check_flag_seeds(flags, fn, modes, names):
    """The flags and the NaN rule of the seeded systems ``names`` (results in that order)."""
    from raft_amd._abi import MODAL_COMPLEX, MODAL_NONPOSITIVE, MODAL_SINGULAR_M, MODAL_SMALL_DIAG
    want = dict(skew=MODAL_COMPLEX, indefinite=MODAL_NONPOSITIVE, singular=MODAL_SINGULAR_M)
    for k, name in enumerate(names):
        if name == "small":
            assert flags[k] == MODAL_SMALL_DIAG, (name, flags[k])
            assert np.all(np.isfinite(fn[k])) and np.all(np.isfinite(modes[k])) and np.all(fn[k] > 0), name
        else:
            assert flags[k] & want[name], (name, flags[k])
            assert np.all(np.isnan(fn[k])) and np.all(np.isnan(modes[k])), name
