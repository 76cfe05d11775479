"""fp64 NumPy restatement of k_mean_pose (raft_amd/csrc/raftx_statics.h): the same expressions in the same order, one
design at a time, on the line records of tests/mooring_device_model.py (``line``).  It is what the gate's constant of
tests/mean_pose_reference.py is measured with on the CPU, and -- through ``seed`` -- the carrier of the deliberate errors
the gate must reject or tolerate (tests/test_mean_pose.py).  The kernel contracts multiply-adds and uses the device's
library functions, so the model agrees with it to rounding, not to the bit.
"""
import numpy as np

from . import mooring_device_model as dm

CAPS = (30.0, 30.0, 5.0, 0.1, 0.1, 0.1)
TOL = (1e-9, 1e-10)
MAX_ITER = 40
FLAG_POSE_CAP, FLAG_SINGULAR = 16, 32
SEEDS = ("no_fr", "khs_sign", "no_xref")


def moor(lines_d, x, depth, seed=None):
    """(flag, C [6,6], F [6], T [2 nL], J [2 nL,6]) of one design at x: k_moor_design's sums in line order."""
    nL = len(lines_d)
    recs = [dm.line(lines_d[l], x, depth) for l in range(nL)]
    flag = 0
    for fl, _ in recs:
        flag |= fl
    C, F, Tn, J = np.zeros((6, 6)), np.zeros(6), np.zeros(2 * nL), np.zeros((2 * nL, 6))
    if flag:
        return flag, C, F, Tn, J
    for l, (_, q) in enumerate(recs):
        f, r, K = q["f"], q["r"], q["K"]
        RX, FX = dm._skew(r), dm._skew(f)
        KR, RK = K @ RX, RX @ K
        C[:3, :3] += K
        C[:3, 3:] += -KR
        C[3:, :3] += RK
        C[3:, 3:] += -(RX @ KR) if seed == "no_fr" else (-(RX @ KR) - FX @ RX)
        F[:3] += f
        F[3:] += np.array([r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]])
        Tn[l], Tn[nL + l] = q["TA"], q["TB"]
        for e, g in ((0, q["gA"]), (1, q["gB"])):
            J[e * nL + l, :3] = g
            J[e * nL + l, 3:] = [r[1] * g[2] - r[2] * g[1], r[2] * g[0] - r[0] * g[2], r[0] * g[1] - r[1] * g[0]]
    return 0, C, F, Tn, J


def lu_solve(K, Y):
    """(dX, singular): Gaussian elimination of [K | Y] with partial pivoting, the first row of the largest |a| as pivot."""
    A = np.concatenate([np.array(K, dtype=np.float64), np.asarray(Y, dtype=np.float64)[:, None]], axis=1)
    sing = False
    for k in range(6):
        p, best = k, abs(A[k, k])
        for i in range(k + 1, 6):
            if abs(A[i, k]) > best:
                p, best = i, abs(A[i, k])
        if p != k:
            A[[k, p]] = A[[p, k]]
        if not (best > 0.0) or not np.isfinite(best):
            sing = True
        with np.errstate(all="ignore"):
            for i in range(k + 1, 6):
                m = A[i, k] / A[k, k]
                for j in range(k + 1, 7):
                    A[i, j] = A[i, j] - m * A[k, j]
    x = np.zeros(6)
    with np.errstate(all="ignore"):
        for i in range(5, -1, -1):
            s = A[i, 6]
            for j in range(i + 1, 6):
                s = s - A[i, j] * x[j]
            x[i] = s / A[i, i]
    return x, sing or not np.all(np.isfinite(x))


def residual(K_hs, F0, F_env, x, x_ref, Fm, seed=None):
    Y = np.zeros(6)
    xr = np.zeros(6) if seed == "no_xref" else x_ref
    for i in range(6):
        acc = 0.0
        for j in range(6):
            acc = acc + K_hs[i, j] * (x[j] - xr[j])
        base = F0[i] + F_env[i]
        Y[i] = ((base + acc) if seed == "khs_sign" else (base - acc)) + Fm[i]
    return Y


def step(K, Y, log=None):
    """(dX, singular) of one iteration: the repaired diagonal, the solve, the diagonal growth while dX.Y < 0, the caps."""
    K = np.array(K, dtype=np.float64)
    kmean = 0.0
    for i in range(6):
        kmean = kmean + K[i, i]
    kmean = kmean / 6.0
    for i in range(6):
        if K[i, i] == 0.0:
            K[i, i] = kmean
            if log is not None:
                log.append(("zero_diagonal", i))
    dX, sing = lu_solve(K, Y)
    for _ in range(10):
        if sing or not (float(np.dot(dX, Y)) < 0.0):
            break
        for i in range(6):
            K[i, i] = K[i, i] + 0.1 * abs(K[i, i])
        if log is not None:
            log.append(("enlarged", None))
        dX, sing = lu_solve(K, Y)
    if sing:
        return dX, True
    s = 1.0
    for i in range(6):
        if abs(dX[i]) * s > CAPS[i]:
            s = CAPS[i] / abs(dX[i])
    if s < 1.0 and log is not None:
        log.append(("capped", s))
    return dX * s, False


def solve(lines_d, depth, K_hs, F0, F_env=None, x_ref=None, tol=None, max_iter=0, seed=None, log=None):
    """dict pose, C, F, T, J, F_res, iterations, flags as raftx_mean_pose gives them for ONE design."""
    assert seed is None or seed in SEEDS
    lines_d = np.asarray(lines_d, dtype=np.float64)
    nL = len(lines_d)
    K_hs, F0 = np.asarray(K_hs, dtype=np.float64), np.asarray(F0, dtype=np.float64)
    F_env = np.zeros(6) if F_env is None else np.asarray(F_env, dtype=np.float64)
    x_ref = np.zeros(6) if x_ref is None else np.asarray(x_ref, dtype=np.float64)
    tol = TOL if tol is None else tol
    max_iter = MAX_ITER if max_iter <= 0 else max_iter
    x, it, flag, final = x_ref.copy(), 0, 0, False
    nan = dict(pose=np.full(6, np.nan), C=np.full((6, 6), np.nan), F=np.full(6, np.nan), T=np.full(2 * nL, np.nan),
               J=np.full((2 * nL, 6), np.nan), F_res=np.full(6, np.nan))
    while True:
        fl, C, Fm, Tn, J = moor(lines_d, x, depth, seed)
        if fl:
            flag |= fl
            break
        Y = residual(K_hs, F0, F_env, x, x_ref, Fm, seed)
        if final:
            return dict(pose=x, C=C, F=Fm, T=Tn, J=J, F_res=Y, iterations=it, flags=0)
        dX, sing = step(K_hs + C, Y, log)
        if sing:
            flag |= FLAG_SINGULAR
            break
        conv = all(abs(dX[i]) <= tol[0 if i < 3 else 1] for i in range(6))
        x = x + dX
        it += 1
        if conv:
            final = True
        elif it >= max_iter:
            flag |= FLAG_POSE_CAP
            break
    nan.update(iterations=it, flags=flag)
    return nan
