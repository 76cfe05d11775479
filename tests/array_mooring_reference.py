"""Independent evaluation of the array mooring system of include/raftx_array_mooring.h in ``numpy.longdouble``: the reference
of tests/test_array_mooring.py and tests/test_hip_array_mooring.py.

Rows are the records of tests/mooring_reference.py with the unit of end B in field 11 and, in field 12, 0 (an anchored row)
or 1 + the unit that carries end A (a shared row).  Anchored rows are single lines: their solve, terms and envelopes are
``mooring_reference.line_state`` / ``line_terms`` at the pose of their unit (composite lines and bridles inside an array are
held to the bits of raftx_mooring_lines by the GPU tests instead).  A shared row is one suspended catenary solved by
``mooring_reference.solve_line`` for (HF, VF) at end B with XF the horizontal distance from end A to end B and ZF = z_B - z_A
of either sign; VA = VF - wL.  With u the horizontal direction from A to B and K3, gA, gB of ``line_terms``:

    f_B = (-HF u, -VF) at r_B        f_A = (+HF u, +VA) at r_A
    C[ii] = [[K3, -K3 [r_i x]], [[r_i x] K3, -[r_i x] K3 [r_i x] - [f_i x][r_i x]]]          i in (A, B)
    C[ij] = -[[K3, -K3 [r_j x]], [[r_i x] K3, -[r_i x] K3 [r_j x]]]                           i != j
    J_B = (g, r_B x g)               J_A = (-g, -(r_A x g))            for both end tensions

Own assembly over the 6 nUnit DOFs and envelopes E = sum over the rows of (1 + kappa_row) E_row, E_row the same sums of
products with every addend replaced by its magnitude, widened for the rounding of the span at global coordinates
(``_with_span_rounding``).  kappa of a shared row is the 2-norm condition number of its catenary
Jacobian d(X, Z)/d(HF, VF) with the columns scaled by (HF, max(|VF|, |VA|)) and the rows by (XF, E_Z), E_Z the sum of the
magnitudes of the addends of Z -- ZF itself may be 0, so it cannot be the scale (for an anchored row E_Z >= ZF: the shared
row's kappa is the smaller notion, the tighter gate).

``fd_check`` holds C and J to central differences of this file's own force function over all 6 nUnit DOFs; the
frozen-partner identity (tests/test_array_mooring.py) ties a shared row to the pinned single-line path.  ``solve`` is the 6 nUnit
version of ``mean_pose_reference.solve``: plain Newton, no safeguards, the root and the bound |K^-1| E_F.
"""
import numpy as np

from . import mooring_reference as mr

EPS = mr.EPS
ML_UNIT_B, ML_UNIT_A = 11, 12
FLAG_GROUNDED = 64

# Worst multiples of the fp64 model of the device algorithm (tests/array_mooring_device_model.py) over the cases of
# tests/array_mooring_cases.py, measured on the CPU (tests/test_array_mooring.py prints them):
#   C / F / T / J, entries of eps E at the reference poses and at the model's solved poses: GATE_WORST_CPU (J of square4 at x_ref)
#   the pose, components of eps |K^-1| E_F:                                                 POSE_WORST_CPU (pair_thrust)
# The gates are the powers of two at or above 4 x those (the rule of tests/mooring_reference.py).
GATE_WORST_CPU = 1.18
GATE_C = 8
POSE_WORST_CPU = 0.082
GATE_POSE = 0.5


def units_of(rec):
    """(unit B, unit A or -1) of a row."""
    return int(rec[ML_UNIT_B]), int(rec[ML_UNIT_A]) - 1


def shared_flag(rec, poseA, poseB, depth):
    """The flag of a shared row from its geometry (fp64), or 0."""
    rec = np.asarray(rec, dtype=np.float64)
    if not (np.all(np.isfinite(rec[:10])) and np.all(np.isfinite(poseA)) and np.all(np.isfinite(poseB))):
        return mr.FLAG_BAD_LINE
    L, EA, w = rec[6], rec[7], rec[8]
    if not (L > 0 and EA > 0 and w > 0):
        return mr.FLAG_BAD_LINE
    pA = np.asarray(poseA[:3], dtype=np.float64) + np.asarray(mr.rotation(poseA[3:], np.float64) @ rec[0:3])
    pB = np.asarray(poseB[:3], dtype=np.float64) + np.asarray(mr.rotation(poseB[3:], np.float64) @ rec[3:6])
    XF = np.hypot(pB[0] - pA[0], pB[1] - pA[1])
    if XF <= 1e-9 * L:
        return mr.FLAG_VERTICAL
    return 0                              # (no SLACK: a suspended line has a catenary for every L above its chord)


def _state_from_ends(pA, pB, L, EA, w, T):
    dx, dy = pB[0] - pA[0], pB[1] - pA[1]
    XF = np.sqrt(dx * dx + dy * dy)
    ZF = pB[2] - pA[2]
    HF, VF, A, br, it, conv = mr.solve_line(XF, ZF, L, EA, w, False)
    K2 = np.linalg.inv(A.astype(np.float64)).astype(T)
    K2 = K2 + K2 @ (np.eye(2, dtype=T) - A @ K2)
    K2 = K2 + K2 @ (np.eye(2, dtype=T) - A @ K2)
    VA = VF - w * L
    vF, vA = VF / HF, VA / HF
    EZ = HF / w * (np.sqrt(1 + vF * vF) + np.sqrt(1 + vA * vA)) + (abs(VF) * L + w * L * L / 2) / EA
    col, row = (HF, max(abs(VF), abs(VA))), (XF, EZ)
    Sc = np.array([[A[i, j] * col[j] / row[i] for j in range(2)] for i in range(2)], dtype=np.float64)
    low = min(pA[2], pB[2])
    if VA < 0 and VF > 0:
        low = pA[2] - (HF / w * (vA * vA / (np.sqrt(1 + vA * vA) + 1)) + VA * VA / (2 * EA * w))
    return dict(u=np.array([dx / XF, dy / XF], dtype=T), XF=XF, ZF=ZF, L=L, EA=EA, w=w, HF=HF, VF=VF, HA=HF, VA=VA, A=A, K2=K2,
                kappa=float(np.linalg.norm(np.linalg.inv(Sc), 2)), it=it, conv=conv, low=low)


def shared_state(rec, poseA, poseB, T=np.longdouble):
    """Geometry and solved state of one (unflagged) shared row: the dict of ``mooring_reference.line_state`` with the arms rA,
    rB of both ends and ``low``, the height of the line's lowest point."""
    rec = np.asarray(rec, dtype=np.float64).astype(T)
    xA, xB = np.asarray(poseA, dtype=np.float64).astype(T), np.asarray(poseB, dtype=np.float64).astype(T)
    rA, rB = mr.rotation(xA[3:], T) @ rec[0:3], mr.rotation(xB[3:], T) @ rec[3:6]
    s = _state_from_ends(xA[:3] + rA, xB[:3] + rB, rec[6], rec[7], rec[8], T)
    s.update(rA=rA, rB=rB)
    return s


def _with_span_rounding(q, rec, pose, s, T):
    """The envelopes of ``line_terms`` widened for the rounding of the span.  The kernels form the span of a row from GLOBAL
    coordinates, (x + R r) - a, or (x_B + R_B r_B) - (x_A + R_A r_A): every addend rounds at eps times its own magnitude, so the
    three span components carry an absolute error of eps P, P the sum of the magnitudes of their addends -- at farm
    coordinates (|x| ~ the array's size) far more than eps times the span, and the whole error of an entry that is small only
    because a direction cosine nearly vanishes.  A relative perturbation rho = |P|_1 / XF of the line's geometry turns and
    stretches every output of the row by about rho times that output's size, so each envelope entry grows by rho times the
    largest entry of its own 3-vector or 3 x 3 block (kappa is folded in afterwards, as for every other term)."""
    ub, ua = units_of(rec)
    P = np.abs(pose[ub, :3]).astype(T) + np.abs(s["rB"] if ua >= 0 else s["r"])
    P = P + (np.abs(pose[ua, :3]).astype(T) + np.abs(s["rA"]) if ua >= 0 else np.abs(np.asarray(rec[0:3], dtype=T)))
    rho = (P[0] + P[1] + P[2]) / s["XF"]
    q = dict(q)
    q["EK"] = q["EK"] + rho * np.max(q["EK"])
    q["Ef"] = q["Ef"] + rho * np.max(q["Ef"])
    for nm in ("A", "B"):
        q["Eg" + nm] = q["Eg" + nm] + rho * np.max(q["Eg" + nm])
        q["ET" + nm] = (1 + rho) * q["T" + nm]
    return q


def _carry(K3, EK, ri, rj, T):
    """(block, envelope) of a 3 x 3 translational stiffness carried to two reference points with the arms ri (rows), rj (columns)."""
    RI, RJ = mr.skew(ri, T), mr.skew(rj, T)
    aRI, aRJ = abs(RI), abs(RJ)
    C, E = np.zeros((6, 6), dtype=T), np.zeros((6, 6), dtype=T)
    C[:3, :3], E[:3, :3] = K3, EK
    C[3:, :3], E[3:, :3] = RI @ K3, aRI @ EK
    C[:3, 3:], E[:3, 3:] = -K3 @ RJ, EK @ aRJ
    C[3:, 3:], E[3:, 3:] = -RI @ K3 @ RJ, aRI @ EK @ aRJ
    return C, E


def evaluate(lines, pose, depth, T=np.longdouble):
    """ONE array: lines [nL,16], pose [nUnit,6].  dict of C [n,n], F [n], T [2 nL], J [2 nL,n] (n = 6 nUnit), their envelopes EC,
    EF, ET, EJ (kappa folded in), flags (int), low (the lowest point of every shared row, NaN for anchored rows), iterations
    per row.  A flagged array is NaN."""
    lines = np.asarray(lines, dtype=np.float64)
    pose = np.asarray(pose, dtype=np.float64)
    nL, nU = len(lines), len(pose)
    n = 6 * nU
    out = dict(C=np.zeros((n, n), dtype=T), F=np.zeros(n, dtype=T), T=np.zeros(2 * nL, dtype=T), J=np.zeros((2 * nL, n), dtype=T),
               flags=0, low=np.full(nL, np.nan), kappa=np.zeros(nL))
    for k in ("C", "F", "T", "J"):
        out["E" + k] = np.zeros_like(out[k])
    for l in range(nL):
        ub, ua = units_of(lines[l])
        out["flags"] |= shared_flag(lines[l], pose[ua], pose[ub], depth) if ua >= 0 else mr.line_flag(lines[l], pose[ub], depth)
    states = []
    if not out["flags"]:
        for l in range(nL):
            ub, ua = units_of(lines[l])
            s = shared_state(lines[l], pose[ua], pose[ub], T) if ua >= 0 else mr.line_state(lines[l], pose[ub], depth, T)
            if not s["conv"]:
                out["flags"] |= mr.FLAG_NO_CONVERGENCE
            elif ua >= 0:
                out["low"][l] = float(s["low"])
                if s["low"] < -depth - 1e-6 * depth:
                    out["flags"] |= FLAG_GROUNDED
            states.append(s)
    if out["flags"]:
        for k in ("C", "F", "T", "J"):
            out[k][...] = np.nan
        return out
    for l, s in enumerate(states):
        ub, ua = units_of(lines[l])
        q = _with_span_rounding(mr.line_terms(s, T), lines[l], pose, s, T)
        k1 = 1 + T(s["kappa"])
        out["kappa"][l] = s["kappa"]
        ends = [(ub, s["rB"] if ua >= 0 else s["r"], q["f"], 1)]
        if ua >= 0:
            fA = np.array([s["HF"] * s["u"][0], s["HF"] * s["u"][1], s["VA"]], dtype=T)
            ends.append((ua, s["rA"], fA, -1))
        for ui, ri, fi, si in ends:
            bi = slice(6 * ui, 6 * ui + 6)
            for uj, rj, _, sj in ends:
                C, E = _carry(q["K3"], q["EK"], ri, rj, T)
                bj = slice(6 * uj, 6 * uj + 6)
                out["C"][bi, bj] += (si * sj) * C
                out["EC"][bi, bj] += k1 * E
            RI, FI = mr.skew(ri, T), mr.skew(fi, T)
            out["C"][6 * ui + 3:6 * ui + 6, 6 * ui + 3:6 * ui + 6] += -FI @ RI
            Efi = q["Ef"] + (abs(fi) - abs(q["f"]))             # (end A: the magnitudes of its own force, the same widening)
            out["EC"][6 * ui + 3:6 * ui + 6, 6 * ui + 3:6 * ui + 6] += k1 * (abs(mr.skew(Efi, T)) @ abs(RI))
            out["F"][6 * ui:6 * ui + 3] += fi
            out["F"][6 * ui + 3:6 * ui + 6] += RI @ fi
            out["EF"][6 * ui:6 * ui + 3] += k1 * Efi
            out["EF"][6 * ui + 3:6 * ui + 6] += k1 * (abs(RI) @ Efi)
            for e, nm in ((0, "A"), (1, "B")):
                i = e * nL + l
                out["J"][i, 6 * ui:6 * ui + 3] += si * q["g" + nm]
                out["J"][i, 6 * ui + 3:6 * ui + 6] += si * (RI @ q["g" + nm])
                out["EJ"][i, 6 * ui:6 * ui + 3] += k1 * q["Eg" + nm]
                out["EJ"][i, 6 * ui + 3:6 * ui + 6] += k1 * (abs(RI) @ q["Eg" + nm])
        for e, nm in ((0, "A"), (1, "B")):
            out["T"][e * nL + l] = q["T" + nm]
            out["ET"][e * nL + l] = k1 * q["ET" + nm]
    return out


def forces(lines, pose, depth, dx=None, T=np.longdouble):
    """(F [n], tensions [2 nL]) of ONE array with every unit displaced by dx[6u:6u+3] and turned by the rotation vector
    dx[6u+3:6u+6] about its reference point on top of its pose's rotation: the function ``fd_check`` differentiates."""
    lines = np.asarray(lines, dtype=np.float64)
    pose = np.asarray(pose, dtype=np.float64).astype(T)
    nL, nU = len(lines), len(pose)
    dx = np.zeros(6 * nU, dtype=T) if dx is None else np.asarray(dx, dtype=T)
    F, Tn = np.zeros(6 * nU, dtype=T), np.zeros(2 * nL, dtype=T)

    def arm(u, rf):
        TX = mr.skew(dx[6 * u + 3:6 * u + 6], T)
        return (np.eye(3, dtype=T) + TX + TX @ TX / 2) @ (mr.rotation(pose[u, 3:], T) @ rf)

    for l in range(nL):
        rec = lines[l].astype(T)
        ub, ua = units_of(lines[l])
        if ua < 0:
            R = mr.rotation(pose[ub, 3:], T)
            f6, TA, TB = mr.forces_perturbed(lines[l], R, pose[ub, :3], dx[6 * ub:6 * ub + 6], depth, T)
            F[6 * ub:6 * ub + 6] += f6
        else:
            rA, rB = arm(ua, rec[0:3]), arm(ub, rec[3:6])
            s = _state_from_ends(pose[ua, :3] + dx[6 * ua:6 * ua + 3] + rA, pose[ub, :3] + dx[6 * ub:6 * ub + 3] + rB, rec[6], rec[7], rec[8], T)
            fB = np.array([-s["HF"] * s["u"][0], -s["HF"] * s["u"][1], -s["VF"]], dtype=T)
            fA = np.array([s["HF"] * s["u"][0], s["HF"] * s["u"][1], s["VA"]], dtype=T)
            F[6 * ub:6 * ub + 3] += fB
            F[6 * ub + 3:6 * ub + 6] += np.cross(rB, fB)
            F[6 * ua:6 * ua + 3] += fA
            F[6 * ua + 3:6 * ua + 6] += np.cross(rA, fA)
            TA, TB = np.sqrt(s["HF"] ** 2 + s["VA"] ** 2), np.sqrt(s["HF"] ** 2 + s["VF"] ** 2)
        Tn[l], Tn[nL + l] = TA, TB
    return F, Tn


def fd_check(lines, pose, depth, h=1e-4):
    """Worst |analytic - central difference| / envelope of C and J of one array, over all 6 nUnit DOFs."""
    T = np.longdouble
    ref = evaluate(lines, pose, depth)
    n = 6 * len(pose)
    Cfd, Jfd = np.zeros((n, n), dtype=T), np.zeros((2 * len(lines), n), dtype=T)
    for j in range(n):
        d = np.zeros(n, dtype=T)
        d[j] = T(h)
        Fp, Tp = forces(lines, pose, depth, d)
        Fm, Tm = forces(lines, pose, depth, -d)
        Cfd[:, j] = -(Fp - Fm) / (2 * T(h))
        Jfd[:, j] = (Tp - Tm) / (2 * T(h))
    tiny = np.finfo(np.float64).tiny
    # (an exactly zero envelope must come with an exactly zero difference: those entries are checked apart)
    zc, zj = ref["EC"] == 0, ref["EJ"] == 0
    assert np.all(np.abs(Cfd[zc]) <= 1e-6 * np.abs(Cfd).max()) and np.all(ref["C"][zc] == 0)
    assert np.all(np.abs(Jfd[zj]) <= 1e-6 * np.abs(Jfd).max()) and np.all(ref["J"][zj] == 0)
    eC = np.where(zc, 0, np.abs(ref["C"] - Cfd) / np.maximum(ref["EC"], tiny))
    eJ = np.where(zj, 0, np.abs(ref["J"] - Jfd) / np.maximum(ref["EJ"], tiny))
    return float(eC.max()), float(eJ.max())


def _solve_lin(K, Y):
    T = np.longdouble
    K64 = K.astype(np.float64)
    x = np.linalg.solve(K64, Y.astype(np.float64)).astype(T)
    for _ in range(3):
        x = x + np.linalg.solve(K64, (Y - K @ x).astype(np.float64)).astype(T)
    return x


def solve(lines, depth, K_hs, F0, F_env, x_ref, max_it=40):
    """Plain Newton over the 6 nUnit DOFs from x_ref [nUnit,6] (fp64 iterates, longdouble evaluation; no safeguards: a case that
    needs them, or that is flagged at an iterate, is not a case for this reference -- ValueError).  dict of the root x [n]
    (longdouble), iterations, K, Kinv_abs, E_F [n], bound = |K^-1| E_F [n], moor (``evaluate`` at the fp64 rounding of the
    root) and lows (the lowest point of the shared rows at every iterate)."""
    T = np.longdouble
    K_hs = np.asarray(K_hs, dtype=np.float64).astype(T)
    nU = len(K_hs)
    n = 6 * nU
    F0 = np.asarray(F0, dtype=np.float64).astype(T).reshape(n)
    F_env = np.zeros(n, dtype=T) if F_env is None else np.asarray(F_env, dtype=np.float64).astype(T).reshape(n)
    xr = np.asarray(x_ref, dtype=np.float64).astype(T).reshape(n)
    Kd = np.zeros((n, n), dtype=T)
    for u in range(nU):
        Kd[6 * u:6 * u + 6, 6 * u:6 * u + 6] = K_hs[u]
    x = xr.astype(np.float64)
    last, it, lows = np.inf, 0, []
    while True:
        m = evaluate(lines, x.reshape(nU, 6), depth)
        if m["flags"]:
            raise ValueError("the array reference flags the iterate %d: %d" % (it, m["flags"]))
        lows.append(m["low"])
        Y = F0 + F_env - Kd @ (x.astype(T) - xr) + m["F"]
        K = Kd + m["C"]
        dX = _solve_lin(K, Y)
        size = float(np.max(np.abs(dX)))
        if size >= last or size == 0.0 or it >= max_it:
            break
        x = (x.astype(T) + dX).astype(np.float64)
        last = size
        it += 1
    if it >= max_it:
        raise ValueError("the reference iteration did not stagnate in %d steps" % max_it)
    root = x.astype(T) + dX
    Kinv = np.abs(np.linalg.inv(K.astype(np.float64))).astype(T)
    E_F = np.abs(F0) + np.abs(F_env) + np.abs(Kd) @ np.abs(root - xr) + m["EF"]
    return dict(x=root, iterations=it, K=K, Kinv_abs=Kinv, E_F=E_F, bound=Kinv @ E_F, moor=m, lows=lows)


def multiples(v, ref, scale):
    """|v - ref| / (eps scale) per entry, any shape: ``mooring_reference.gate_multiples``."""
    return mr.gate_multiples(v, ref, scale)


def worst_multiples(res, ref):
    """Worst multiple of eps E per output of a result dict (C, F, T, J) against ``evaluate``'s."""
    return {k: float(mr.gate_multiples(np.asarray(res[k]).reshape(ref[k].shape), ref[k], ref["E" + k]).max()) for k in ("C", "F", "T", "J")}
