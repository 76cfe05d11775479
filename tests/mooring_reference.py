"""Independent evaluation of the quasi-static mooring system of include/raftx_mooring.h in ``numpy.longdouble``: the
reference of tests/test_mooring.py and tests/test_hip_mooring.py.

Every line is one elastic catenary segment from a fixed anchor to a point on the vessel (Jonkman 2007, "Dynamics
Modeling and Loads Analysis of an Offshore Floating Wind Turbine", eqs. 2-35 .. 2-38), in two branches:

    no contact                          XF = HF/w (asinh vF - asinh vA) + HF L/EA
    (VF >= wL, or anchor off the bed)   ZF = HF/w (sF - sA) + (VF L - w L^2/2)/EA         vF = VF/HF, vA = (VF - wL)/HF
    contact, CB = 0                     XF = L_B + HF/w asinh vF + HF L/EA                L_B = L - VF/w
    (VF < wL, anchor on the bed)        ZF = HF/w (sF - 1) + VF^2/(2 EA w)                s. = sqrt(1 + v.^2)

``evaluate(lines, pose, depth)`` solves (HF, VF) of every line to longdouble stagnation (Newton from the lambda guess,
the branch re-chosen at every evaluation) and returns, per design, C_moor [6,6] = -dF_moor/dx6, F_moor [6], T [2 nLine]
(ends A, then ends B), J [2 nLine,6] = dT/dx6 by ANALYTIC differentiation -- ``fd_check`` compares C and J with central
differences of this file's own force function -- and for each of them the envelope

    Ek = sum over the design's lines of (1 + kappa_line) E_line

where E_line is the same sum of products with every addend replaced by its magnitude (for one line this is the
(1 + kappa) E of DESIGN.md section 4) and kappa_line the 2-norm condition number of the line's catenary Jacobian
d(XF, ZF)/d(HF, VF) scaled by (HF, VF) and (XF, ZF).  The accuracy gate is |x - ref| <= C eps Ek per entry; where
Ek == 0 the result must be exactly 0.

No code is shared with raft_amd or the kernels, but the catenary expressions and the iteration are the same ones restated
in longdouble: a formula wrong in both would agree.  Independence comes from elsewhere: the recorded Tmoor_avg of the
reference's decks (tests/golden/refgold_mooring.npz, rtol 1e-5) pins the solve, and ``fd_check`` pins C and J against
central differences of the force function.  Rotations are Rz Ry Rx of (roll, pitch, yaw); rotational columns
of C and J are derivatives with respect to an infinitesimal rotation vector about the reference point applied on top of
the pose's rotation.
"""
import numpy as np

ML_N = 16
EPS = float(np.finfo(np.float64).eps)
FLAG_BAD_LINE, FLAG_VERTICAL, FLAG_SLACK, FLAG_NO_CONVERGENCE = 1, 2, 4, 8

# Worst multiple of eps Ek of the fp64 model of the device algorithm (tests/mooring_device_model.py) over the batches of
# tests/mooring_cases.py, measured on the CPU: 2.34 (a J entry of the nearly taut line; C of the same line 2.33, every
# other batch <= 1.05).  GATE_C is the power of two at or above 4 x that.
GATE_WORST_CPU = 2.34
GATE_C = 16


def rotation(ang, T=np.longdouble):
    """Rz(yaw) Ry(pitch) Rx(roll)."""
    r, p, y = (T(a) for a in ang)
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]], dtype=T)
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]], dtype=T)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]], dtype=T)
    return Rz @ Ry @ Rx


def skew(v, T=np.longdouble):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype=T)


def catenary(HF, VF, L, EA, w, seabed):
    """X, Z, the Jacobian A = d(X, Z)/d(HF, VF) and the branch (1: seabed contact) at (HF, VF)."""
    T = type(HF)
    W = w * L
    vF = VF / HF
    sF = np.sqrt(1 + vF * vF)
    aF = np.arcsinh(vF)
    if seabed and VF < W:
        LB = L - VF / w
        X = LB + HF / w * aF + HF * L / EA
        Z = HF / w * (vF * vF / (sF + 1)) + VF * VF / (2 * EA * w)
        a11 = (aF - vF / sF) / w + L / EA
        a12 = -(vF * vF / (sF * (sF + 1))) / w
        a22 = vF / sF / w + VF / (EA * w)
        branch = 1
    else:
        vA = (VF - W) / HF
        sA = np.sqrt(1 + vA * vA)
        aA = np.arcsinh(vA)
        X = HF / w * (aF - aA) + HF * L / EA
        Z = HF / w * ((W / HF) * (vF + vA) / (sF + sA)) + (VF * L - W * L / 2) / EA
        a11 = ((aF - aA) - (vF / sF - vA / sA)) / w + L / EA
        a12 = -((W / HF) * (vF + vA) / ((sF + sA) * sF * sA)) / w
        a22 = (vF / sF - vA / sA) / w + L / EA
        branch = 0
    A = np.array([[a11, a12], [a12, a22]], dtype=T)
    return X, Z, A, branch


def solve_line(XF, ZF, L, EA, w, seabed, max_it=200):
    """(HF, VF, A, branch, iterations, converged) of one line, to stagnation of the residual in the working precision."""
    T = type(XF)
    if L * L <= XF * XF + ZF * ZF:
        lam = T(0.2)
    else:
        lam = np.sqrt(3 * ((L * L - ZF * ZF) / (XF * XF) - 1))
    H = abs(w * XF / (2 * lam))
    V = w / 2 * (ZF / np.tanh(lam) + L)
    tight = T(1e-10)

    def res(H, V):
        X, Z, A, br = catenary(H, V, L, EA, w, seabed)
        return X - XF, Z - ZF, A, br

    eX, eZ, A, br = res(H, V)
    r = max(abs(eX), abs(eZ)) / L
    a, it, conv = T(1), 0, r == 0
    while not conv and it < max_it:
        it += 1
        det = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
        dH = -(A[1, 1] * eX - A[0, 1] * eZ) / det
        dV = -(A[0, 0] * eZ - A[1, 0] * eX) / det
        s = a
        if H + s * dH <= 0:
            s = -H / dH / 2
        tX, tZ, tA, tbr = res(H + s * dH, V + s * dV)
        rt = max(abs(tX), abs(tZ)) / L
        if rt < r:
            H, V, eX, eZ, A, br, r, a = H + s * dH, V + s * dV, tX, tZ, tA, tbr, rt, T(1)
            conv = r == 0
        elif r <= tight:
            conv = True
        else:
            a = a / 2
            if a < 2.0 ** -40:
                break
    return H, V, A, br, it, conv


def line_flag(rec, pose, depth):
    """The flag of one line record at a pose (fp64 tests, the conditions of include/raftx_mooring.h), or 0."""
    rec = np.asarray(rec, dtype=np.float64)
    if not (np.all(np.isfinite(rec[:10])) and np.all(np.isfinite(pose))):
        return FLAG_BAD_LINE
    a, L, EA, w = rec[0:3], rec[6], rec[7], rec[8]
    if not (L > 0 and EA > 0 and w > 0) or a[2] < -depth - 1e-6 * depth:
        return FLAG_BAD_LINE
    p = np.asarray(pose[:3], dtype=np.float64) + np.asarray(rotation(pose[3:], np.float64) @ rec[3:6])
    XF, ZF = np.hypot(p[0] - a[0], p[1] - a[1]), p[2] - a[2]
    if not ZF > 0:
        return FLAG_BAD_LINE
    if XF <= 1e-9 * L:
        return FLAG_VERTICAL
    if L >= XF + ZF:
        return FLAG_SLACK
    return 0


def line_state(rec, pose, depth, T=np.longdouble):
    """Geometry and solved state of one (unflagged) line: a dict with r, u, XF, ZF, HF, VF, HA, VA, LB, A, K2, kappa..."""
    rec = np.asarray(rec, dtype=np.float64).astype(T)
    a, rf, L, EA, w = rec[0:3], rec[3:6], rec[6], rec[7], rec[8]
    x = np.asarray(pose, dtype=np.float64).astype(T)
    r = rotation(x[3:], T) @ rf
    p = x[:3] + r
    dx, dy = p[0] - a[0], p[1] - a[1]
    XF = np.sqrt(dx * dx + dy * dy)
    ZF = p[2] - a[2]
    seabed = bool(abs(float(rec[2]) + depth) <= 1e-6 * depth)
    HF, VF, A, br, it, conv = solve_line(XF, ZF, L, EA, w, seabed)
    K2 = np.linalg.inv(A.astype(np.float64)).astype(T)
    K2 = K2 + K2 @ (np.eye(2, dtype=T) - A @ K2)                      # two refinement steps in T
    K2 = K2 + K2 @ (np.eye(2, dtype=T) - A @ K2)
    Sc = np.array([[A[i, j] * (HF, VF)[j] / (XF, ZF)[i] for j in range(2)] for i in range(2)], dtype=np.float64)
    kappa = float(np.linalg.cond(Sc))
    VA = T(0) if br else VF - w * L
    LB = L - VF / w if br else T(0)
    return dict(a=a, r=r, p=p, u=np.array([dx / XF, dy / XF], dtype=T), XF=XF, ZF=ZF, L=L, EA=EA, w=w, HF=HF, VF=VF, HA=HF,
                VA=VA, LB=LB, A=A, K2=K2, kappa=kappa, branch=br, it=it, conv=conv)


def line_terms(s, T=np.longdouble):
    """f, K3, gA, gB, TA, TB of a solved line and the magnitude envelopes of each (E_*)."""
    HF, VF, VA, XF, u, K2 = s["HF"], s["VF"], s["VA"], s["XF"], s["u"], s["K2"]
    u3 = np.array([u[0], u[1], 0], dtype=T)
    f = np.array([-HF * u[0], -HF * u[1], -VF], dtype=T)
    t = HF / XF
    K3 = np.zeros((3, 3), dtype=T)
    EK = np.zeros((3, 3), dtype=T)
    for i in range(2):
        for j in range(2):
            K3[i, j] = K2[0, 0] * u[i] * u[j] + t * ((1 if i == j else 0) - u[i] * u[j])
            EK[i, j] = abs(K2[0, 0] * u[i] * u[j]) + t * ((1 if i == j else 0) + abs(u[i] * u[j]))
        K3[i, 2] = K2[0, 1] * u[i]
        K3[2, i] = K2[1, 0] * u[i]
        EK[i, 2] = abs(K3[i, 2])
        EK[2, i] = abs(K3[2, i])
    K3[2, 2] = K2[1, 1]
    EK[2, 2] = abs(K2[1, 1])
    TB = np.sqrt(HF * HF + VF * VF)
    TA = np.sqrt(HF * HF + VA * VA)
    out = dict(f=f, Ef=abs(f), K3=K3, EK=EK, TA=TA, TB=TB)
    for nm, Vx, Tx in (("A", VA, TA), ("B", VF, TB)):
        gX = (HF * K2[0, 0] + Vx * K2[1, 0]) / Tx
        gZ = (HF * K2[0, 1] + Vx * K2[1, 1]) / Tx
        eX = (abs(HF * K2[0, 0]) + abs(Vx * K2[1, 0])) / Tx
        eZ = (abs(HF * K2[0, 1]) + abs(Vx * K2[1, 1])) / Tx
        out["g" + nm] = np.array([gX * u[0], gX * u[1], gZ], dtype=T)
        out["Eg" + nm] = np.array([eX * abs(u[0]), eX * abs(u[1]), eZ], dtype=T)
    return out


def evaluate(lines, pose, depth, T=np.longdouble, seed=None):
    """dict of C [nD,6,6], F [nD,6], T [nD,2nL], J [nD,2nL,6], line_out [nD,nL,8], flags [nD], kappa [nD,nL] and the
    envelopes EC, EF, ET, EJ (kappa folded in).  Flagged designs are NaN.  ``seed``: the name of a deliberate error
    (tests of the gate only; never set otherwise)."""
    lines = np.asarray(lines, dtype=np.float64)
    nD, nL = lines.shape[:2]
    pose = np.zeros((nD, 6)) if pose is None else np.asarray(pose, dtype=np.float64).reshape(nD, 6)
    out = dict(C=np.zeros((nD, 6, 6), dtype=T), F=np.zeros((nD, 6), dtype=T), T=np.zeros((nD, 2 * nL), dtype=T),
               J=np.zeros((nD, 2 * nL, 6), dtype=T), line_out=np.zeros((nD, nL, 8), dtype=T),
               flags=np.zeros(nD, dtype=np.int32), kappa=np.zeros((nD, nL)))
    for k in ("C", "F", "T", "J"):
        out["E" + k] = np.zeros_like(out[k])
    for d in range(nD):
        for l in range(nL):
            out["flags"][d] |= line_flag(lines[d, l], pose[d], depth)
        if out["flags"][d]:
            continue
        for l in range(nL):
            s = line_state(lines[d, l], pose[d], depth, T)
            if not s["conv"]:
                out["flags"][d] |= FLAG_NO_CONVERGENCE
                break
            q = line_terms(s, T)
            k1 = 1 + T(s["kappa"])
            r, f, K3 = s["r"], q["f"], q["K3"]
            RX, FX = skew(r, T), skew(f, T)
            aRX, aFX = abs(RX), abs(FX)
            C, E = np.zeros((6, 6), dtype=T), np.zeros((6, 6), dtype=T)
            C[:3, :3], E[:3, :3] = K3, q["EK"]
            C[3:, :3], E[3:, :3] = RX @ K3, aRX @ q["EK"]
            C[:3, 3:], E[:3, 3:] = -K3 @ RX, q["EK"] @ aRX
            C[3:, 3:], E[3:, 3:] = -RX @ K3 @ RX - FX @ RX, aRX @ q["EK"] @ aRX + aFX @ aRX
            out["C"][d] += C
            out["EC"][d] += k1 * E
            out["F"][d, :3] += f
            out["F"][d, 3:] += RX @ f
            out["EF"][d, :3] += k1 * q["Ef"]
            out["EF"][d, 3:] += k1 * (aRX @ q["Ef"])
            for e, nm in ((0, "A"), (1, "B")):
                i = e * nL + l
                out["T"][d, i] = q["T" + nm]
                out["ET"][d, i] = k1 * q["T" + nm]
                out["J"][d, i, :3] = q["g" + nm]
                out["J"][d, i, 3:] = RX @ q["g" + nm]
                out["EJ"][d, i, :3] = k1 * q["Eg" + nm]
                out["EJ"][d, i, 3:] = k1 * (aRX @ q["Eg" + nm])
            out["line_out"][d, l] = [s["HF"], s["VF"], s["HA"], s["VA"], s["LB"], s["it"], s["branch"], 0]
            out["kappa"][d, l] = s["kappa"]
    bad = out["flags"] != 0
    for k in ("C", "F", "T", "J", "line_out"):
        out[k][bad] = np.nan
    return out


def forces(lines_d, pose_d, depth, T=np.longdouble):
    """F_moor [6] and the tensions [2 nL] of ONE design at a pose: the function ``fd_check`` differentiates."""
    nL = len(lines_d)
    F, Tn = np.zeros(6, dtype=T), np.zeros(2 * nL, dtype=T)
    for l in range(nL):
        s = line_state(lines_d[l], pose_d, depth, T)
        q = line_terms(s, T)
        F[:3] += q["f"]
        F[3:] += np.cross(s["r"], q["f"])
        Tn[l], Tn[nL + l] = q["TA"], q["TB"]
    return F, Tn


def forces_perturbed(rec_l, R, x, dx6, depth, T=np.longdouble):
    """One line's (f, r x f, TA, TB) with the unit displaced by dx6[:3] and turned by the rotation vector dx6[3:] about
    the reference point on top of R: the arm is (I + [th x] + [th x]^2 / 2) R r_f, exact to second order."""
    rec = np.asarray(rec_l, dtype=np.float64).astype(T)
    th = np.asarray(dx6[3:], dtype=T)
    TX = skew(th, T)
    r = (np.eye(3, dtype=T) + TX + TX @ TX / 2) @ (R @ rec[3:6])
    p = x + np.asarray(dx6[:3], dtype=T) + r
    a, L, EA, w = rec[0:3], rec[6], rec[7], rec[8]
    ddx, ddy = p[0] - a[0], p[1] - a[1]
    XF, ZF = np.sqrt(ddx * ddx + ddy * ddy), p[2] - a[2]
    seabed = bool(abs(float(rec[2]) + depth) <= 1e-6 * depth)
    HF, VF, A, br, it, conv = solve_line(XF, ZF, L, EA, w, seabed)
    f = np.array([-HF * ddx / XF, -HF * ddy / XF, -VF], dtype=T)
    VA = T(0) if br else VF - w * L
    return np.concatenate([f, np.cross(r, f)]), np.sqrt(HF * HF + VA * VA), np.sqrt(HF * HF + VF * VF)


def fd_check(lines_d, pose_d, depth, h=1e-4):
    """Worst |analytic - central difference| / envelope of C and J of one design (longdouble; the differences are
    O(h^2) accurate, so a correct derivative gives about h^2 times a curvature ratio)."""
    T = np.longdouble
    lines_d = np.asarray(lines_d, dtype=np.float64)
    nL = len(lines_d)
    ref = evaluate(lines_d[None], np.asarray(pose_d, dtype=np.float64)[None], depth)
    x = np.asarray(pose_d, dtype=np.float64).astype(T)
    R = rotation(x[3:], T)
    Cfd, Jfd = np.zeros((6, 6), dtype=T), np.zeros((2 * nL, 6), dtype=T)
    for j in range(6):
        d6 = np.zeros(6, dtype=T)
        d6[j] = T(h)
        for l in range(nL):
            Fp, TAp, TBp = forces_perturbed(lines_d[l], R, x[:3], d6, depth)
            Fm, TAm, TBm = forces_perturbed(lines_d[l], R, x[:3], -d6, depth)
            Cfd[:, j] -= (Fp - Fm) / (2 * T(h))
            Jfd[l, j] = (TAp - TAm) / (2 * T(h))
            Jfd[nL + l, j] = (TBp - TBm) / (2 * T(h))
    eC = np.abs(ref["C"][0] - Cfd) / np.maximum(ref["EC"][0], np.finfo(np.float64).tiny)
    eJ = np.abs(ref["J"][0] - Jfd) / np.maximum(ref["EJ"][0], np.finfo(np.float64).tiny)
    return float(eC.max()), float(eJ.max())


def gate_multiples(x, ref, Ek):
    """|x - ref| / (eps Ek) per entry; entries with Ek == 0 give 0 where x is exactly 0 and inf otherwise; where the
    reference is NaN the entry gives 0 if x is NaN too and inf otherwise.  No entry is left out."""
    x, ref, Ek = (np.asarray(a, dtype=np.longdouble) for a in (x, ref, Ek))
    out = np.full(ref.shape, np.inf)
    nan = np.isnan(ref)
    out[nan & np.isnan(x)] = 0.0
    zero = ~nan & (Ek == 0)
    out[zero & (x == 0)] = 0.0
    ok = ~nan & ~zero & np.isfinite(x)
    out[ok] = (np.abs(x[ok] - ref[ok]) / (EPS * Ek[ok])).astype(np.float64)
    return out
