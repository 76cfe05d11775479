"""fp64 NumPy restatement of the device algorithm of raft_amd/csrc/raftx_mooring.h (k_moor_line + k_moor_design): the
same expressions in the same order, one line at a time.  It is what the gate's constant of tests/mooring_reference.py
is measured with on the CPU, and -- through ``seed`` -- the carrier of the deliberate errors the gate must reject
(tests/test_mooring.py).  The kernels contract multiply-adds and use the device's asinh / tanh, so the model agrees with
them to rounding, not to the bit.
"""
import numpy as np

MAX_IT = 60
TIGHT = 1e-10
SEEDS = ("no_stretch", "lb_stretched", "arm_sign", "no_coupling", "ja_from_b")


def _eval(H, V, L, EA, w, seabed, seed):
    W = w * L
    vF = V / H
    sF = np.sqrt(1.0 + vF * vF)
    aF = np.arcsinh(vF)
    st = 0.0 if seed == "no_stretch" else L / EA                 # the stretch term H L/EA and its derivative
    if seabed and V < W:
        LB = L - V / w
        X = LB + (H / w) * aF + H * st
        if seed == "lb_stretched":
            X = X + H * L / EA                                    # L_B from the stretched length L (1 + H/EA)
        Z = (H / w) * (vF * vF / (sF + 1.0)) + V * V / (2.0 * EA * w)
        a11 = (aF - vF / sF) / w + st
        a12 = -(vF * vF / (sF * (sF + 1.0))) / w
        a22 = vF / sF / w + V / (EA * w)
        return X, Z, a11, a12, a22, 1
    vA = (V - W) / H
    sA = np.sqrt(1.0 + vA * vA)
    aA = np.arcsinh(vA)
    q = (W / H) * (vF + vA) / (sF + sA)
    X = (H / w) * (aF - aA) + H * st
    Z = (H / w) * q + (V * L - 0.5 * W * L) / EA
    a11 = ((aF - aA) - (vF / sF - vA / sA)) / w + st
    a12 = -(q / (sF * sA)) / w
    a22 = (vF / sF - vA / sA) / w + L / EA
    return X, Z, a11, a12, a22, 0


def _arm(rf, ang):
    """R r_f as geom_pose leaves it: r_f + (R - I) r_f, R = Rz Ry Rx of (roll, pitch, yaw)."""
    sr, cr, sp, cp, sy, cy = np.sin(ang[0]), np.cos(ang[0]), np.sin(ang[1]), np.cos(ang[1]), np.sin(ang[2]), np.cos(ang[2])
    R = np.array([[cy * cp, cy * sp * sr - cr * sy, sy * sr + cy * cr * sp],
                  [cp * sy, cy * cr + sy * sp * sr, cr * sy * sp - cy * sr],
                  [-sp, cp * sr, cp * cr]])
    r = np.zeros(3)
    for i in range(3):
        dsp = (R[i, 0] - (i == 0)) * rf[0] + (R[i, 1] - (i == 1)) * rf[1] + (R[i, 2] - (i == 2)) * rf[2]
        r[i] = rf[i] + (0.0 + dsp)
    return r


def newton(ev, Lt, we, XF, ZF):
    """(conv, H, V, it, last evaluation) of one element between ends XF, ZF apart: moor_shoot, THE damped Newton iteration on
    (H, V), cold start.  ev(H, V) -> (X, Z, a11, a12, a22, ...); Lt, we: the length and weight per length of the guess."""
    lam = 0.2 if Lt * Lt <= XF * XF + ZF * ZF else np.sqrt(3.0 * ((Lt * Lt - ZF * ZF) / (XF * XF) - 1.0))
    H, V = abs(we * XF / (2.0 * lam)), 0.5 * we * (ZF / np.tanh(lam) + Lt)
    cur = ev(H, V)
    eX, eZ = cur[0] - XF, cur[1] - ZF
    res, a, it = max(abs(eX), abs(eZ)) / Lt, 1.0, 0
    conv = res == 0.0
    while not conv and it < MAX_IT:
        it += 1
        a11, a12, a22 = cur[2:5]
        det = a11 * a22 - a12 * a12
        dH, dV = -(a22 * eX - a12 * eZ) / det, -(a11 * eZ - a12 * eX) / det
        s = a
        if H + s * dH <= 0.0:
            s = -0.5 * H / dH
        Ht, Vt = H + s * dH, V + s * dV
        nx = ev(Ht, Vt)
        nX, nZ = nx[0] - XF, nx[1] - ZF
        rn = max(abs(nX), abs(nZ)) / Lt
        if rn < res:
            H, V, eX, eZ, res, a, cur = Ht, Vt, nX, nZ, rn, 1.0, nx
            conv = res == 0.0
        elif res <= TIGHT:
            conv = True
        else:
            a *= 0.5
            if a < 2.0 ** -40:
                break
    return conv, H, V, it, cur


def end(H, V, a11, a12, a22, ux, uy, XF):
    """A solved element (MoorEnd / moor_end_set): (k) the inverse of its catenary Jacobian and the 3 x 3 end stiffness K."""
    det = a11 * a22 - a12 * a12
    k11, k12, k22 = a22 / det, -a12 / det, a11 / det
    th = H / XF
    K = np.array([[k11 * ux * ux + th * (1.0 - ux * ux), k11 * ux * uy - th * (ux * uy), k12 * ux],
                  [k11 * ux * uy - th * (ux * uy), k11 * uy * uy + th * (1.0 - uy * uy), k12 * uy],
                  [k12 * ux, k12 * uy, k22]])
    return dict(H=H, V=V, ux=ux, uy=uy, k11=k11, k12=k12, k22=k22, K=K)


def end_grad(m, Vx, Tx):
    """The gradient of the tension Tx where the element's vertical force is Vx (moor_end_grad)."""
    gX, gZ = (m["H"] * m["k11"] + Vx * m["k12"]) / Tx, (m["H"] * m["k12"] + Vx * m["k22"]) / Tx
    return np.array([gX * m["ux"], gX * m["uy"], gZ])


def line(rec, ps, depth, seed=None):
    """(flag, dict) of one line: the record k_moor_line writes."""
    rec = np.asarray(rec, dtype=np.float64)
    ps = np.asarray(ps, dtype=np.float64)
    L, EA, w, az = rec[6], rec[7], rec[8], rec[2]
    if not (np.all(np.isfinite(rec[:10])) and np.all(np.isfinite(ps))) or not (L > 0 and EA > 0 and w > 0) or az < -depth - 1e-6 * depth:
        return 1, None
    r = _arm(rec[3:6], ps[3:])
    dx, dy = (ps[0] + r[0]) - rec[0], (ps[1] + r[1]) - rec[1]
    XF = np.sqrt(dx * dx + dy * dy)
    ZF = (ps[2] + r[2]) - az
    if not ZF > 0:
        return 1, None
    if XF <= 1e-9 * L:
        return 2, None
    if L >= XF + ZF:
        return 4, None
    ux, uy = dx / XF, dy / XF
    seabed = abs(az + depth) <= 1e-6 * depth
    conv, H, V, it, (_, _, a11, a12, a22, ct) = newton(lambda H, V: _eval(H, V, L, EA, w, seabed, seed), L, w, XF, ZF)
    if not conv:
        return 8, None
    m = end(H, V, a11, a12, a22, ux, uy, XF)
    VA = 0.0 if ct else V - w * L
    TB, TA = np.sqrt(H * H + V * V), np.sqrt(H * H + VA * VA)
    return 0, dict(f=np.array([-H * ux, -H * uy, -V]), r=r, K=m["K"], gA=end_grad(m, VA, TA), gB=end_grad(m, V, TB), TA=TA, TB=TB,
                   lo=np.array([H, V, H, VA, L - V / w if ct else 0.0, it, ct, 0.0]))


def _skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def evaluate(lines, pose, depth, seed=None):
    """dict C [nD,6,6], F [nD,6], T [nD,2nL], J [nD,2nL,6], line_out [nD,nL,8], flags [nD] as raftx_mooring_lines."""
    assert seed is None or seed in SEEDS
    lines = np.asarray(lines, dtype=np.float64)
    nD, nL = lines.shape[:2]
    pose = np.zeros((nD, 6)) if pose is None else np.asarray(pose, dtype=np.float64).reshape(nD, 6)
    out = dict(C=np.zeros((nD, 6, 6)), F=np.zeros((nD, 6)), T=np.zeros((nD, 2 * nL)), J=np.zeros((nD, 2 * nL, 6)),
               line_out=np.full((nD, nL, 8), np.nan), flags=np.zeros(nD, dtype=np.int32))
    for d in range(nD):
        recs = [line(lines[d, l], pose[d], depth, seed) for l in range(nL)]
        for fl, _ in recs:
            out["flags"][d] |= fl
        if out["flags"][d]:
            for k in ("C", "F", "T", "J", "line_out"):
                out[k][d] = np.nan
            continue
        for l, (_, q) in enumerate(recs):
            f, r, K = q["f"], q["r"], q["K"]
            RX, FX = _skew(r), _skew(f)
            KR, RK = K @ RX, RX @ K
            fr = FX @ RX
            out["C"][d, :3, :3] += K
            if seed != "no_coupling":
                out["C"][d, :3, 3:] += -KR
            out["C"][d, 3:, :3] += RK
            out["C"][d, 3:, 3:] += (-(RX @ KR) + fr) if seed == "arm_sign" else (-(RX @ KR) - fr)
            out["F"][d, :3] += f
            out["F"][d, 3:] += np.array([r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]])
            out["T"][d, l], out["T"][d, nL + l] = q["TA"], q["TB"]
            for e, g in ((0, q["gB"] if seed == "ja_from_b" else q["gA"]), (1, q["gB"])):
                out["J"][d, e * nL + l, :3] = g
                out["J"][d, e * nL + l, 3:] = [r[1] * g[2] - r[2] * g[1], r[2] * g[0] - r[0] * g[2], r[0] * g[1] - r[1] * g[0]]
            out["line_out"][d, l] = q["lo"]
    return out
