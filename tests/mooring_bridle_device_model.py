"""fp64 NumPy restatement of the device's algorithm for BRIDLES (moor_shoot / moor_bridle_record of
raft_amd/csrc/raftx_mooring.h, then k_moor_design<true>): the junction P as the unknown of a damped Newton iteration, the
stem shot in the vertical plane through the anchor and P, every leg a suspended catenary in its own plane, the same start,
acceptance rule and condensation.  It is what the bridle gate's constant of tests/mooring_bridle_reference.py is measured
with on the CPU, and -- through ``seed`` -- the carrier of the deliberate errors the gate must reject
(tests/test_mooring_bridles.py).  Rows that belong to no bridle go through tests/mooring_chain_device_model.py unchanged.
The kernels contract multiply-adds and use the device's asinh / tanh: agreement to rounding, not to the bit.
"""
import numpy as np

from . import mooring_chain_device_model as cdm
from . import mooring_device_model as dm

MAX_IT, TIGHT, BR_MAX_IT, GROW, MAX_SEG, MAX_LEG = 60, 1e-10, 60, 1e3, 4, 3
ML_WJOINT, ML_LEG, ML_CONT = 10, 14, 15
GROUNDED = 64
SEEDS = ("junction_weight_dropped", "no_junction_coupling", "leg_missing_from_kpp", "arm_turning_second_dropped")


def _shoot(kind, L, EA, w, Wj, seabed, Lt, we, XF, ZF, top=None):
    """(conv, H, V, a11, a12, a22, contact, Vtop) of one element between ends XF, ZF apart: moor_shoot.  kind 0: the chain
    L, EA, w, Wj; 1: one suspended segment; 2: the chain with the suspended segment top = (L, EA, w, weight of the point at
    its lower end) above it."""
    def ev(H, V):
        if kind == 1:
            X, Z, a11, a12, a22, ct = dm._eval(H, V, L[0], EA[0], w[0], False, None)
            return X, Z, a11, a12, a22, ct, [V]
        if kind == 2:
            t = dm._eval(H, V, top[0], top[1], top[2], False, None)
            c = cdm._chain_eval(H, (V - top[2] * top[0]) - top[3], L, EA, w, Wj, seabed, None)
            return (t[0] + c[0], t[1] + c[1], t[2] + c[2], t[3] + c[3], t[4] + c[4], c[5], c[6])
        return cdm._chain_eval(H, V, L, EA, w, Wj, seabed, None)

    conv, H, V, _, cur = dm.newton(ev, Lt, we, XF, ZF)
    return (conv, H, V) + tuple(cur[2:])


def bridle(rows, ns, ps, depth, seed=None):
    """(flag, dict) of one bridle: rows [ns + nleg, 16], the first ns its stem.  dict: C [6,6], F [6], T [n,2] (A, B),
    J [n,2,6], lo [n,8], P."""
    rows = np.asarray(rows, dtype=np.float64)
    ps = np.asarray(ps, dtype=np.float64)
    rec, stem, legs = rows[0], rows[:ns], rows[ns:]
    nleg = len(legs)
    L, EA, w = list(stem[:, 6]), list(stem[:, 7]), list(stem[:, 8])
    Wjs = [0.0] + list(stem[1:, ML_WJOINT])
    fin = (np.all(np.isfinite(rec[:10])) and np.all(np.isfinite(ps)) and np.all(np.isfinite(stem[1:, 6:11]))
           and np.all(np.isfinite(legs[:, 3:11])))
    Ls, Ws = L[0], w[0] * L[0]
    for i in range(1, ns):
        Ls += L[i]
        Ws += w[i] * L[i] + Wjs[i]
    az = rec[2]
    if not fin or not np.all(rows[:, 6:9] > 0) or not Ws > 0.0 or az < -depth - 1e-6 * depth:
        return 1, None
    Wj = 0.0 if seed == "junction_weight_dropped" else legs[0, ML_WJOINT]
    Wl = Lm = 0.0
    for i in range(nleg):
        Wl += legs[i, 8] * legs[i, 6]
        Lm += legs[i, 6]
    Lm = Lm / nleg
    Wt = Ws + Wl
    if not Wt + Wj > 0.0:
        return 1, None
    rl = [dm._arm(legs[i, 3:6], ps[3:]) for i in range(nleg)]
    pf = [ps[:3] + rl[i] for i in range(nleg)]
    slack = True
    for i in range(nleg):
        XFi, ZFi = np.sqrt((pf[i][0] - rec[0]) ** 2 + (pf[i][1] - rec[1]) ** 2), pf[i][2] - az
        if not ZFi > 0:
            return 1, None
        slack = slack and Ls + legs[i, 6] >= XFi + ZFi
    if slack:
        return 4, None
    seabed = abs(az + depth) <= 1e-6 * depth
    wes = Ws / Ls

    def at(Pt):
        dx, dy, ZF = Pt[0] - rec[0], Pt[1] - rec[1], Pt[2] - az
        XF = np.sqrt(dx * dx + dy * dy)
        if not (XF > 1e-9 * Ls and (not seabed or (ZF > 0.0 and Ls < XF + ZF))):
            return None
        s = _shoot(0, L, EA, w, Wjs, seabed, Ls, wes, XF, ZF)
        if not s[0]:
            return None
        S = dm.end(s[1], s[2], s[3], s[4], s[5], dx / XF, dy / XF, XF)
        S["contact"], S["Vtop"] = s[6], s[7]
        R = np.array([-S["H"] * S["ux"], -S["H"] * S["uy"], -S["V"] - Wj])
        K = S["K"].copy()
        G = []
        for i in range(nleg):
            dx, dy, ZF = pf[i][0] - Pt[0], pf[i][1] - Pt[1], pf[i][2] - Pt[2]
            XF = np.sqrt(dx * dx + dy * dy)
            if not XF > 1e-9 * legs[i, 6]:
                return None
            s = _shoot(1, [legs[i, 6]], [legs[i, 7]], [legs[i, 8]], [0.0], False, legs[i, 6], legs[i, 8], XF, ZF)
            if not s[0]:
                return None
            g = dm.end(s[1], s[2], s[3], s[4], s[5], dx / XF, dy / XF, XF)
            R = R + np.array([g["H"] * g["ux"], g["H"] * g["uy"], g["V"] - legs[i, 8] * legs[i, 6]])
            if not (seed == "leg_missing_from_kpp" and i == nleg - 1):
                K = K + g["K"]
            G.append(g)
        return S, G, R, K

    # the start: the stem with ONE equivalent leg above it (the legs' summed EA and weight, their mean length along the axis)
    # to the centroid of the fairleads, shot as a composite line; the junction is that leg's span below the centroid.  Where
    # this plane problem has no solution: on the straight line from the anchor to the centroid.
    cf = np.zeros(3)
    for i in range(nleg):
        cf = cf + pf[i]
    cf = cf / nleg
    Le = EAe = 0.0
    for i in range(nleg):
        o2 = (pf[i][0] - cf[0]) ** 2 + (pf[i][1] - cf[1]) ** 2 + (pf[i][2] - cf[2]) ** 2
        Li = legs[i, 6]
        Le += np.sqrt(max(Li * Li - o2, 0.25 * Li * Li))
        EAe += legs[i, 7]
    Le = Le / nleg
    dxc, dyc, ZFc = cf[0] - rec[0], cf[1] - rec[1], cf[2] - az
    XFc = np.sqrt(dxc * dxc + dyc * dyc)
    Pt = rec[:3] + (Ls / (Ls + Le)) * (cf - rec[:3])
    if XFc > 1e-9 * (Ls + Le) and (not seabed or Ls + Le < XFc + ZFc):
        top = (Le, EAe, Wl / Le, Wj)
        s0 = _shoot(2, L, EA, w, Wjs, seabed, Ls + Le, (Wt + Wj) / (Ls + Le), XFc, ZFc, top)
        if s0[0]:
            t = dm._eval(s0[1], s0[2], top[0], top[1], top[2], False, None)
            Pt = np.array([cf[0] - t[0] * (dxc / XFc), cf[1] - t[0] * (dyc / XFc), cf[2] - t[1]])
    have, conv, up, it, a = False, False, False, 0, 1.0
    while True:
        st = at(Pt)
        rt = max(abs(st[2])) / Wt if st is not None else 0.0
        take = False
        if not have:
            if st is None:
                break
            take = True
        elif st is not None and rt < res:
            take, up = True, False
        elif res <= TIGHT:
            conv = True
            break
        elif st is not None and not up and a == 1.0 and rt <= GROW * res:
            take, up = True, True                          # a full step from the soft side lands on the stiff side: Newton's way in
        else:
            a *= 0.5
            if a < 2.0 ** -40:
                break
        if take:
            have, P, res, a = True, Pt, rt, 1.0
            S, G, R, K = st
            Ki = np.linalg.inv(K)
            d = Ki @ R
            if res == 0.0:
                conv = True
                break
        if it >= BR_MAX_IT:
            break
        it += 1
        Pt = P + a * d
    if not conv:
        return 8, None
    floor = -depth - 1e-6 * depth
    flag = 0
    if cdm.grounded(S["H"], S["Vtop"], S["contact"], L, EA, w, seabed, az, depth) or P[2] < floor:
        flag = GROUNDED
    for i in range(nleg):
        Vb = G[i]["V"] - legs[i, 8] * legs[i, 6]
        if Vb < 0.0 and G[i]["V"] > 0.0 and P[2] - cdm.sag_drop(G[i]["H"], Vb, legs[i, 7], legs[i, 8]) < floor:
            flag = GROUNDED
    if flag:
        return flag, dict(P=P)                             # (the junction, for who wants to look: the records are not written)
    D = [Ki @ G[j]["K"] for j in range(nleg)]
    B = [np.hstack([np.eye(3), -dm._skew(rl[j])]) for j in range(nleg)]
    DP = np.zeros((3, 6))
    for j in range(nleg):
        DP = DP + D[j] @ B[j]
    C, F = np.zeros((6, 6)), np.zeros(6)
    for i in range(nleg):
        g = G[i]
        f = np.array([-g["H"] * g["ux"], -g["H"] * g["uy"], -g["V"]])
        RI = dm._skew(rl[i])
        for j in range(nleg):
            M = (g["K"] if i == j else np.zeros((3, 3)))
            if seed != "no_junction_coupling":
                M = M - g["K"] @ D[j]
            RJ = dm._skew(rl[j])
            C[:3, :3] += M
            C[:3, 3:] += -(M @ RJ)
            C[3:, :3] += RI @ M
            C[3:, 3:] += -(RI @ (M @ RJ))
        if not (seed == "arm_turning_second_dropped" and i == 1):
            C[3:, 3:] += -(dm._skew(f) @ RI)
        F[:3] += f
        F[3:] += np.cross(rl[i], f)
    n = ns + nleg
    T, J, lo = np.zeros((n, 2)), np.zeros((n, 2, 6)), np.zeros((n, 8))
    for i in range(ns):
        ct = i == 0 and S["contact"]
        VB = S["Vtop"][i]
        VA = 0.0 if ct else VB - w[i] * L[i]
        for e, Vx in ((0, VA), (1, VB)):
            Tx = np.sqrt(S["H"] ** 2 + Vx * Vx)
            T[i, e] = Tx
            J[i, e] = dm.end_grad(S, Vx, Tx) @ DP
        lo[i] = [S["H"], VB, S["H"], VA, L[0] - VB / w[0] if ct else 0.0, it, 1.0 if ct else 0.0, 0.0]
    for i in range(nleg):
        g = G[i]
        VB = g["V"]
        VA = VB - legs[i, 8] * legs[i, 6]
        for e, Vx in ((0, VA), (1, VB)):
            Tx = np.sqrt(g["H"] ** 2 + Vx * Vx)
            T[ns + i, e] = Tx
            J[ns + i, e] = dm.end_grad(g, Vx, Tx) @ (B[i] - DP)
        lo[ns + i] = [g["H"], VB, g["H"], VA, 0.0, it, 0.0, 0.0]
    return 0, dict(C=C, F=F, T=T, J=J, lo=lo, P=P)


def groups_of(rows):
    """[(first row, stem rows, leg rows)] of one design's rows: single lines and chains have 0 leg rows."""
    out, l, nL = [], 0, len(rows)
    while l < nL:
        ns = 1
        while l + ns < nL and ns < MAX_SEG and rows[l + ns, ML_CONT] != 0:
            ns += 1
        nleg = 0
        while l + ns + nleg < nL and nleg < MAX_LEG and rows[l + ns + nleg, ML_LEG] != 0:
            nleg += 1
        out.append((l, ns, nleg))
        l += ns + nleg
    return out


def evaluate(lines, pose, depth, seed=None):
    """dict C [nD,6,6], F [nD,6], T [nD,2nRow], J [nD,2nRow,6], line_out [nD,nRow,8], flags [nD] as raftx_mooring_lines."""
    assert seed is None or seed in SEEDS
    lines = np.asarray(lines, dtype=np.float64)
    nD, nL = lines.shape[:2]
    pose = np.zeros((nD, 6)) if pose is None else np.asarray(pose, dtype=np.float64).reshape(nD, 6)
    out = dict(C=np.zeros((nD, 6, 6)), F=np.zeros((nD, 6)), T=np.zeros((nD, 2 * nL)), J=np.zeros((nD, 2 * nL, 6)),
               line_out=np.full((nD, nL, 8), np.nan), flags=np.zeros(nD, dtype=np.int32))
    for d in range(nD):
        parts = []
        for l, ns, nleg in groups_of(lines[d]):
            if nleg:
                fl, q = bridle(lines[d, l:l + ns + nleg], ns, pose[d], depth, seed)
            else:
                q = cdm.evaluate(lines[d:d + 1, l:l + ns], pose[d:d + 1], depth)
                fl = int(q["flags"][0])
                if not fl:
                    q = dict(C=q["C"][0], F=q["F"][0], T=np.stack([q["T"][0, :ns], q["T"][0, ns:]], axis=1),
                             J=np.stack([q["J"][0, :ns], q["J"][0, ns:]], axis=1), lo=q["line_out"][0])
            out["flags"][d] |= fl
            parts.append((l, ns + nleg, q))
        if out["flags"][d]:
            for k in ("C", "F", "T", "J", "line_out"):
                out[k][d] = np.nan
            continue
        for l, n, q in parts:
            out["C"][d] += q["C"]
            out["F"][d] += q["F"]
            out["T"][d, l:l + n], out["T"][d, nL + l:nL + l + n] = q["T"][:, 0], q["T"][:, 1]
            out["J"][d, l:l + n], out["J"][d, nL + l:nL + l + n] = q["J"][:, 0], q["J"][:, 1]
            out["line_out"][d, l:l + n] = q["lo"]
    return out
