"""fp64 NumPy restatement of the device's algorithm for composite mooring lines (moor_chain_eval / moor_chain_record of
raft_amd/csrc/raftx_mooring.h, then k_moor_design): the same expressions in the same order.  It is what the chain gate's
constant of tests/mooring_chain_reference.py is measured with on the CPU, and -- through ``seed`` -- the carrier of the
deliberate errors the gate must reject (tests/test_mooring_chains.py).  Single rows go through tests/mooring_device_model.py
unchanged.  The kernels contract multiply-adds and use the device's asinh / tanh: agreement to rounding, not to the bit.
"""
import numpy as np

from . import mooring_device_model as dm

MAX_IT, TIGHT, MAX_SEG = 60, 1e-10, 4
ML_WJOINT, ML_CONT = 10, 15
GROUNDED = 64
SEEDS = ("joint_dropped", "segment_no_stretch", "gradient_wrong_end", "rows_fairlead_first")


def _chain_eval(H, V, L, EA, w, Wj, seabed, seed):
    n = len(L)
    X = Z = a11 = a12 = a22 = 0.0
    contact, Vt, Vtop = 0, V, [0.0] * n
    for i in range(n - 1, -1, -1):
        Vtop[i] = Vt
        if i == 0 and seabed and Vt <= 0.0:
            X += L[0] + H * L[0] / EA[0]
            a11 += L[0] / EA[0]
            contact = 1
        else:
            s = dm._eval(H, Vt, L[i], EA[i], w[i], seabed and i == 0, "no_stretch" if seed == "segment_no_stretch" and i == n - 2 else None)
            X += s[0]; Z += s[1]; a11 += s[2]; a12 += s[3]; a22 += s[4]
            if i == 0:
                contact = s[5]
        Vt = (Vt - w[i] * L[i]) - (0.0 if seed == "joint_dropped" else Wj[i])
    return X, Z, a11, a12, a22, contact, Vtop


def sag_drop(H, Vb, EA, w):
    """How far a segment sags below its lower end, where the vertical force is Vb < 0 (moor_sag_drop)."""
    vb = Vb / H
    sb = np.sqrt(1.0 + vb * vb)
    return (H / w) * (vb * vb / (sb + 1.0)) + Vb * Vb / (2.0 * EA * w)


def grounded(H, Vtop, ct, L, EA, w, seabed, az, depth):
    """The solved chain against the seabed (moor_chain_grounded): the anchor-side segment rests wholly, or a joint or a sag
    (where V changes sign inside a segment) lies below the floor, from the anchor up."""
    if seabed and Vtop[0] <= 0.0:
        return True
    floor, z, n = -depth - 1e-6 * depth, az, len(L)
    for i in range(n):
        Vb = Vtop[i] - w[i] * L[i]
        if not (i == 0 and ct) and Vb < 0.0 and Vtop[i] > 0.0 and z - sag_drop(H, Vb, EA[i], w[i]) < floor:
            return True
        z += dm._eval(H, Vtop[i], L[i], EA[i], w[i], seabed and i == 0, None)[1]
        if i + 1 < n and z < floor:
            return True
    return False


def chain(rows, ps, depth, seed=None):
    """(flag, [record per row]) of one composite line: what the head row's lane writes."""
    rows = np.asarray(rows, dtype=np.float64)
    ps = np.asarray(ps, dtype=np.float64)
    rec, n = rows[0], len(rows)
    L, EA, w = list(rows[:, 6]), list(rows[:, 7]), list(rows[:, 8])
    Wj = [0.0] + list(rows[1:, ML_WJOINT])
    fin = np.all(np.isfinite(rec[:10])) and np.all(np.isfinite(ps)) and np.all(np.isfinite(rows[1:, 6:11]))
    Lt, Wt = L[0], w[0] * L[0]
    for i in range(1, n):
        Lt += L[i]
        Wt += w[i] * L[i] + Wj[i]
    az = rec[2]
    if not fin or not np.all(rows[:, 6:9] > 0) or not Wt > 0.0 or az < -depth - 1e-6 * depth:
        return 1, None
    r = dm._arm(rec[3:6], ps[3:])
    dx, dy = (ps[0] + r[0]) - rec[0], (ps[1] + r[1]) - rec[1]
    XF = np.sqrt(dx * dx + dy * dy)
    ZF = (ps[2] + r[2]) - az
    if not ZF > 0:
        return 1, None
    if XF <= 1e-9 * Lt:
        return 2, None
    if Lt >= XF + ZF:
        return 4, None
    ux, uy = dx / XF, dy / XF
    seabed = abs(az + depth) <= 1e-6 * depth
    we = Wt / Lt
    conv, H, V, it, (_, _, a11, a12, a22, ct, Vtop) = dm.newton(lambda H, V: _chain_eval(H, V, L, EA, w, Wj, seabed, seed), Lt, we, XF, ZF)
    if not conv:
        return 8, None
    if grounded(H, Vtop, ct, L, EA, w, seabed, az, depth):
        return GROUNDED, None
    m = dm.end(H, V, a11, a12, a22, ux, uy, XF)
    out = []
    for i in range(n):
        c = i == 0 and ct
        VB = Vtop[i]
        VA = 0.0 if c else VB - w[i] * L[i]
        TB, TA = np.sqrt(H * H + VB * VB), np.sqrt(H * H + VA * VA)
        VgA = VB if seed == "gradient_wrong_end" else VA
        out.append(dict(f=np.array([-H * ux, -H * uy, -V]) if i == 0 else np.zeros(3), r=r, K=m["K"] if i == 0 else np.zeros((3, 3)),
                        gA=dm.end_grad(m, VgA, TA), gB=dm.end_grad(m, VB, TB), TA=TA, TB=TB,
                        lo=np.array([H, VB, H, VA, L[0] - VB / w[0] if c else 0.0, it, 1.0 if c else 0.0, 0.0])))
    return 0, out


def evaluate(lines, pose, depth, seed=None):
    """dict C [nD,6,6], F [nD,6], T [nD,2nRow], J [nD,2nRow,6], line_out [nD,nRow,8], flags [nD] as raftx_mooring_lines."""
    assert seed is None or seed in SEEDS
    lines = np.asarray(lines, dtype=np.float64)
    nD, nL = lines.shape[:2]
    pose = np.zeros((nD, 6)) if pose is None else np.asarray(pose, dtype=np.float64).reshape(nD, 6)
    out = dict(C=np.zeros((nD, 6, 6)), F=np.zeros((nD, 6)), T=np.zeros((nD, 2 * nL)), J=np.zeros((nD, 2 * nL, 6)),
               line_out=np.full((nD, nL, 8), np.nan), flags=np.zeros(nD, dtype=np.int32))
    for d in range(nD):
        recs, l = [], 0
        while l < nL:
            n = 1
            while l + n < nL and n < MAX_SEG and lines[d, l + n, ML_CONT] != 0:
                n += 1
            if n == 1:
                fl, q = dm.line(lines[d, l], pose[d], depth)
                q = [q]
            else:
                fl, q = chain(lines[d, l:l + n], pose[d], depth, seed)
                if seed == "rows_fairlead_first" and not fl:
                    q = [dict(q[n - 1 - i], f=q[i]["f"], K=q[i]["K"]) for i in range(n)]
            out["flags"][d] |= fl
            recs += q if not fl else [None] * n
            l += n
        if out["flags"][d]:
            for k in ("C", "F", "T", "J", "line_out"):
                out[k][d] = np.nan
            continue
        for l, q in enumerate(recs):
            f, r, K = q["f"], q["r"], q["K"]
            RX, FX = dm._skew(r), dm._skew(f)
            KR, RK = K @ RX, RX @ K
            out["C"][d, :3, :3] += K
            out["C"][d, :3, 3:] += -KR
            out["C"][d, 3:, :3] += RK
            out["C"][d, 3:, 3:] += -(RX @ KR) - FX @ RX
            out["F"][d, :3] += f
            out["F"][d, 3:] += np.array([r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]])
            out["T"][d, l], out["T"][d, nL + l] = q["TA"], q["TB"]
            for e, g in ((0, q["gA"]), (1, q["gB"])):
                out["J"][d, e * nL + l, :3] = g
                out["J"][d, e * nL + l, 3:] = [r[1] * g[2] - r[2] * g[1], r[2] * g[0] - r[0] * g[2], r[0] * g[1] - r[1] * g[0]]
            out["line_out"][d, l] = q["lo"]
    return out
