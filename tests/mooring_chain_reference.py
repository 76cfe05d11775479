"""Independent evaluation of COMPOSITE mooring lines (include/raftx_mooring.h: a head row and its continuation rows, segments
joined at free points that may carry a weight or a buoy) in ``numpy.longdouble``: the reference of
tests/test_mooring_chains.py and tests/test_hip_mooring_chains.py.

Formulation -- MoorPy's, not the device's.  The device shoots: two unknowns (HF, VF) at the fairlead, every segment's span an
explicit function of them.  Here the unknowns are the POSITIONS of the joints in the line's vertical plane.  Every segment is
solved on its own between its two ends with ``mooring_reference.solve_line`` (the single-line solver that
tests/golden/refgold_mooring.npz pins), and the joints are moved by Newton -- the Jacobian assembled from the segments'
own end stiffnesses -- until at every joint

    H(segment above) - H(segment below) = 0        V_bottom(segment above) - V_top(segment below) - W_joint = 0

to stagnation in longdouble.  (The Newton iteration starts from joint positions found by a coarse shooting pass, which only
sets where it starts: the answer is whatever closes the force balance.)  C, F, T, J follow by ANALYTIC differentiation of
that system: the joints' motion for a fairlead displacement from the implicit function theorem, the fairlead stiffness as
the condensed stiffness of the chain, the gradient of every segment-end tension through its own segment's end stiffness.
``fd_check`` compares C and J with central differences of this file's own force function (a full re-solve per perturbed pose).

Envelope: Ek = sum over the lines of (1 + kappa_line) E_line as in tests/mooring_reference.py, with kappa_line the condition
number of the chain's summed catenary Jacobian (the inverse of the condensed fairlead stiffness) scaled by (HF, VF) and
(XF, ZF), and E_line the magnitudes of the closed forms of DESIGN.md section 3.v.

There is NO recorded reference value to pin a composite line against: MoorPy is not available to this test suite and none of
the reference's decks has a composite line.  Independence comes from (1) the different formulation, (2) ``fd_check``, and
(3) the split identity -- a single line cut into rows of equal properties with weightless joints must give the single
line's results, which ties chains to the single-line path that refgold_mooring.npz pins.

Rows: as the device, ``nLine`` counts rows; T and J hold ends A of all rows, then ends B; C and F receive a chain once.
"""
import numpy as np

from . import mooring_reference as mr

ML_N, ML_WJOINT, ML_CONT, MAX_SEG = 16, 10, 15, 4
EPS = mr.EPS
FLAG_BAD_LINE, FLAG_VERTICAL, FLAG_SLACK, FLAG_NO_CONVERGENCE, FLAG_GROUNDED = 1, 2, 4, 8, 64

# Worst multiple of eps Ek of the fp64 model of the device's chain algorithm (tests/mooring_chain_device_model.py) over the
# accuracy cases of tests/mooring_chain_cases.py, measured on the CPU (tests/test_mooring_chains.py prints every case): 4.28
# (a J entry of the chain - rope - chain line just after its anchor-side chain has lifted off the seabed; C of the same
# design 3.90; clump 2.53; every other batch <= 1.97).  GATE_C is the power of two at or above 4 x that.
GATE_WORST_CPU = 4.28
GATE_C = 32


def chains_of(rows):
    """[(first row, number of rows)] of the lines of one design's rows [nRow,16]."""
    out = []
    for i, r in enumerate(rows):
        if r[ML_CONT] != 0:
            if not out:
                raise ValueError("row 0 is a continuation row")
            out[-1][1] += 1
        else:
            out.append([i, 1])
    return [(a, n) for a, n in out]


def chain_flag(rows, pose, depth):
    """The flag of one line (its rows) that needs no solve: BAD_LINE, VERTICAL, SLACK on the total length; or 0."""
    rows = np.asarray(rows, dtype=np.float64)
    head = rows[0]
    if not (np.all(np.isfinite(head[:10])) and np.all(np.isfinite(pose)) and np.all(np.isfinite(rows[1:, 6:11]))):
        return FLAG_BAD_LINE
    if not np.all(rows[:, 6:9] > 0) or head[2] < -depth - 1e-6 * depth:
        return FLAG_BAD_LINE
    Lt = rows[:, 6].sum()
    if not (rows[:, 6] * rows[:, 8]).sum() + rows[1:, ML_WJOINT].sum() > 0:
        return FLAG_BAD_LINE
    p = np.asarray(pose[:3], dtype=np.float64) + np.asarray(mr.rotation(pose[3:], np.float64) @ head[3:6])
    XF, ZF = np.hypot(p[0] - head[0], p[1] - head[1]), p[2] - head[2]
    if not ZF > 0:
        return FLAG_BAD_LINE
    if XF <= 1e-9 * Lt:
        return FLAG_VERTICAL
    if Lt >= XF + ZF:
        return FLAG_SLACK
    return 0


def _segment(X, Z, L, EA, w, seabed):
    """One segment between its ends: dict HF, VF (top), VA (bottom), A, K2, branch, conv."""
    T = np.longdouble
    HF, VF, A, br, it, conv = mr.solve_line(T(X), T(Z), L, EA, w, seabed)
    K2 = np.linalg.inv(A.astype(np.float64)).astype(T)
    K2 = K2 + K2 @ (np.eye(2, dtype=T) - A @ K2)
    K2 = K2 + K2 @ (np.eye(2, dtype=T) - A @ K2)
    VA = T(0) if br else VF - w * L
    return dict(HF=HF, VF=VF, VA=VA, A=A, K2=K2, branch=br, conv=conv, LB=(L - VF / w if br else T(0)))


def _shoot_guess(XF, ZF, L, EA, w, Wj, seabed):
    """Joint positions [(x, z)] relative to the anchor from a coarse shooting pass (a start for ``solve_chain`` only)."""
    T = np.longdouble
    n = len(L)
    Lt, Wt = sum(L), sum(w[i] * L[i] + Wj[i] for i in range(n))
    we = Wt / Lt
    lam = T(0.2) if Lt * Lt <= XF * XF + ZF * ZF else np.sqrt(3 * ((Lt * Lt - ZF * ZF) / (XF * XF) - 1))
    H, V = abs(we * XF / (2 * lam)), we / 2 * (ZF / np.tanh(lam) + Lt)

    def spans(H, V):
        Vt, out, A = V, [None] * n, np.zeros((2, 2), dtype=T)
        for i in range(n - 1, -1, -1):
            if i == 0 and seabed and Vt <= 0:
                X, Z, Ai = L[0] + H * L[0] / EA[0], T(0), np.array([[L[0] / EA[0], 0], [0, 0]], dtype=T)
            else:
                X, Z, Ai, _ = mr.catenary(H, Vt, L[i], EA[i], w[i], seabed and i == 0)
            out[i] = (X, Z)
            A = A + Ai
            Vt = Vt - w[i] * L[i] - Wj[i]
        return out, A

    sp, A = spans(H, V)
    for _ in range(200):
        e = np.array([sum(s[0] for s in sp) - XF, sum(s[1] for s in sp) - ZF], dtype=T)
        if max(abs(e)) <= 1e-12 * Lt:
            break
        d = -np.linalg.solve(A.astype(np.float64), e.astype(np.float64)).astype(T)
        s = T(1)
        while True:
            Ht, Vt = H + s * d[0], V + s * d[1]
            if Ht > 0:
                spt, At = spans(Ht, Vt)
                et = max(abs(sum(q[0] for q in spt) - XF), abs(sum(q[1] for q in spt) - ZF))
                if et < max(abs(e)):
                    break
            s = s / 2
            if s < 2.0 ** -40:
                return None
        H, V, sp, A = Ht, Vt, spt, At
    pts, x, z = [], T(0), T(0)
    for i in range(n - 1):
        x, z = x + sp[i][0], z + sp[i][1]
        pts.append((x, z))
    return pts


def solve_chain(XF, ZF, L, EA, w, Wj, seabed, max_it=60):
    """The chain between the anchor (0, 0) and the fairlead (XF, ZF): (segments, joints y [2(n-1)], R_y, converged).
    Wj[i] is the weight of the point at the lower end of segment i (Wj[0] unused)."""
    T = np.longdouble
    n = len(L)
    if n == 1:
        s = _segment(XF, ZF, L[0], EA[0], w[0], seabed)
        return [s], np.zeros(0, dtype=T), np.zeros((0, 0), dtype=T), bool(s["conv"])
    g = _shoot_guess(XF, ZF, L, EA, w, Wj, seabed)
    if g is None:
        return None, None, None, False
    y = np.array([c for p in g for c in p], dtype=T)

    def system(y):
        P = [(T(0), T(0))] + [(y[2 * j], y[2 * j + 1]) for j in range(n - 1)] + [(XF, ZF)]
        segs = []
        for i in range(n):
            X, Z = P[i + 1][0] - P[i][0], P[i + 1][1] - P[i][1]
            if not X > 0:
                return None, None, None
            s = _segment(X, Z, L[i], EA[i], w[i], seabed and i == 0)
            if not s["conv"]:
                return None, None, None
            segs.append(s)
        R = np.zeros(2 * (n - 1), dtype=T)
        Ry = np.zeros((2 * (n - 1), 2 * (n - 1)), dtype=T)
        for j in range(1, n):                              # joint j: between segment j-1 (below) and segment j (above)
            lo, up = segs[j - 1], segs[j]
            R[2 * (j - 1)] = up["HF"] - lo["HF"]
            R[2 * (j - 1) + 1] = up["VA"] - lo["VF"] - Wj[j]
            # d(H, V_top)/d(X, Z) of a segment is K2; V_bottom = V_top - w L of the (never resting) upper one: the same row
            for seg, sgn, who in ((up, +1, j), (lo, -1, j - 1)):
                # segment `who` spans joints who .. who+1 (joint 0 the anchor, joint n the fairlead): X = x[who+1] - x[who]
                for end, de in ((who + 1, +1), (who, -1)):
                    if 1 <= end <= n - 1:
                        Ry[2 * (j - 1):2 * j, 2 * (end - 1):2 * end] += sgn * de * seg["K2"]
        return segs, R, Ry

    segs, R, Ry = system(y)
    if segs is None:
        return None, None, None, False
    scale = max(abs(sum(w[i] * L[i] for i in range(n))), T(1))
    res, a, conv = max(abs(R)) / scale, T(1), False
    for it in range(max_it):
        if res == 0:
            conv = True
            break
        d = -np.linalg.solve(Ry.astype(np.float64), R.astype(np.float64)).astype(T)
        d = d - np.linalg.solve(Ry.astype(np.float64), (Ry @ d + R).astype(np.float64)).astype(T)      # refined in T
        st, Rt, Ryt = system(y + a * d)
        rt = max(abs(Rt)) / scale if st is not None else np.inf
        if rt < res:
            y, segs, R, Ry, res, a = y + a * d, st, Rt, Ryt, rt, T(1)
        elif res <= 1e-10:
            conv = True                                    # stagnation: the step no longer improves the balance (solve_line's rule)
            break
        else:
            a = a / 2
            if a < 2.0 ** -40:
                break
    return segs, y, Ry, conv


def _inv(M, T=np.longdouble):
    K = np.linalg.inv(M.astype(np.float64)).astype(T)
    I = np.eye(len(M), dtype=T)
    K = K + K @ (I - M @ K)
    return K + K @ (I - M @ K)


def chain_state(rows, pose, depth):
    """Geometry, solved state and derivatives of one (unflagged) line: dict with r, u, XF, HF, VF, K2 (condensed fairlead
    stiffness), kappa, per row Vtop, Vbot, TA, TB and dTA, dTB = d/d(XF, ZF)."""
    T = np.longdouble
    rows = np.asarray(rows, dtype=np.float64).astype(T)
    head = rows[0]
    n = len(rows)
    x = np.asarray(pose, dtype=np.float64).astype(T)
    r = mr.rotation(x[3:], T) @ head[3:6]
    p = x[:3] + r
    dx, dy = p[0] - head[0], p[1] - head[1]
    XF, ZF = np.sqrt(dx * dx + dy * dy), p[2] - head[2]
    seabed = bool(abs(float(head[2]) + depth) <= 1e-6 * depth)
    L, EA, w = list(rows[:, 6]), list(rows[:, 7]), list(rows[:, 8])
    Wj = [T(0)] + list(rows[1:, ML_WJOINT])
    segs, y, Ry, conv = solve_chain(XF, ZF, L, EA, w, Wj, seabed)
    if not conv:
        return dict(conv=False)
    # the joints' motion for a fairlead displacement: R_y dy + R_p dp = 0; only the last joint's equations see the fairlead
    m = 2 * (n - 1)
    dyp = np.zeros((m, 2), dtype=T)
    if n > 1:
        Rp = np.zeros((m, 2), dtype=T)
        Rp[m - 2:m] = segs[-1]["K2"]
        dyp = -_inv(Ry) @ Rp
    dP = [np.zeros((2, 2), dtype=T)] + [dyp[2 * j:2 * j + 2] for j in range(n - 1)] + [np.eye(2, dtype=T)]
    out = dict(conv=True, r=r, u=np.array([dx / XF, dy / XF], dtype=T), XF=XF, ZF=ZF, HF=segs[-1]["HF"], VF=segs[-1]["VF"],
               branch=segs[0]["branch"], LB=segs[0]["LB"], n=n, rows=[], z=[head[2] + (y[2 * j + 1] if j < n - 1 else ZF) for j in range(n)])
    for i, s in enumerate(segs):
        dHV = s["K2"] @ (dP[i + 1] - dP[i])                # d(H, V_top)/d(XF, ZF) of this segment
        H, Vt, Vb = s["HF"], s["VF"], s["VA"]
        TB, TA = np.sqrt(H * H + Vt * Vt), np.sqrt(H * H + Vb * Vb)
        dTB = (H * dHV[0] + Vt * dHV[1]) / TB
        dTA = (H * dHV[0] + (0 if s["branch"] else Vb) * dHV[1]) / TA
        out["rows"].append(dict(H=H, Vtop=Vt, Vbot=Vb, TA=TA, TB=TB, dTA=dTA, dTB=dTB, LB=s["LB"], branch=s["branch"]))
        if i == n - 1:
            out["K2"] = dHV
    A = _inv(out["K2"])
    Sc = np.array([[A[i, j] * (out["HF"], out["VF"])[j] / (XF, ZF)[i] for j in range(2)] for i in range(2)], dtype=np.float64)
    out["kappa"] = float(np.linalg.cond(Sc))
    out["VA"] = segs[0]["VA"]
    # grounded: a joint, or the lowest point of a sagging segment, below the seabed (the device's GROUNDED condition)
    low = []
    for i, s in enumerate(segs):
        zb = head[2] + (y[2 * i - 1] if i > 0 else 0)
        if i > 0:
            low.append(zb)
        if not s["branch"] and s["VA"] < 0 < s["VF"]:
            vb = s["VA"] / s["HF"]
            low.append(zb - (s["HF"] / w[i] * (np.sqrt(1 + vb * vb) - 1) + s["VA"] ** 2 / (2 * EA[i] * w[i])))
    out["grounded"] = bool(low and min(low) < -depth - 1e-6 * depth) or bool(seabed and n > 1 and segs[0]["VF"] <= 0)
    return out


def evaluate(lines, pose, depth):
    """dict of C [nD,6,6], F [nD,6], T [nD,2nRow], J [nD,2nRow,6], line_out [nD,nRow,8], flags [nD], kappa [nD,nRow] and the
    envelopes EC, EF, ET, EJ (kappa folded in) of designs of rows [nD,nRow,16].  Flagged designs are NaN."""
    T = np.longdouble
    lines = np.asarray(lines, dtype=np.float64)
    nD, nL = lines.shape[:2]
    pose = np.zeros((nD, 6)) if pose is None else np.asarray(pose, dtype=np.float64).reshape(nD, 6)
    out = dict(C=np.zeros((nD, 6, 6), dtype=T), F=np.zeros((nD, 6), dtype=T), T=np.zeros((nD, 2 * nL), dtype=T),
               J=np.zeros((nD, 2 * nL, 6), dtype=T), line_out=np.zeros((nD, nL, 8), dtype=T),
               flags=np.zeros(nD, dtype=np.int32), kappa=np.zeros((nD, nL)))
    for k in ("C", "F", "T", "J"):
        out["E" + k] = np.zeros_like(out[k])
    for d in range(nD):
        groups = chains_of(lines[d])
        for a, n in groups:
            if n > MAX_SEG:
                raise ValueError("a line of %d rows" % n)
            out["flags"][d] |= chain_flag(lines[d, a:a + n], pose[d], depth)
        if out["flags"][d]:
            continue
        for a, n in groups:
            s = chain_state(lines[d, a:a + n], pose[d], depth)
            if not s["conv"]:
                out["flags"][d] |= FLAG_NO_CONVERGENCE
                break
            if s["grounded"]:
                out["flags"][d] |= FLAG_GROUNDED
                break
            q = mr.line_terms(dict(HF=s["HF"], VF=s["VF"], VA=s["VA"], XF=s["XF"], u=s["u"], K2=s["K2"]), T)
            k1 = 1 + T(s["kappa"])
            r, f, K3, u = s["r"], q["f"], q["K3"], s["u"]
            RX, FX = mr.skew(r, T), mr.skew(f, T)
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
            K2 = s["K2"]
            for i, row in enumerate(s["rows"]):
                for e, nm, Vx in ((0, "A", 0 if row["branch"] else row["Vbot"]), (1, "B", row["Vtop"])):
                    k = e * nL + a + i
                    dT_, Tx = row["dT" + nm], row["T" + nm]
                    g3 = np.array([dT_[0] * u[0], dT_[0] * u[1], dT_[1]], dtype=T)
                    eX = (abs(s["HF"] * K2[0, 0]) + abs(Vx * K2[1, 0])) / Tx
                    eZ = (abs(s["HF"] * K2[0, 1]) + abs(Vx * K2[1, 1])) / Tx
                    Eg = np.array([eX * abs(u[0]), eX * abs(u[1]), eZ], dtype=T)
                    out["T"][d, k], out["ET"][d, k] = Tx, k1 * Tx
                    out["J"][d, k, :3], out["J"][d, k, 3:] = g3, RX @ g3
                    out["EJ"][d, k, :3], out["EJ"][d, k, 3:] = k1 * Eg, k1 * (aRX @ Eg)
                out["line_out"][d, a + i] = [row["H"], row["Vtop"], row["H"], row["Vbot"], row["LB"], 0, row["branch"], 0]
                out["kappa"][d, a + i] = s["kappa"]
    bad = out["flags"] != 0
    for k in ("C", "F", "T", "J", "line_out"):
        out[k][bad] = np.nan
    return out


def _forces_perturbed(rows, R, x, dx6, depth):
    """One line's (f, r x f) and its rows' (TA, TB) with the unit displaced by dx6[:3] and turned by the rotation vector
    dx6[3:] on top of R (mooring_reference.forces_perturbed for a chain): a full re-solve."""
    T = np.longdouble
    rows = np.asarray(rows, dtype=np.float64).astype(T)
    head = rows[0]
    TX = mr.skew(np.asarray(dx6[3:], dtype=T), T)
    r = (np.eye(3, dtype=T) + TX + TX @ TX / 2) @ (R @ head[3:6])
    p = x + np.asarray(dx6[:3], dtype=T) + r
    ddx, ddy = p[0] - head[0], p[1] - head[1]
    XF, ZF = np.sqrt(ddx * ddx + ddy * ddy), p[2] - head[2]
    seabed = bool(abs(float(head[2]) + depth) <= 1e-6 * depth)
    segs, y, Ry, conv = solve_chain(XF, ZF, list(rows[:, 6]), list(rows[:, 7]), list(rows[:, 8]), [T(0)] + list(rows[1:, ML_WJOINT]), seabed)
    assert conv
    HF, VF = segs[-1]["HF"], segs[-1]["VF"]
    f = np.array([-HF * ddx / XF, -HF * ddy / XF, -VF], dtype=T)
    TA = [np.sqrt(s["HF"] ** 2 + s["VA"] ** 2) for s in segs]
    TB = [np.sqrt(s["HF"] ** 2 + s["VF"] ** 2) for s in segs]
    return np.concatenate([f, np.cross(r, f)]), TA, TB


def fd_check(lines_d, pose_d, depth, h=1e-4):
    """Worst |analytic - central difference| / envelope of C and J of one design (see mooring_reference.fd_check)."""
    T = np.longdouble
    lines_d = np.asarray(lines_d, dtype=np.float64)
    nL = len(lines_d)
    ref = evaluate(lines_d[None], np.asarray(pose_d, dtype=np.float64)[None], depth)
    assert ref["flags"][0] == 0
    x = np.asarray(pose_d, dtype=np.float64).astype(T)
    R = mr.rotation(x[3:], T)
    Cfd, Jfd = np.zeros((6, 6), dtype=T), np.zeros((2 * nL, 6), dtype=T)
    for j in range(6):
        d6 = np.zeros(6, dtype=T)
        d6[j] = T(h)
        for a, n in chains_of(lines_d):
            Fp, TAp, TBp = _forces_perturbed(lines_d[a:a + n], R, x[:3], d6, depth)
            Fm, TAm, TBm = _forces_perturbed(lines_d[a:a + n], R, x[:3], -d6, depth)
            Cfd[:, j] -= (Fp - Fm) / (2 * T(h))
            for i in range(n):
                Jfd[a + i, j] = (TAp[i] - TAm[i]) / (2 * T(h))
                Jfd[nL + a + i, j] = (TBp[i] - TBm[i]) / (2 * T(h))
    eC = np.abs(ref["C"][0] - Cfd) / np.maximum(ref["EC"][0], np.finfo(np.float64).tiny)
    eJ = np.abs(ref["J"][0] - Jfd) / np.maximum(ref["EJ"][0], np.finfo(np.float64).tiny)
    return float(eC.max()), float(eJ.max())


gate_multiples = mr.gate_multiples
