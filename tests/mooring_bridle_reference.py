"""Independent evaluation of BRIDLES (include/raftx_mooring.h: stem rows anchor -> junction, then leg rows junction ->
fairlead) in ``numpy.longdouble``: the reference of tests/test_mooring_bridles.py and tests/test_hip_mooring_bridles.py.

Formulation -- MoorPy's, not the device's.  The device has three unknowns, the junction, and shoots the whole stem in one
vertical plane.  Here EVERY free point -- the junction and every joint of the stem -- is a point with three unknown
coordinates; every segment is solved on its own between its two ends with ``mooring_reference.solve_line`` (the single-line
solver that tests/golden/refgold_mooring.npz pins), and the points are moved by Newton on the assembled point stiffness
(3 x 3 end stiffness of every segment, in global axes) until the net force on every free point -- segment ends and the
point's weight -- vanishes, to stagnation in longdouble.  (The iteration starts from the fp64 model's junction and a plane
solve of the stem's joints, which only sets where it starts: the answer is whatever closes this file's own force balance.)
C, F, T, J follow by ANALYTIC differentiation of that system: the points' motion for a fairlead displacement from the
implicit function theorem, the fairlead stiffness blocks K_ij as the stiffness condensed to the fairleads, the gradient of
every segment-end tension through its own segment's end stiffness and the motion of its two ends.  ``fd_check`` compares C
and J with central differences of this file's own force function (a full re-solve per perturbed pose).

Envelope: Ek = (1 + kappa) E with E the magnitudes of the closed forms (sums of absolute values of every product that
enters), as in tests/mooring_chain_reference.py, and kappa = (largest condition number of an element's scaled catenary
Jacobian) + cond_2(K_PP), K_PP the point stiffness condensed to the junction: a rounding error of the force balance moves
the junction by K_PP^-1 times it, and the junction's motion enters every output.

There is NO recorded reference value to pin a bridle against: MoorPy is not available to this test suite and none of the
reference's decks has a bridle.  Independence comes from (1) the different formulation, (2) ``fd_check``, (3) the
coincident-legs identity -- two legs to one fairlead, each with half the EA and w, are the composite line with one last
segment of the whole, which ties bridles to the chain path and through it to refgold_mooring.npz -- and (4) the mirror identity.

Rows without a leg mark go through tests/mooring_chain_reference.py unchanged.
"""
import numpy as np

from . import mooring_bridle_device_model as bdm
from . import mooring_chain_reference as mcr
from . import mooring_reference as mr

ML_N, ML_WJOINT, ML_LEG, ML_CONT, MAX_SEG, MAX_LEG = 16, 10, 14, 15, 4, 3
EPS = mr.EPS
FLAG_BAD_LINE, FLAG_VERTICAL, FLAG_SLACK, FLAG_NO_CONVERGENCE, FLAG_GROUNDED = 1, 2, 4, 8, 64

# Worst multiple of eps Ek of the fp64 model of the device's bridle algorithm (tests/mooring_bridle_device_model.py) over the
# accuracy cases of tests/mooring_bridle_cases.py, measured on the CPU (tests/test_mooring_bridles.py prints every case): 1.79
# (the tension of the taut leg of symmetric_200 at the yawed offset; F of the same design 1.45; clump 1.26; every other case
# below 1).  C and J stay below 0.02: their envelope carries cond(K_PP) on every term, the tensions' does too but has one term.
# GATE_C is the power of two at or above 4 x that.
GATE_WORST_CPU = 1.79
GATE_C = 8

T_ = np.longdouble


def _inv(M):
    K = np.linalg.inv(M.astype(np.float64)).astype(T_)
    I = np.eye(len(M), dtype=T_)
    K = K + K @ (I - M @ K)
    return K + K @ (I - M @ K)


def bridle_flag(rows, ns, pose, depth):
    """The flag of one bridle that needs no solve: BAD_LINE or SLACK; or 0."""
    rows = np.asarray(rows, dtype=np.float64)
    head, stem, legs = rows[0], rows[:ns], rows[ns:]
    if not (np.all(np.isfinite(head[:10])) and np.all(np.isfinite(pose)) and np.all(np.isfinite(stem[1:, 6:11]))
            and np.all(np.isfinite(legs[:, 3:11]))):
        return FLAG_BAD_LINE
    if not np.all(rows[:, 6:9] > 0) or head[2] < -depth - 1e-6 * depth:
        return FLAG_BAD_LINE
    Ws = (stem[:, 6] * stem[:, 8]).sum() + stem[1:, ML_WJOINT].sum()
    if not Ws > 0 or not Ws + (legs[:, 6] * legs[:, 8]).sum() + legs[0, ML_WJOINT] > 0:
        return FLAG_BAD_LINE
    R = np.asarray(mr.rotation(pose[3:], np.float64))
    slack = True
    for lg in legs:
        p = np.asarray(pose[:3], dtype=np.float64) + R @ lg[3:6]
        XF, ZF = np.hypot(p[0] - head[0], p[1] - head[1]), p[2] - head[2]
        if not ZF > 0:
            return FLAG_BAD_LINE
        slack = slack and stem[:, 6].sum() + lg[6] >= XF + ZF
    return FLAG_SLACK if slack else 0


def _segment3(A, B, L, EA, w, seabed):
    """One segment between the points A (lower) and B: forces on its ends, end stiffness, tensions and their gradients for a
    displacement of B relative to A, the envelopes of each.  None where it has no solution."""
    d = B - A
    XF, ZF = np.sqrt(d[0] * d[0] + d[1] * d[1]), d[2]
    if not XF > 1e-9 * L or (seabed and L >= XF + ZF):
        return None
    HF, VF, Aj, br, it, conv = mr.solve_line(T_(XF), T_(ZF), L, EA, w, seabed)
    if not conv:
        return None
    K2 = _inv(Aj)
    VA = T_(0) if br else VF - w * L
    u = np.array([d[0] / XF, d[1] / XF], dtype=T_)
    q = mr.line_terms(dict(HF=HF, VF=VF, VA=VA, XF=XF, u=u, K2=K2), T_)
    Sc = np.array([[Aj[i, j] * (HF, VF)[j] / (XF, abs(ZF) + XF * 1e-300)[i] for j in range(2)] for i in range(2)], dtype=np.float64)
    q.update(HF=HF, VF=VF, VA=VA, branch=br, LB=(L - VF / w if br else T_(0)), fA=np.array([HF * u[0], HF * u[1], VA], dtype=T_),
             kappa=float(np.linalg.cond(Sc)), w=w, EA=EA, zA=A[2])
    return q


class _System:
    """The points and segments of one bridle at given fairlead positions."""

    def __init__(self, rows, ns, depth):
        rows = np.asarray(rows, dtype=np.float64).astype(T_)
        self.rows, self.ns, self.nleg, self.depth = rows, ns, len(rows) - ns, depth
        self.anchor = rows[0, 0:3].copy()
        self.seabed = bool(abs(float(rows[0, 2]) + depth) <= 1e-6 * depth)
        self.m = ns                                              # free points: ns - 1 stem joints, then the junction
        self.weight = [rows[i + 1, ML_WJOINT] for i in range(ns - 1)] + [rows[ns, ML_WJOINT]]

    def segments(self, u, fair):
        pts = [self.anchor] + [u[3 * k:3 * k + 3] for k in range(self.m)]
        segs = []
        for i in range(self.ns):
            r = self.rows[i]
            segs.append(_segment3(pts[i], pts[i + 1], r[6], r[7], r[8], self.seabed and i == 0))
        for j in range(self.nleg):
            r = self.rows[self.ns + j]
            segs.append(_segment3(pts[self.m], fair[j], r[6], r[7], r[8], False))
        return None if any(s is None for s in segs) else segs

    def balance(self, segs):
        """Net force on the free points [3m] and the point stiffness K_uu [3m,3m] (minus its derivative)."""
        m, ns = self.m, self.ns
        R, K = np.zeros(3 * m, dtype=T_), np.zeros((3 * m, 3 * m), dtype=T_)
        for k in range(m):
            R[3 * k + 2] -= self.weight[k]
        for i, s in enumerate(segs):
            a, b = (i - 1, i) if i < ns else (m - 1, None)       # free-point indices of its ends (-1: the anchor, None: a fairlead)
            if b is not None:
                R[3 * b:3 * b + 3] += s["f"]
                K[3 * b:3 * b + 3, 3 * b:3 * b + 3] += s["K3"]
            if a >= 0:
                R[3 * a:3 * a + 3] += s["fA"]
                K[3 * a:3 * a + 3, 3 * a:3 * a + 3] += s["K3"]
                if b is not None:
                    K[3 * a:3 * a + 3, 3 * b:3 * b + 3] -= s["K3"]
                    K[3 * b:3 * b + 3, 3 * a:3 * a + 3] -= s["K3"]
        return R, K

    def start(self, fair, P):
        """The free points [3m] for the junction P: the stem's joints from a plane solve between the anchor and P."""
        d = P - self.anchor
        XF = np.sqrt(d[0] * d[0] + d[1] * d[1])
        r = self.rows[:self.ns]
        u = np.zeros(3 * self.m, dtype=T_)
        if self.ns > 1:
            segs, y, Ry, conv = mcr.solve_chain(XF, d[2], list(r[:, 6]), list(r[:, 7]), list(r[:, 8]), [T_(0)] + list(r[1:, ML_WJOINT]), self.seabed)
            if not conv:
                return None
            for k in range(self.ns - 1):
                u[3 * k:3 * k + 3] = self.anchor + np.array([y[2 * k] * d[0] / XF, y[2 * k] * d[1] / XF, y[2 * k + 1]], dtype=T_)
        u[3 * (self.m - 1):] = P
        return u

    def solve(self, fair, u, max_it=60):
        """Newton on all free points from u: (u, segments, K_uu, converged)."""
        segs = self.segments(u, fair)
        if segs is None:
            return u, None, None, False
        R, K = self.balance(segs)
        scale = sum(r[6] * r[8] for r in self.rows)
        res, a, conv = max(abs(R)) / scale, T_(1), False
        for _ in range(max_it):
            if res == 0:
                conv = True
                break
            d = np.linalg.solve(K.astype(np.float64), R.astype(np.float64)).astype(T_)
            d = d + np.linalg.solve(K.astype(np.float64), (R - K @ d).astype(np.float64)).astype(T_)       # refined in T
            st = self.segments(u + a * d, fair)
            if st is not None:
                Rt, Kt = self.balance(st)
                rt = max(abs(Rt)) / scale
            else:
                rt = np.inf
            if rt < res:
                u, segs, R, K, res, a = u + a * d, st, Rt, Kt, rt, T_(1)
            elif res <= 1e-10:
                conv = True                                      # stagnation (solve_line's rule)
                break
            else:
                a = a / 2
                if a < 2.0 ** -40:
                    break
        return u, segs, K, conv


def _fairleads(rows, ns, x, R, d6=None):
    """Arms and positions of the legs' fairleads at the pose (x, R), displaced by d6 = (translation, rotation vector) on top."""
    out_r, out_p = [], []
    for lg in rows[ns:]:
        r = R @ np.asarray(lg[3:6], dtype=T_)
        t = np.zeros(3, dtype=T_)
        if d6 is not None:
            TX = mr.skew(np.asarray(d6[3:], dtype=T_), T_)
            r = (np.eye(3, dtype=T_) + TX + TX @ TX / 2) @ r
            t = np.asarray(d6[:3], dtype=T_)
        out_r.append(r)
        out_p.append(x[:3] + t + r)
    return out_r, out_p


def bridle_state(rows, ns, pose, depth, d6=None, u0=None):
    """The solved system of one (unflagged) bridle: dict conv, sys, u, segs, K, r (arms), p (fairleads)."""
    rows = np.asarray(rows, dtype=np.float64)
    x = np.asarray(pose, dtype=np.float64).astype(T_)
    R = mr.rotation(x[3:], T_)
    S = _System(rows, ns, depth)
    r, p = _fairleads(rows.astype(T_), ns, x, R, d6)
    if u0 is None:
        fl, q = bdm.bridle(rows, ns, pose, depth)
        if q is None:
            return dict(conv=False)
        u0 = S.start(p, np.asarray(q["P"], dtype=np.float64).astype(T_))
        if u0 is None:
            return dict(conv=False)
    u, segs, K, conv = S.solve(p, u0)
    return dict(conv=conv, sys=S, u=u, segs=segs, K=K, r=r, p=p)


def bridle_terms(st):
    """C [6,6], F [6], T [n,2], J [n,2,6], lo [n,8], grounded, kappa and the envelopes EC, EF, ET, EJ of a solved bridle."""
    S, segs, K, r = st["sys"], st["segs"], st["K"], st["r"]
    m, ns, nleg = S.m, S.ns, S.nleg
    Ki = _inv(K)
    jP = slice(3 * (m - 1), 3 * m)
    legs = segs[ns:]
    B = [np.hstack([np.eye(3, dtype=T_), -mr.skew(r[j], T_)]) for j in range(nleg)]
    # the free points' motion for the unit's motion: du/dx6 = K_uu^-1 sum_j K_uf,j B_j, K_uf,j = the leg's K3 in the junction's rows
    dU, aU = np.zeros((3 * m, 6), dtype=T_), np.zeros((3 * m, 6), dtype=T_)
    for j in range(nleg):
        dU += Ki[:, jP] @ legs[j]["K3"] @ B[j]
        aU += abs(Ki[:, jP]) @ legs[j]["EK"] @ abs(B[j])
    KPP = _inv(Ki[jP, jP])                                       # the point stiffness condensed to the junction
    kappa = max(s["kappa"] for s in segs) + float(np.linalg.cond(KPP.astype(np.float64)))
    k1 = 1 + T_(kappa)
    C, EC, F, EF = (np.zeros((6, 6), dtype=T_), np.zeros((6, 6), dtype=T_), np.zeros(6, dtype=T_), np.zeros(6, dtype=T_))
    for i in range(nleg):
        f, RI = legs[i]["f"], mr.skew(r[i], T_)
        # -df_i/dx6 = K_i (B_i - dP/dx6)
        M = legs[i]["K3"] @ (B[i] - dU[jP])
        EM = legs[i]["EK"] @ (abs(B[i]) + aU[jP])
        C[:3] += M
        C[3:] += RI @ M
        EC[:3] += EM
        EC[3:] += abs(RI) @ EM
        C[3:, 3:] += -mr.skew(f, T_) @ RI
        EC[3:, 3:] += abs(mr.skew(f, T_)) @ abs(RI)
        F[:3] += f
        F[3:] += RI @ f
        EF[:3] += abs(f)
        EF[3:] += abs(RI) @ abs(f)
    n = ns + nleg
    Tn, J, ET, EJ, lo = (np.zeros((n, 2), dtype=T_), np.zeros((n, 2, 6), dtype=T_), np.zeros((n, 2), dtype=T_),
                         np.zeros((n, 2, 6), dtype=T_), np.zeros((n, 8), dtype=T_))
    zero = np.zeros((3, 6), dtype=T_)
    for i, s in enumerate(segs):
        if i < ns:
            dA, aA = (dU[3 * (i - 1):3 * i], aU[3 * (i - 1):3 * i]) if i > 0 else (zero, zero)
            dB, aB = dU[3 * i:3 * i + 3], aU[3 * i:3 * i + 3]
        else:
            dA, aA, dB, aB = dU[jP], aU[jP], B[i - ns], abs(B[i - ns])
        for e, nm in ((0, "A"), (1, "B")):
            Tn[i, e], ET[i, e] = s["T" + nm], s["T" + nm]
            J[i, e] = s["g" + nm] @ (dB - dA)
            EJ[i, e] = s["Eg" + nm] @ (aB + aA)
        lo[i] = [s["HF"], s["VF"], s["HF"], s["VA"], s["LB"], 0, s["branch"], 0]
    # grounded: the chain's rule for the stem; a free point, or the lowest point of a sagging segment, below the seabed
    floor = -S.depth - 1e-6 * S.depth
    low = [st["u"][3 * k + 2] for k in range(m)]
    for i, s in enumerate(segs):
        if not s["branch"] and s["VA"] < 0 < s["VF"]:
            vb = s["VA"] / s["HF"]
            low.append(s["zA"] - (s["HF"] / s["w"] * (np.sqrt(1 + vb * vb) - 1) + s["VA"] ** 2 / (2 * s["EA"] * s["w"])))
    grounded = bool(min(low) < floor) or bool(S.seabed and segs[0]["VF"] <= 0)
    return dict(C=C, F=F, T=Tn, J=J, lo=lo, EC=k1 * EC, EF=k1 * EF, ET=k1 * ET, EJ=k1 * EJ, kappa=kappa, grounded=grounded)


def evaluate(lines, pose, depth):
    """dict of C [nD,6,6], F [nD,6], T [nD,2nRow], J [nD,2nRow,6], line_out [nD,nRow,8], flags [nD] and the envelopes EC, EF,
    ET, EJ (kappa folded in) of designs of rows [nD,nRow,16].  Flagged designs are NaN."""
    lines = np.asarray(lines, dtype=np.float64)
    nD, nL = lines.shape[:2]
    pose = np.zeros((nD, 6)) if pose is None else np.asarray(pose, dtype=np.float64).reshape(nD, 6)
    out = dict(C=np.zeros((nD, 6, 6), dtype=T_), F=np.zeros((nD, 6), dtype=T_), T=np.zeros((nD, 2 * nL), dtype=T_),
               J=np.zeros((nD, 2 * nL, 6), dtype=T_), line_out=np.zeros((nD, nL, 8), dtype=T_), flags=np.zeros(nD, dtype=np.int32))
    for k in ("C", "F", "T", "J"):
        out["E" + k] = np.zeros_like(out[k])
    for d in range(nD):
        groups = bdm.groups_of(lines[d])
        parts = []
        for l, ns, nleg in groups:
            rows = lines[d, l:l + ns + nleg]
            if nleg:
                fl = bridle_flag(rows, ns, pose[d], depth)
                q = None
                if not fl:
                    st = bridle_state(rows, ns, pose[d], depth)
                    if not st["conv"]:
                        fl = FLAG_NO_CONVERGENCE
                    else:
                        q = bridle_terms(st)
                        if q["grounded"]:
                            fl = FLAG_GROUNDED
            else:
                c = mcr.evaluate(lines[d:d + 1, l:l + ns], pose[d:d + 1], depth)
                fl = int(c["flags"][0])
                q = dict(lo=c["line_out"][0])
                for k in ("C", "F", "EC", "EF"):
                    q[k] = c[k][0]
                for k in ("T", "J", "ET", "EJ"):
                    q[k] = np.stack([c[k][0, :ns], c[k][0, ns:]], axis=1)
            out["flags"][d] |= fl
            parts.append((l, ns + nleg, q))
        if out["flags"][d]:
            continue
        for l, n, q in parts:
            for k in ("C", "F", "EC", "EF"):
                out[k][d] += q[k]
            for k in ("T", "J", "ET", "EJ"):
                out[k][d, l:l + n], out[k][d, nL + l:nL + l + n] = q[k][:, 0], q[k][:, 1]
            out["line_out"][d, l:l + n] = q["lo"]
    bad = out["flags"] != 0
    for k in ("C", "F", "T", "J", "line_out"):
        out[k][bad] = np.nan
    return out


def fd_check(rows, ns, pose, depth, h=1e-4):
    """Worst |analytic - central difference| / envelope of C and J of one bridle (its rows only): the differences are of
    this file's own force function, a full re-solve per perturbed pose."""
    st = bridle_state(rows, ns, pose, depth)
    assert st["conv"]
    ref = bridle_terms(st)
    n = len(rows)
    Cfd, Jfd = np.zeros((6, 6), dtype=T_), np.zeros((n, 2, 6), dtype=T_)
    for j in range(6):
        vals = []
        for sgn in (+1, -1):
            d6 = np.zeros(6, dtype=T_)
            d6[j] = sgn * T_(h)
            sp = bridle_state(rows, ns, pose, depth, d6=d6, u0=st["u"])
            assert sp["conv"]
            F = np.zeros(6, dtype=T_)
            for i in range(sp["sys"].nleg):
                f = sp["segs"][ns + i]["f"]
                F[:3] += f
                F[3:] += np.cross(sp["r"][i], f)
            vals.append((F, np.array([[s["TA"], s["TB"]] for s in sp["segs"]], dtype=T_)))
        Cfd[:, j] = -(vals[0][0] - vals[1][0]) / (2 * T_(h))
        Jfd[:, :, j] = (vals[0][1] - vals[1][1]) / (2 * T_(h))
    tiny = np.finfo(np.float64).tiny
    return float((abs(ref["C"] - Cfd) / np.maximum(ref["EC"], tiny)).max()), float((abs(ref["J"] - Jfd) / np.maximum(ref["EJ"], tiny)).max())


gate_multiples = mr.gate_multiples
