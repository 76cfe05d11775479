"""Independent evaluation of everything the geometry generator derives from member, station and cap rows: the reference of
tests/test_geom_reference.py and tests/test_hip_geom_reference.py.

``design_reference(members, stations, caps, pose, rho, g, ...)`` evaluates ONE design in ``numpy.longdouble`` (or in plain
fp64 with ``dtype=np.float64``: the host restatement the gate's constant is measured with) by plain loops over members,
sections, strips and caps, from the formulas of

    raft_member.py:190-271      strip discretisation            raft_member.py:312-377    setPosition
    raft_member.py:1261-1368    calcHydroConstants              raft_member.py:2058-2110  drag areas
    raft_member.py:838-1010     getHydrostatics                 raft_member.py:380-836    getInertia (+ getWeight, :1179)
    helpers.py:36-148           FrustumVCV, FrustumMOI, RectangularFrustumMOI
    raft_fowt.py:1120-1201      T^T C T reductions, the geometric stiffness of the varying T, symmetrisation
    raft_model.py:1772-1827     adjustBallastDensity

and returns, per output, the value ``D`` and the envelope ``E``.

Envelope.  Every number is carried as a pair (v, e): an input double has e = |v|; a + b and a - b have e = e_a + e_b (the
sum of the absolute values of the addends, recursively: the subtractions INSIDE a formula -- Vo - Vi, hco Vo - hci Vi,
Iro - Iri, (r2^5 - r1^5) / (r2 - r1), ... - mass hc hc, the parallel-axis terms, the waterplane terms, the member-to-platform
arms, -m g + rho g V + Fz -- all widen it); a b has e_a |b| + |a| (e_b - |b|) and a / b that over b^2: the magnitude of
the result times one plus the relative excesses e / |v| - 1 of both operands, to first order (a zero operand passes the
other's envelope on); sqrt keeps the relative excess of its argument; sin, cos, tan and atan2 carry the conditioning of
their arguments, |f| + |f'| e_x.  An fp64 evaluation of the same formula in any order of its sums errs by
a small multiple of eps E; the gate is

    |x - D| <= C eps E per entry;  where E == 0 the result must be exactly 0;  where D is NaN it must be NaN.

Decisions.  DISCONTINUOUS decisions (wet or dry, the class of a section, ceil(l / dlsMax), the placement of a cap, the zero
guards, the whole part of the tensor a zero-length section adds once more) are recorded in ``decisions``; ``design_firmness`` evaluates the design in fp64 -- in the reference procedure's own
operation order, which is the order this file is written in -- and in longdouble and reports every disagreement.  A case
with one is a defect of the case list.  Decisions between branches that agree in the limit (dA == dB, La == Lb, Wa == Wb
of the moments of inertia, an exact hit of np.interp, the waterline scaling of v_i) are taken in the working precision;
the envelope covers them.  Every number also carries its fp64 shadow -- the same operations in plain fp64 -- so that the
one branch whose fp64 form is ill-conditioned, FrustumMOI's tapered quotient at a taper of rounding size, is recognised
in longdouble and given the envelope of what fp64 does there (``frustum_moi``).

Nothing here is shared with raft_amd or the kernels except the record-layout constants below.
"""
from types import SimpleNamespace

import numpy as np

GM_RA, GM_RB, GM_GAMMA, GM_SHAPE, GM_DLSMAX, GM_FLAGS, GM_L, GM_RHOSHELL = 0, 3, 6, 7, 8, 9, 10, 11
GS_S, GS_D, GS_T, GS_CD, GS_CA, GS_LFILL, GS_RHOFILL = 0, 1, 3, 4, 8, 12, 13
FLAG_POTMOD, FLAG_MCF, FLAG_NOSTATIC = 1, 2, 4
F_X, F_AX, F_Q, F_P1, F_P2 = 0, 3, 6, 9, 12
F_IQ, F_IP1, F_IP2, F_AI = 15, 16, 17, 18
F_DQ, F_DP1, F_DP2, F_DEND, F_CIRC, F_MCF, F_RHOV = 19, 20, 21, 22, 23, 24, 25
NGATED = 26                     # columns 0:26 of a strip record are gated; 26:28 (member, strip index) are exact
SP_V, SP_AWP, SP_RCB, SP_MASS, SP_RCG, SP_DRHO, SP_VFILL, SP_NGATED = 0, 1, 2, 5, 6, 9, 10, 11
EPS = float(np.finfo(np.float64).eps)

# C = the power of two at or above 16 x the worst CPU-side multiple (the fp64 mode of this file and the oracle library
# against the longdouble mode, over the whole case list of tests/geom_cases.py); the host implementations stay inside
# C / 4.  Measured by tests/test_geom_reference.py::test_gate_constant_is_the_measured_one (figures: DESIGN.md section 4).
GATE_C = 64          # worst CPU multiples: fp64 mode 3.02, oracle library 3.02 (C_hydro of the 129-member design)

STATICS = ("A_morison", "C_hydro", "W_hydro", "M_struc", "C_struc", "W_struc", "props")


# ------------------------------------------------------------------ numbers with envelopes
class N:
    """A value, its envelope (module docstring) and its fp64 shadow ``f``: the same operations in plain fp64."""
    __slots__ = ("v", "e", "f")

    def __init__(self, v, e, f=None):
        self.v, self.e, self.f = v, e, np.float64(v) if f is None else f

    def _of(self, o):
        if isinstance(o, N):
            return o
        t = type(self.v)(o)
        return N(t, abs(t), np.float64(o))

    def __add__(self, o):
        o = self._of(o)
        return N(self.v + o.v, self.e + o.e, self.f + o.f)

    __radd__ = __add__

    def __sub__(self, o):
        o = self._of(o)
        return N(self.v - o.v, self.e + o.e, self.f - o.f)

    def __rsub__(self, o):
        return self._of(o) - self

    def __mul__(self, o):
        o = self._of(o)
        return N(self.v * o.v, self.e * abs(o.v) + abs(self.v) * (o.e - abs(o.v)), self.f * o.f)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._of(o)
        return N(self.v / o.v, (self.e * abs(o.v) + abs(self.v) * (o.e - abs(o.v))) / (o.v * o.v), self.f / o.f)

    def __rtruediv__(self, o):
        return self._of(o) / self

    def __neg__(self):
        return N(-self.v, self.e, -self.f)

    def __abs__(self):
        return N(abs(self.v), self.e, abs(self.f))


def fsqrt(x):
    v = np.sqrt(x.v)
    return N(v, v * (x.e / abs(x.v)) if x.v != 0 else np.sqrt(x.e), np.sqrt(x.f))


def fsin(x):
    s, c = np.sin(x.v), np.cos(x.v)
    return N(s, abs(s) + abs(c) * x.e, np.sin(x.f))


def fcos(x):
    s, c = np.sin(x.v), np.cos(x.v)
    return N(c, abs(c) + abs(s) * x.e, np.cos(x.f))


def ftan(x):
    t = np.tan(x.v)
    return N(t, abs(t) + (1 + t * t) * x.e, np.tan(x.f))


def fatan2(y, x):
    v = np.arctan2(y.v, x.v)
    h = x.v * x.v + y.v * y.v
    return N(v, abs(v) + ((abs(x.v) * y.e + abs(y.v) * x.e) / h if h != 0 else h), np.arctan2(y.f, x.f))


def fpow5(x):
    x2 = x * x
    return x2 * x2 * x


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def matvec(M, v):
    return [M[i][0] * v[0] + M[i][1] * v[1] + M[i][2] * v[2] for i in range(3)]


class Refused(Exception):
    """A cap layout the reference procedure itself fails on (raft_member.py:684-688, 731-755)."""


class _Model:
    def __init__(self, T, faults):
        self.T = T
        self.faults = faults or {}
        self.decisions = []
        self.PI = self.num(np.pi)                     # the fp64 constant the procedure is written with

    def num(self, x):
        t = self.T(x)
        return N(t, abs(t), np.float64(x))

    def zero(self):
        return N(self.T(0), self.T(0), np.float64(0))

    def zeros(self, *shape):
        if len(shape) == 1:
            return [self.zero() for _ in range(shape[0])]
        return [self.zeros(*shape[1:]) for _ in range(shape[0])]

    def decide(self, tag, outcome):
        self.decisions.append((tag, outcome))
        return outcome

    # ---------------------------------------------------------------- np.interp(x, xp, fp), numpy's own rules
    def interp(self, x, xp, fp):
        n = len(xp)
        if x.v < xp[0].v:
            return fp[0]
        if x.v > xp[n - 1].v:
            return fp[n - 1]
        j = 0
        for i in range(n):
            if xp[i].v <= x.v:
                j = i                                 # the LAST station at or below x
        if self.faults.get("interp_first"):
            for i in range(n):
                if xp[i].v == x.v:
                    j = i
                    break
        if j == n - 1 or xp[j].v == x.v:
            return fp[j]
        slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j])
        return slope * (x - xp[j]) + fp[j]

    # ---------------------------------------------------------------- setPosition, raft_member.py:312-377
    def pose_member(self, gm, pose):
        num = self.num
        rA0 = [num(gm[GM_RA + i]) for i in range(3)]
        rAB = [num(gm[GM_RB + i]) - rA0[i] for i in range(3)]
        nrm = fsqrt(rAB[0] * rAB[0] + rAB[1] * rAB[1] + rAB[2] * rAB[2])
        q0 = [c / nrm for c in rAB]
        beta = fatan2(q0[1], q0[0])
        phi = fatan2(fsqrt(q0[0] * q0[0] + q0[1] * q0[1]), q0[2])
        gam = num(gm[GM_GAMMA]) * num(np.pi / 180.0)
        s1, c1, s2, c2, s3, c3 = fsin(beta), fcos(beta), fsin(phi), fcos(phi), fsin(gam), fcos(gam)
        R0 = [[c1 * c2 * c3 - s1 * s3, -c3 * s1 - c1 * c2 * s3, c1 * s2],
              [c1 * s3 + c2 * c3 * s1, c1 * c3 - c2 * s1 * s3, s1 * s2],
              [-c3 * s2, s2 * s3, c2]]
        p10 = [R0[0][0], R0[1][0], R0[2][0]]
        p20 = cross(q0, p10)
        a3, a2, a1 = (num(pose[3 + i]) for i in range(3))
        s1, c1, s2, c2, s3, c3 = fsin(a1), fcos(a1), fsin(a2), fcos(a2), fsin(a3), fcos(a3)
        Rp = [[c1 * c2, c1 * s2 * s3 - c3 * s1, s1 * s3 + c1 * c3 * s2],          # helpers.py:439-466
              [c2 * s1, c1 * c3 + s1 * s2 * s3, c3 * s1 * s2 - c1 * s3],
              [-s2, c2 * s3, c2 * c3]]
        P = SimpleNamespace(rA0=rA0, L=num(gm[GM_L]))
        P.R = [[Rp[i][0] * R0[0][j] + Rp[i][1] * R0[1][j] + Rp[i][2] * R0[2][j] for j in range(3)] for i in range(3)]
        P.q, P.p1, P.p2 = matvec(Rp, q0), matvec(Rp, p10), matvec(Rp, p20)
        RmI = [[Rp[i][j] - (1.0 if i == j else 0.0) for j in range(3)] for i in range(3)]
        d = matvec(RmI, rA0)                                                      # raft_fowt.py:706-718
        P.rA = [rA0[i] + (num(pose[i]) + d[i]) for i in range(3)]
        P.rB = [P.rA[i] + P.L * P.q[i] for i in range(3)]
        return P

    # ---------------------------------------------------------------- strips of Member.__init__, raft_member.py:190-271
    def discretise(self, gm, st, m):
        circ = gm[GM_SHAPE] != 0.0
        nd = 1 if circ else 2
        n = len(st)
        dlsMax = self.num(gm[GM_DLSMAX])
        half = lambda i, c: 0.5 * st[i][GS_D + c]
        out = [(st[0][GS_S], self.zero(), [half(0, c) for c in range(nd)], [half(0, c) for c in range(nd)])]
        for i in range(1, n):
            l = st[i][GS_S] - st[i - 1][GS_S]
            if l.v > 0:
                nsub = self.decide("m%d section %d: ceil(l / dlsMax)" % (m, i), int(np.ceil((l / dlsMax).v)))
                dl = l / nsub
                for j in range(nsub):
                    ds, drs = [], []
                    for c in range(nd):
                        mm = 0.5 * (st[i][GS_D + c] - st[i - 1][GS_D + c]) / l
                        ds.append(st[i - 1][GS_D + c] + dl * 2 * mm * (0.5 + j))
                        drs.append(dl * mm)
                    out.append((st[i - 1][GS_S] + dl * (0.5 + j), dl, ds, drs))
            elif l.v == 0:
                out.append((st[i - 1][GS_S], self.zero(), [0.5 * (st[i - 1][GS_D + c] + st[i][GS_D + c]) for c in range(nd)],
                            [0.5 * (st[i][GS_D + c] - st[i - 1][GS_D + c]) for c in range(nd)]))
        out.append((st[n - 1][GS_S], self.zero(), [half(n - 1, c) for c in range(nd)], [-half(n - 1, c) for c in range(nd)]))
        return out

    # ---------------------------------------------------------------- calcHydroConstants + drag areas for one member
    def member_strips(self, gm, st, P, rP, rho, m, recs, idx, amor, n_mcf):
        circ = gm[GM_SHAPE] != 0.0
        flags = int(gm[GM_FLAGS])
        potmod, mcf = bool(flags & FLAG_POTMOD), bool(flags & FLAG_MCF) and circ
        num, PI = self.num, self.PI
        cdrag = num(np.sqrt(8 / np.pi))
        arm_node = [P.rA[i] - rP[i] for i in range(3)]
        sx = [row[GS_S] for row in st]
        coef = lambda ls, f: self.interp(ls, sx, [row[f] for row in st])
        for il, (ls, dls, ds, drs) in enumerate(self.discretise(gm, st, m)):
            r = [P.rA[i] + (ls / P.L) * (P.rB[i] - P.rA[i]) for i in range(3)]   # :362
            if not self.decide("m%d strip %d: r_z < 0" % (m, il), bool(r[2].v < 0)):
                continue
            rec = self.zeros(NGATED)
            ax = [(r[i] - P.rA[i]) + arm_node[i] for i in range(3)]
            for i in range(3):
                rec[F_X + i], rec[F_AX + i] = r[i], ax[i]
                rec[F_Q + i], rec[F_P1 + i], rec[F_P2 + i] = P.q[i], P.p1[i], P.p2[i]
            rec[F_CIRC] = num(1.0 if circ else 0.0)
            rec[F_MCF] = num(-1.0)
            if not potmod:
                if circ:
                    v_i = 0.25 * PI * ds[0] * ds[0] * dls                         # :1323
                    a3, b3 = ds[0] + drs[0], ds[0] - drs[0]
                    v_end = PI / 12.0 * abs(a3 * a3 * a3 - b3 * b3 * b3)          # :1341
                    a_i = PI * ds[0] * drs[0]
                else:
                    v_i = ds[0] * ds[1] * dls
                    ma = 0.5 * ((ds[0] + drs[0]) + (ds[1] + drs[1]))
                    mb = 0.5 * ((ds[0] - drs[0]) + (ds[1] - drs[1]))
                    v_end = PI / 12.0 * (ma * ma * ma - mb * mb * mb)             # :1345
                    a_i = (ds[0] + drs[0]) * (ds[1] + drs[1]) - (ds[0] - drs[0]) * (ds[1] - drs[1])
                if (r[2] + 0.5 * dls).v > 0 and not self.faults.get("no_wl_scale"):
                    v_i = v_i * (0.5 * dls - r[2]) / dls                          # :1328-1330
                Ca1, Ca2, CaE = coef(ls, GS_CA + 1), coef(ls, GS_CA + 2), coef(ls, GS_CA + 3)
                rec[F_IQ] = rho * v_end * CaE
                rec[F_AI] = a_i
                rec[F_RHOV] = rho * v_i
                if mcf:
                    rec[F_MCF] = num(float(n_mcf[0]))
                    n_mcf[0] += 1
                else:
                    rec[F_IP1] = rho * v_i * (1.0 + Ca1)
                    rec[F_IP2] = rho * v_i * (1.0 + Ca2)
                amor.append((ax, [(rho * v_i * Ca1, P.p1), (rho * v_i * Ca2, P.p2), (rho * v_end * CaE, P.q)]))
            if circ:                                                              # :2066-2110
                a_q, a_p1, a_p2, a_end = PI * ds[0] * dls, ds[0] * dls, ds[0] * dls, abs(PI * ds[0] * drs[0])
            else:
                a_q, a_p1, a_p2 = 2 * (ds[0] + ds[0]) * dls, ds[0] * dls, ds[1] * dls       # (sic) :2070
                a_end = abs((ds[0] + drs[0]) * (ds[1] + drs[1]) - (ds[0] - drs[0]) * (ds[1] - drs[1]))
            rec[F_DQ] = cdrag * 0.5 * rho * a_q * coef(ls, GS_CD + 0)
            rec[F_DP1] = cdrag * 0.5 * rho * a_p1 * coef(ls, GS_CD + 1)
            rec[F_DP2] = cdrag * 0.5 * rho * a_p2 * coef(ls, GS_CD + 2)
            rec[F_DEND] = cdrag * 0.5 * rho * a_end * coef(ls, GS_CD + 3)
            recs.append(rec)
            idx.append((m, il))

    def morison(self, amor):
        """A_hydro_morison: translateMatrix3to6DOF(Amat, arm) summed over the wet strips (helpers.py:537-560)."""
        A = self.zeros(6, 6)
        S = len(amor)
        if self.faults.get("amor_drop3") and S == 2:
            amor = amor[:(S * 2) // 3]
        for ax, terms in amor:
            Am = self.zeros(3, 3)
            for c, v in terms:
                for i in range(3):
                    for j in range(3):
                        Am[i][j] = Am[i][j] + c * (v[i] * v[j])
            self.add_translated3(A, Am, ax)
        return A

    def H(self, r):
        z = self.zero()
        return [[z, r[2], -r[1]], [-r[2], z, r[0]], [r[1], -r[0], z]]

    def add_translated3(self, out, M, r):
        H = self.H(r)
        MH = [[M[i][0] * H[0][j] + M[i][1] * H[1][j] + M[i][2] * H[2][j] for j in range(3)] for i in range(3)]
        HM = [[H[i][0] * M[0][j] + H[i][1] * M[1][j] + H[i][2] * M[2][j] for j in range(3)] for i in range(3)]
        for i in range(3):
            for j in range(3):
                out[i][j] = out[i][j] + M[i][j]
                out[i][3 + j] = out[i][3 + j] + MH[i][j]
                out[3 + i][j] = out[3 + i][j] + MH[j][i]
                out[3 + i][3 + j] = out[3 + i][3 + j] + (HM[i][0] * H[j][0] + HM[i][1] * H[j][1] + HM[i][2] * H[j][2])

    # ---------------------------------------------------------------- helpers.py:36-63
    def frustum_vcv(self, dA, dB, H, tag):
        sA, sB = sum(d.v for d in dA), sum(d.v for d in dB)
        if self.decide(tag + ": sA == 0 and sB == 0", bool(sA == 0 and sB == 0)):
            return self.zero(), self.zero()
        if len(dA) == 1:
            c = self.num(np.pi / 4)
            A1, A2, Am = c * dA[0] * dA[0], c * dB[0] * dB[0], c * dA[0] * dB[0]
        else:
            A1, A2 = dA[0] * dA[1], dB[0] * dB[1]
            Am = fsqrt(A1 * A2)
        return (A1 + A2 + Am) * H / 3, ((A1 + 2 * Am + 3 * A2) / (A1 + Am + A2)) * H / 4

    def force3to6(self, F, r):                                                    # helpers.py:468-483
        return list(F) + cross(r, F)

    # ---------------------------------------------------------------- getHydrostatics, raft_member.py:838-1010
    def hydrostatics(self, gm, st, P, rho, g, m):
        circ = gm[GM_SHAPE] != 0.0
        nd = 1 if circ else 2
        z = self.zero
        out = SimpleNamespace(F=self.zeros(6), C=self.zeros(6, 6), V=z(), rcV=self.zeros(3), AWP=z())
        beta = fatan2(P.q[1], P.q[0])
        phi = fatan2(fsqrt(P.q[0] * P.q[0] + P.q[1] * P.q[1]), P.q[2])
        cosPhi, sinPhi, cosBeta, sinBeta = fcos(phi), fsin(phi), fcos(beta), fsin(beta)
        rg = rho * g
        C = out.C
        for i in range(1, len(st)):
            rA = [P.rA[c] + P.q[c] * st[i - 1][GS_S] for c in range(3)]
            rB = [P.rA[c] + P.q[c] * st[i][GS_S] for c in range(3)]
            dlo = [st[i - 1][GS_D + c] for c in range(nd)]
            dhi = [st[i][GS_D + c] for c in range(nd)]
            if rA[2].v * rB[2].v <= 0:
                cls = 1
            elif rA[2].v <= 0 and rB[2].v <= 0:
                cls = 2
            else:
                cls = 0
            self.decide("m%d section %d: crossing / submerged / dry" % (m, i), cls)
            if cls == 1:
                xWP = rA[0] + (0 - rA[2]) * (rB[0] - rA[0]) / (rB[2] - rA[2])   # helpers.py:423
                yWP = rA[1] + (0 - rA[2]) * (rB[1] - rA[1]) / (rB[2] - rA[2])
                if self.faults.get("wp_lower"):
                    dWP = [dlo[c] + (0 - rA[2]) * (dhi[c] - dlo[c]) / (rB[2] - rA[2]) for c in range(nd)]
                else:                                                             # (sic) d[i] first, :899,905
                    dWP = [dhi[c] + (0 - rA[2]) * (dlo[c] - dhi[c]) / (rB[2] - rA[2]) for c in range(nd)]
                if circ:
                    AWP = self.num(np.pi / 4) * dWP[0] * dWP[0]
                    IxWP = IyWP = self.num(np.pi / 64) * dWP[0] * dWP[0] * dWP[0] * dWP[0]
                else:
                    AWP = dWP[0] * dWP[1]
                    Ix = (1.0 / 12) * dWP[0] * dWP[1] * dWP[1] * dWP[1]
                    Iy = (1.0 / 12) * dWP[0] * dWP[0] * dWP[0] * dWP[1]
                    IxWP = P.R[0][0] * Ix * P.R[0][0] + P.R[0][1] * Iy * P.R[0][1]   # :909-913
                    IyWP = P.R[1][0] * Ix * P.R[1][0] + P.R[1][1] * Iy * P.R[1][1]
                LWP = abs(rA[2] / cosPhi)
                V, hc = self.frustum_vcv(dlo, dWP, LWP, "m%d section %d wet part" % (m, i))
                rc = [rA[c] + P.q[c] * hc for c in range(3)]
                Mm = z()
                if circ:
                    tanPhi = ftan(phi)
                    Mm = -rg * self.PI * (dWP[0] * dWP[0] / 32 * (2.0 + tanPhi * tanPhi)
                                          + 0.5 * (rA[2] / cosPhi) * (rA[2] / cosPhi)) * sinPhi
                rel = [rA[c] - P.rA[c] for c in range(3)]
                F6 = self.force3to6([z(), z(), rg * V], rel)
                for c in range(6):
                    out.F[c] = out.F[c] + F6[c]
                out.F[3] = out.F[3] + Mm * (-sinBeta)
                out.F[4] = out.F[4] + Mm * cosBeta
                xWP, yWP = xWP - P.rA[0], yWP - P.rA[1]
                C[2][2] = C[2][2] + rg * AWP / cosPhi
                C[2][3] = C[2][3] + rg * (-AWP * yWP)
                C[2][4] = C[2][4] + rg * (AWP * xWP)
                C[3][2] = C[3][2] + rg * (-AWP * yWP)
                C[3][3] = C[3][3] + rg * (IxWP + AWP * yWP * yWP)
                C[3][4] = C[3][4] + rg * (AWP * xWP * yWP)
                C[4][2] = C[4][2] + rg * (AWP * xWP)
                C[4][3] = C[4][3] + rg * (AWP * xWP * yWP)
                C[4][4] = C[4][4] + rg * (IyWP + AWP * xWP * xWP)
                out.AWP = AWP                                                     # the last crossing wins, :866-869
            elif cls == 2:
                V, hc = self.frustum_vcv(dlo, dhi, st[i][GS_S] - st[i - 1][GS_S], "m%d section %d" % (m, i))
                rc = [rA[c] + P.q[c] * hc for c in range(3)]
                F6 = self.force3to6([z(), z(), rg * V], [rc[c] - P.rA[c] for c in range(3)])
                for c in range(6):
                    out.F[c] = out.F[c] + F6[c]
            else:
                continue
            rr = [rc[c] - P.rA[c] for c in range(3)]
            t33 = rg * V * rr[2]
            if self.faults.get("ch33_rel") and not getattr(self, "_ch33_done", False):
                t33 = N(t33.v * (1 + self.T(self.faults["ch33_rel"])), t33.e, t33.f)
                self._ch33_done = True
            C[3][3] = C[3][3] + t33
            C[4][4] = C[4][4] + rg * V * rr[2]
            C[3][5] = C[3][5] - rg * V * rr[0]
            C[4][5] = C[4][5] - rg * V * rr[1]
            out.V = out.V + V
            for c in range(3):
                out.rcV[c] = out.rcV[c] + rc[c] * V
        return out

    # ---------------------------------------------------------------- helpers.py:65-148
    def frustum_moi(self, dA, dB, H, p):
        if H.v == 0:
            return self.zero(), self.zero()
        PI = self.PI
        r1, r2 = dA / 2, dB / 2
        same = dA.v == dB.v and dA.f == dB.f
        # radii that only a rounding error separates (a hole "tapered" by dA (dBi / dB), :691): the procedure in fp64 takes
        # the tapered branch, whose quotient is then decided by the last bits of r^5; the value is the limit the branches
        # share, the envelope that of the quotient at the smallest separation fp64 can see, ulp(r) >= eps r / 2
        blurred = not same and self.T is not np.float64 and abs(r2.v - r1.v) <= EPS * (r1.e + r2.e)
        if same or blurred:
            Ir = (1.0 / 12) * (p * H * PI * r1 * r1) * (3 * r1 * r1 + 4 * H * H)
            Ia = (1.0 / 2) * p * PI * H * r1 * r1 * r1 * r1
            if blurred:
                qe = (fpow5(r2).e + fpow5(r1).e) / (EPS * max(abs(r1.v), abs(r2.v)) / 2)
                c = abs(p.v * PI.v * H.v)
                Ir, Ia = N(Ir.v, Ir.e + c * qe / 20, Ir.f), N(Ia.v, Ia.e + c * qe / 10, Ia.f)
            return Ir, Ia
        quo = (fpow5(r2) - fpow5(r1)) / (r2 - r1)
        return ((1.0 / 20) * p * PI * H * quo + (1.0 / 30) * p * PI * H * H * H * (r1 * r1 + 3 * r1 * r2 + 6 * r2 * r2),
                (1.0 / 10) * p * PI * H * quo)

    def rect_moi(self, La, Wa, Lb, Wb, H, p):
        if H.v == 0:
            return self.zeros(3)
        if La.v == Lb.v and Wa.v == Wb.v:
            M = p * La * Wa * H
            return [(1.0 / 12) * M * (Wa * Wa + 4 * H * H), (1.0 / 12) * M * (La * La + 4 * H * H), (1.0 / 12) * M * (La * La + Wa * Wa)]
        if La.v != Lb.v and Wa.v != Wb.v:
            dL, dW = Lb - La, Wb - Wa
            x2 = (1.0 / 12) * p * (dL * dL * dL * H * (Wb / 5 + Wa / 20) + dL * dL * La * H * (3 * Wb / 4 + Wa / 4)
                                   + dL * La * La * H * (Wb + Wa / 2) + La * La * La * H * (Wb / 2 + Wa / 2))
            y2 = (1.0 / 12) * p * (dW * dW * dW * H * (Lb / 5 + La / 20) + dW * dW * Wa * H * (3 * Lb / 4 + La / 4)
                                   + dW * Wa * Wa * H * (Lb + La / 2) + Wa * Wa * Wa * H * (Lb / 2 + La / 2))
            z2 = p * (Wb * Lb / 5 + Wa * Lb / 20 + La * Wb / 20 + Wa * La * (1.0 / 30)) * H * H * H
        elif La.v == Lb.v:
            L = La
            x2 = (1.0 / 24) * p * (L * L * L) * H * (Wb + Wa)
            y2 = (1.0 / 48) * p * L * H * (Wb * Wb * Wb + Wa * Wb * Wb + Wa * Wa * Wb + Wa * Wa * Wa)
            z2 = (1.0 / 12) * p * L * (H * H * H) * (3 * Wb + Wa)
        else:
            W = Wa
            x2 = (1.0 / 48) * p * W * H * (Lb * Lb * Lb + La * Lb * Lb + La * La * Lb + La * La * La)
            y2 = (1.0 / 24) * p * (W * W * W) * H * (Lb + La)
            z2 = (1.0 / 12) * p * W * (H * H * H) * (3 * Lb + La)
        return [y2 + z2, x2 + z2, x2 + y2]

    def moi3(self, circ, dA, dB, H, p):
        if circ:
            Ir, Ia = self.frustum_moi(dA[0], dB[0], H, p)
            return [Ir, Ir, Ia]
        return self.rect_moi(dA[0], dA[1], dB[0], dB[1], H, p)

    def add_submember(self, M, mass, Iv, R, r, whole=None):
        """M += translateMatrix6to6DOF(diag(m, m, m) (+) R diag(I) R^T, r), helpers.py:563-585.  ``whole`` (a tag): the
        sub-member matrix is an INTEGER array -- np.diag of the integer mass 0 of a zero-length section, :417,531 -- so the
        rotated tensor stored into it (:537) loses its fractional part, towards zero: a discontinuous decision per entry."""
        H = self.H(r)
        for i in range(3):
            for j in range(3):
                Irot = R[i][0] * Iv[0] * R[j][0] + R[i][1] * Iv[1] * R[j][1] + R[i][2] * Iv[2] * R[j][2]
                if whole and not self.faults.get("readd_fraction"):
                    w = np.trunc(Irot.v)
                    self.decide("%s: whole part of I_rot[%d][%d]" % (whole, i, j), float(w))
                    Irot = N(w, abs(w), np.trunc(Irot.f))
                hmh = H[i][0] * mass * H[j][0] + H[i][1] * mass * H[j][1] + H[i][2] * mass * H[j][2]
                if i == j:
                    M[i][j] = M[i][j] + mass
                M[i][3 + j] = M[i][3 + j] + mass * H[i][j]
                M[3 + i][j] = M[3 + i][j] + mass * H[j][i]
                M[3 + i][3 + j] = M[3 + i][3 + j] + (hmh + Irot)

    def shell(self, dA, dB, dAi, dBi, H, tag):
        """Volume difference and its centre: (Vo - Vi, hc) of FrustumVCV outside minus inside."""
        Vo, hco = self.frustum_vcv(dA, dB, H, tag + " outer")
        Vi, hci = self.frustum_vcv(dAi, dBi, H, tag + " inner")
        dV = Vo - Vi
        if self.decide(tag + ": Vo - Vi != 0", bool(dV.v != 0)):
            hc = hco * Vo / dV if self.faults.get("hc_shell_outer") and "cap" not in tag else ((hco * Vo) - (hci * Vi)) / dV
        else:
            hc = self.zero()
        return dV, hc

    # ---------------------------------------------------------------- getInertia + getWeight, raft_member.py:380-836, 1179
    def inertia(self, gm, st, caps, P, g, m):
        circ = gm[GM_SHAPE] != 0.0
        nd = 1 if circ else 2
        n = len(st)
        z = self.zero
        rho_shell = self.num(gm[GM_RHOSHELL])
        out = SimpleNamespace(M=self.zeros(6, 6), vfill=z())
        mc = self.zeros(3)
        I3 = self.zeros(3)                                        # NOT reset for a zero-length section (:420-513): its
        #                                                           tensor is added once more, with zero mass, as whole numbers
        for i in range(1, n):
            l = st[i][GS_S] - st[i - 1][GS_S]
            mass, center = z(), self.zeros(3)
            if l.v > 0:
                tag = "m%d section %d" % (m, i)
                l_fill, rho_fill = st[i - 1][GS_LFILL], st[i - 1][GS_RHOFILL]
                dA = [st[i - 1][GS_D + c] for c in range(nd)]
                dB = [st[i][GS_D + c] for c in range(nd)]
                dAi = [dA[c] - 2 * st[i - 1][GS_T] for c in range(nd)]
                dBi = [dB[c] - 2 * st[i][GS_T] for c in range(nd)]
                dBf = [(dBi[c] - dAi[c]) * (l_fill / l) + dAi[c] for c in range(nd)]
                dV, hc_shell = self.shell(dA, dB, dAi, dBi, l, tag)
                m_shell = dV * rho_shell
                vf, hcf = self.frustum_vcv(dAi, dBf, l_fill, tag + " fill")
                out.vfill = out.vfill + vf
                m_fill = vf * rho_fill
                mass = m_shell + m_fill
                if self.decide(tag + ": mass != 0", bool(mass.v != 0)):
                    hc = ((hcf * m_fill) + (hc_shell * m_shell)) / mass
                else:
                    hc = z()
                Io, Ii, If = (self.moi3(circ, dA, dB, l, rho_shell), self.moi3(circ, dAi, dBi, l, rho_shell),
                              self.moi3(circ, dAi, dBf, l_fill, rho_fill))
                I3 = [((Io[0] - Ii[0]) + If[0]) - mass * hc * hc, ((Io[1] - Ii[1]) + If[1]) - mass * hc * hc,
                      (Io[2] - Ii[2]) + If[2]]
                center = [P.rA[c] + P.q[c] * (st[i - 1][GS_S] + hc) for c in range(3)]
            for c in range(3):
                mc[c] = mc[c] + mass * center[c]
            self.add_submember(out.M, mass, I3, P.R, [center[c] - P.rA[c] for c in range(3)],
                               whole=None if l.v > 0 else "m%d section %d" % (m, i))
        # ---- end caps and bulkheads, :659-810
        sx = [row[GS_S] for row in st]
        din = [[row[GS_D + c] - 2 * row[GS_T] for row in st] for c in range(nd)]
        DIN = lambda x, c: self.interp(x, sx, din[c])
        s0, s1 = st[0][GS_S], st[n - 1][GS_S]
        ncap = len(caps)
        for i in range(ncap):
            Lc, h = self.num(caps[i][0]), self.num(caps[i][1])
            hole = [self.num(caps[i][2 + c]) for c in range(nd)]
            tag = "m%d cap %d" % (m, i)
            if Lc.v == s0.v:
                where = 0
            elif Lc.v == s1.v:
                where = 1
            elif (Lc.v > s0.v and Lc.v < (s0 + h).v) or (Lc.v < s1.v and Lc.v > (s1 - h).v):
                where = 3
            else:
                where = 2
            pair = 0
            if where == 2:
                if i < ncap - 1 and caps[i][0] == caps[i + 1][0]:
                    pair = -1                                     # the cap going down at a discontinuity
                elif i > 0 and caps[i][0] == caps[i - 1][0]:
                    pair = 1                                      # ... and the one going up
            self.decide(tag + ": bottom / top / middle / too close, paired", (where, pair))
            if where == 3:
                raise Refused("member %d cap %d: closer to the end than its own thickness" % (m, i))
            if where != 0 and not circ:
                raise Refused("member %d cap %d: a rectangular cap that is not at end A" % (m, i))
            if where == 0:
                dA = [din[c][0] for c in range(nd)]
                dB = [DIN(Lc + h, c) for c in range(nd)]
                dAi = hole
                dBi = [dB[c] * (dAi[c] / dA[c]) for c in range(nd)]
            elif where == 1:
                dA, dB, dBi = [DIN(Lc - h, 0)], [din[0][n - 1]], hole
                dAi = [dA[0] * (dBi[0] / dB[0])]
            elif pair:
                if i >= n:
                    raise Refused("member %d cap %d: no station of that index" % (m, i))
                if pair < 0:                                      # (sic) the station of the CAP's index, :690
                    dA, dB, dBi = [DIN(Lc - h, 0)], [din[0][i]], hole
                    dAi = [dA[0] * (dBi[0] / dB[0])]
                else:
                    dA, dB, dAi = [din[0][i]], [DIN(Lc + h, 0)], hole
                    dBi = [dB[0] * (dAi[0] / dA[0])]
            else:
                dA, dB, dM = [DIN(Lc - h / 2, 0)], [DIN(Lc + h / 2, 0)], DIN(Lc, 0)
                dAi, dBi = [dA[0] * (hole[0] / dM)], [dB[0] * (hole[0] / dM)]
            dV, hc_cap = self.shell(dA, dB, dAi, dBi, h, tag)
            m_cap = dV * rho_shell
            Io, Ii = self.moi3(circ, dA, dB, h, rho_shell), self.moi3(circ, dAi, dBi, h, rho_shell)
            Ic = [(Io[0] - Ii[0]) - m_cap * hc_cap * hc_cap, (Io[1] - Ii[1]) - m_cap * hc_cap * hc_cap, Io[2] - Ii[2]]
            cc = []
            for c in range(3):
                pos = P.rA[c] + P.q[c] * Lc                       # :772-778
                if where == 0:
                    cc.append(pos + P.q[c] * hc_cap)
                elif where == 1:
                    cc.append(pos - P.q[c] * (h - hc_cap))
                elif self.faults.get("midcap_sign"):
                    cc.append(pos + P.q[c] * ((h / 2) - hc_cap))
                else:
                    cc.append(pos - P.q[c] * ((h / 2) - hc_cap))
                mc[c] = mc[c] + m_cap * cc[c]
            self.add_submember(out.M, m_cap, Ic, P.R, [cc[c] - P.rA[c] for c in range(3)])
        out.mass = out.M[0][0]
        if self.decide("m%d: mass != 0" % m, bool(out.mass.v != 0)):
            out.center = [mc[c] / out.mass for c in range(3)]
        else:
            out.center = self.zeros(3)
        dR = [out.center[c] - P.rA[c] for c in range(3)]          # helpers.py:1060-1082
        out.W = self.force3to6([z(), z(), -g * out.mass], dR)
        out.C = self.zeros(6, 6)
        out.C[3][3] = out.C[3][3] - out.mass * g * dR[2]
        out.C[4][4] = out.C[4][4] - out.mass * g * dR[2]
        return out

    # ---------------------------------------------------------------- raft_fowt.py:1120-1201
    def reduce_matrix(self, out, M, arm):
        H = self.H(arm)
        one = self.num(1.0)
        T = [[(one if i == j else None) for j in range(6)] for i in range(6)]
        for i in range(3):
            for j in range(3):
                if i != j:
                    T[i][3 + j] = H[i][j]
        tmp = self.zeros(6, 6)
        for i in range(6):
            for j in range(6):
                s = self.zero()
                for k in range(6):
                    if T[k][j] is not None:
                        s = s + M[i][k] * T[k][j]
                tmp[i][j] = s
        for i in range(6):
            for j in range(6):
                s = self.zero()
                for k in range(6):
                    if T[k][i] is not None:
                        s = s + T[k][i] * tmp[k][j]
                out[i][j] = out[i][j] + s

    def reduce_vector(self, out, W, arm):
        x = cross(arm, W[:3])
        for i in range(3):
            out[i] = out[i] + W[i]
            out[3 + i] = out[3 + i] + (W[3 + i] + x[i])

    def geom_stiffness(self, out, W, arm0, arm, theta):
        """The stiffness from the variation of T (raft_fowt.py:1181-1192 with dT of :640-666)."""
        for j in range(3):
            th = list(theta)
            th[j] = th[j] + 1.0
            x = cross(th, arm)
            dA = [arm0[c] + x[c] - arm[c] for c in range(3)]
            H = self.H(dA)
            for i in range(3):
                out[3 + i][3 + j] = out[3 + i][3 + j] - (H[0][i] * W[0] + H[1][i] * W[1] + H[2][i] * W[2])

    @staticmethod
    def symmetrise(M):
        for i in range(6):
            for j in range(i + 1, 6):
                M[i][j] = M[j][i] = (M[i][j] + M[j][i]) / 2


def _evaluate(members, stations, caps, pose, rho, g, T, trim, Fz_moor, mass0, faults):
    mdl = _Model(T, faults)
    num = mdl.num
    nM = len(members)
    pose = np.zeros(6) if pose is None else np.asarray(pose, dtype=np.float64)
    rho_, g_ = num(rho), num(g)
    rP = [num(pose[i]) for i in range(3)]
    theta = [num(pose[3 + i]) for i in range(3)]
    st = [[[num(x) for x in row] for row in np.asarray(s, dtype=np.float64)] for s in stations]
    poses = [mdl.pose_member(members[m], pose) for m in range(nM)]
    static = [not (int(members[m][GM_FLAGS]) & FLAG_NOSTATIC) for m in range(nM)]
    drho = mdl.zero()
    if trim:                                                      # raft_model.py:1772-1827
        for rows in st:
            for row in rows:
                if row[GS_RHOFILL].v == 0:
                    row[GS_LFILL] = mdl.zero()                    # :1780-1787
        mass, V, vfill = num(mass0), mdl.zero(), mdl.zero()
        mark = len(mdl.decisions)
        for m in range(nM):
            if static[m]:
                In = mdl.inertia(members[m], st[m], caps[m], poses[m], g_, m)
                mass, vfill = mass + In.mass, vfill + In.vfill
                V = V + mdl.hydrostatics(members[m], st[m], poses[m], rho_, g_, m).V
        del mdl.decisions[mark:]                                  # the same decisions are taken again below
        if not mdl.decide("ballast volume > 0", bool(vfill.v > 0)):
            raise Refused("ballast trim needs some ballast volume")
        sumFz = -mass * g_ + V * rho_ * g_ + num(Fz_moor)         # :1791
        drho = sumFz / g_ / vfill                                 # :1805
        for rows in st:
            for row in rows:
                if row[GS_LFILL].v > 0:
                    row[GS_RHOFILL] = row[GS_RHOFILL] + drho      # :1810-1817
    recs, idx, amor, n_mcf = [], [], [], [0]
    Ch, Cs, Ms = mdl.zeros(6, 6), mdl.zeros(6, 6), mdl.zeros(6, 6)
    Chg, Csg = mdl.zeros(6, 6), mdl.zeros(6, 6)
    Wh, Ws = mdl.zeros(6), mdl.zeros(6)
    sumVr, sumMr, Vtot, AWPtot, vfill = mdl.zeros(3), mdl.zeros(3), mdl.zero(), mdl.zero(), mdl.zero()
    for m in range(nM):
        gm, P = members[m], poses[m]
        mdl.member_strips(gm, st[m], P, rP, rho_, m, recs, idx, amor, n_mcf)
        if not static[m]:
            continue
        arm = [P.rA[i] - rP[i] for i in range(3)]
        if mdl.faults.get("arm_rA0"):
            arm = [P.rA0[i] - rP[i] for i in range(3)]
        In = mdl.inertia(gm, st[m], caps[m], P, g_, m)
        mdl.reduce_matrix(Ms, In.M, arm)
        mdl.reduce_matrix(Cs, In.C, arm)
        mdl.reduce_vector(Ws, In.W, arm)
        mdl.geom_stiffness(Csg, In.W, P.rA0, arm, theta)
        for x in range(3):
            sumMr[x] = sumMr[x] + ((In.center[x] - P.rA[x]) + P.rA0[x]) * In.mass      # raft_fowt.py:902-903
        vfill = vfill + In.vfill
        Hy = mdl.hydrostatics(gm, st[m], P, rho_, g_, m)
        mdl.reduce_matrix(Ch, Hy.C, arm)
        mdl.reduce_vector(Wh, Hy.F, arm)
        mdl.geom_stiffness(Chg, Hy.F, P.rA0, arm, theta)
        Vtot, AWPtot = Vtot + Hy.V, AWPtot + Hy.AWP
        if mdl.decide("m%d: V > 0" % m, bool(Hy.V.v > 0)):        # :1006, raft_fowt.py:938
            for x in range(3):
                sumVr[x] = sumVr[x] + ((Hy.rcV[x] / Hy.V - P.rA[x]) + P.rA0[x]) * Hy.V
    for i in range(6):
        for j in range(6):
            Ch[i][j] = Ch[i][j] + Chg[i][j]
            Cs[i][j] = Cs[i][j] + Csg[i][j]
    for M in (Ch, Ms, Cs):
        mdl.symmetrise(M)
    props = mdl.zeros(SP_NGATED)
    props[SP_DRHO], props[SP_VFILL], props[SP_MASS], props[SP_V], props[SP_AWP] = drho, vfill, Ms[0][0], Vtot, AWPtot
    if mdl.decide("design mass != 0", bool(Ms[0][0].v != 0)):
        props[SP_RCG:SP_RCG + 3] = [sumMr[x] / Ms[0][0] for x in range(3)]
    if mdl.decide("design volume != 0", bool(Vtot.v != 0)):
        props[SP_RCB:SP_RCB + 3] = [sumVr[x] / Vtot for x in range(3)]
    vals = dict(strips=recs if recs else np.zeros((0, NGATED)), A_morison=mdl.morison(amor), C_hydro=Ch, W_hydro=Wh,
                M_struc=Ms, C_struc=Cs, W_struc=Ws, props=props)
    out = SimpleNamespace(decisions=mdl.decisions, idx=np.array(idx, dtype=np.float64).reshape(-1, 2), D={}, E={})
    for k, v in vals.items():
        a = np.array(v, dtype=object)
        out.D[k] = np.array([x.v for x in a.ravel()], dtype=T).reshape(a.shape) if a.dtype == object else a.astype(T)
        out.E[k] = np.array([x.e for x in a.ravel()], dtype=T).reshape(a.shape) if a.dtype == object else a.astype(T)
    return out


def design_reference(members, stations, caps, pose=None, rho=1025.0, g=9.81, dtype=np.longdouble, trim=False, Fz_moor=0.0,
                     mass0=0.0, faults=None):
    """One design: ``members`` [nM,16], ``stations`` / ``caps`` lists of [n,16] / [ncap,4] per member, ``pose`` [6].
    ``trim``: the ballast trim first, with the mass ``mass0`` that is not geometry and ``Fz_moor``.  Returns a namespace
    with D[name], E[name] for 'strips' [S,26] and the seven statics, ``idx`` [S,2] (member, strip index: exact) and the
    recorded discontinuous ``decisions``.  Raises ``Refused`` where the reference procedure fails."""
    members = np.asarray(members, dtype=np.float64).reshape(-1, 16)
    caps = [np.zeros((0, 4))] * len(members) if caps is None else [np.asarray(c, dtype=np.float64).reshape(-1, 4) for c in caps]
    with np.errstate(all="ignore"):
        return _evaluate(members, stations, caps, pose, rho, g, dtype, trim, Fz_moor, mass0, faults)


def design_firmness(*args, **kw):
    """The disagreements between the discontinuous decisions taken in fp64 and in longdouble: [] for a firm design."""
    a = design_reference(*args, dtype=np.float64, **kw).decisions
    b = design_reference(*args, dtype=np.longdouble, **kw).decisions
    if len(a) != len(b):
        return [("number of decisions", len(a), len(b))]
    return [(ta, oa, ob) for (ta, oa), (tb, ob) in zip(a, b) if ta != tb or oa != ob]


def gate_multiples(x, D, E):
    """|x - D| / (eps E) per entry; entries with E == 0 give 0 where x is exactly 0 and inf otherwise; where the
    reference is NaN the entry gives 0 if x is NaN too and inf otherwise.  No entry is left out."""
    x, D, E = (np.asarray(a, dtype=np.longdouble) for a in (x, D, E))
    assert x.shape == D.shape == E.shape, (x.shape, D.shape, E.shape)
    out = np.full(D.shape, np.inf)
    nan = np.isnan(D)
    out[nan & np.isnan(x)] = 0.0
    zero = ~nan & (E == 0)
    out[zero & (x == 0)] = 0.0
    ok = ~nan & ~zero & np.isfinite(x)
    out[ok] = (np.abs(x[ok] - D[ok]) / (EPS * E[ok])).astype(np.float64)
    return out
