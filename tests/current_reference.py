"""Independent evaluation of the mean current loads (raft_member.py:1846-1896 summed as raft_fowt.py:1976-1983) from a
packed strip table: the reference of tests/test_current.py and tests/test_hip_current.py.

``current_loads(strips, off, ...)`` walks the 32-double records of include/raftx.h in ``numpy.longdouble`` (or in plain
fp64 with ``dtype=np.float64``: the host restatement the gate's constant is measured with) and returns

    D [nD,nCur,6]   the loads about the reduced-DOF point, and
    E [nD,nCur,6]   the envelope: the sum over the strips of the absolute value of every addend -- for a force
                    component |Dq| + |Dend| + |Dp1| + |Dp2|, for a moment component |a_y D_z| + |a_z D_y| (cyclically).

The accuracy gate is |x - D| <= C eps E per entry; where E == 0 the result must be exactly 0.
Nothing here is shared with raft_amd or the kernels: plain loops over strips and currents.
"""
import numpy as np

F_X, F_AX, F_Q, F_P1, F_P2 = 0, 3, 6, 9, 12
F_DQ, F_DP1, F_DP2, F_DEND, F_CIRC = 19, 20, 21, 22, 23
NFIELD = 32
EPS = float(np.finfo(np.float64).eps)

GATE_C = 128         # 16 x the worst CPU-side multiple (6.5) over tests/golden/refgold_current.npz, rounded up to a power of two: DESIGN.md section 4


def _norm(v):
    return np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def current_loads(strips, off, speed, heading_deg, depth, Zref=None, shearExp=0.12, dtype=np.longdouble):
    """D, E [nD,nCur,6] (in ``dtype``) of the designs ``off`` [nD+1] of ``strips`` [nS,32]."""
    T = dtype
    strips = np.asarray(strips, dtype=np.float64).reshape(-1, NFIELD)
    off = np.asarray(off, dtype=np.int64)
    nD = len(off) - 1
    speed = np.atleast_1d(np.asarray(speed, dtype=np.float64))
    heading = np.broadcast_to(np.asarray(heading_deg, dtype=np.float64), speed.shape)
    nC = len(speed)
    Zref = np.zeros(nD) if Zref is None else np.broadcast_to(np.asarray(Zref, dtype=np.float64), (nD,))
    c_drag = T(np.sqrt(8 / np.pi))                           # the fp64 constant the table was scaled with
    D = np.zeros((nD, nC, 6), dtype=T)
    E = np.zeros((nD, nC, 6), dtype=T)
    with np.errstate(invalid="ignore"):
        for d in range(nD):
            for c in range(nC):
                rad = T(np.deg2rad(heading[c]))                  # :1848: the angle is the fp64 np.deg2rad(heading)
                ch, sh = np.cos(rad), np.sin(rad)
                for rec in strips[off[d]:off[d + 1]]:
                    r = rec.astype(T)
                    z = r[F_X + 2]
                    if not z < 0:
                        continue
                    v = T(speed[c]) * ((T(depth) - abs(z)) / (T(depth) + T(Zref[d]))) ** T(shearExp)
                    vcur = np.array([v * ch, v * sh, T(0)], dtype=T)
                    q, p1, p2, a = r[F_Q:F_Q + 3], r[F_P1:F_P1 + 3], r[F_P2:F_P2 + 3], r[F_AX:F_AX + 3]
                    vq = np.sum(vcur * q) * q
                    vp = vcur - vq
                    vp1 = np.sum(vcur * p1) * p1
                    vp2 = np.sum(vcur * p2) * p2
                    if r[F_CIRC] != 0:
                        n1 = n2 = _norm(vp)
                    else:
                        n1, n2 = _norm(vp1), _norm(vp2)
                    Dq = r[F_DQ] / c_drag * _norm(vq) * vq
                    Dp1 = r[F_DP1] / c_drag * n1 * vp1
                    Dp2 = r[F_DP2] / c_drag * n2 * vp2
                    De = r[F_DEND] / c_drag * _norm(vq) * vq
                    F = Dq + Dp1 + Dp2 + De
                    D[d, c, :3] += F
                    E[d, c, :3] += abs(Dq) + abs(De) + abs(Dp1) + abs(Dp2)
                    D[d, c, 3] += a[1] * F[2] - a[2] * F[1]
                    D[d, c, 4] += a[2] * F[0] - a[0] * F[2]
                    D[d, c, 5] += a[0] * F[1] - a[1] * F[0]
                    E[d, c, 3] += abs(a[1] * F[2]) + abs(a[2] * F[1])
                    E[d, c, 4] += abs(a[2] * F[0]) + abs(a[0] * F[2])
                    E[d, c, 5] += abs(a[0] * F[1]) + abs(a[1] * F[0])
    return D, E


def gate_multiples(x, D, E):
    """|x - D| / (eps E) per entry; entries with E == 0 give 0 where x is exactly 0 and inf otherwise; where the
    reference is NaN the entry gives 0 if x is NaN too and inf otherwise.  No entry is left out."""
    x, D, E = (np.asarray(a, dtype=np.longdouble) for a in (x, D, E))
    out = np.full(D.shape, np.inf)
    nan = np.isnan(D)
    out[nan & np.isnan(x)] = 0.0
    zero = ~nan & (E == 0)
    out[zero & (x == 0)] = 0.0
    ok = ~nan & ~zero & np.isfinite(x)
    out[ok] = (np.abs(x[ok] - D[ok]) / (EPS * E[ok])).astype(np.float64)
    return out
