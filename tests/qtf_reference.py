"""Extended-precision references of the second-order path (raftx_qtf_slender[_rows], raftx_qtf_kay, raftx_qtf_force),
each with the NON-CANCELLING envelope of what it sums, in numpy.longdouble / numpy.clongdouble:

    qtf_slender_ref   oracle/qtf_oracle.py evaluated in clongdouble (its dtype parameter), inputs promoted exactly
    kay_ref           Member.correction_KAY (raft/raft_member.py:1676-1791) per item record of raft_amd.qtf.kay_items,
                      with sinh / cosh / tanh directly and J_n, Y_n from tests/golden/kay_hankel_ref.npz (mpmath, 50 digits)
    qtf_force_ref     FOWT.calcHydroForce_2ndOrd, interpMode 'qtf' (raft/raft_fowt.py:2209-2245), from the rules in the
                      header comment of raftx_qtf_force: bilinear interpolation, zero outside the grid, the one-bin shift

The bound every implementation is held to is  |x - ref| <= C eps E  entry by entry, eps = 2^-52, E the envelope; where
E == 0 the result has to be exactly 0.  ``used`` returns max |x - ref| / (eps E), i.e. the share of C in units of C = 1.

The module also builds the Kim & Yue input sets (kay_grid, kay_geometry): the generator of the Bessel fixture
(oracle/make_kay_hankel.py) and the tests take their arguments x = k R from the same place."""
import os

import numpy as np

from oracle import qtf_oracle

LD, CLD = np.longdouble, np.clongdouble
EPS = 2.0 ** -52                                       # of the fp64 arithmetic under test
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kay_hankel_ref.npz")
N_ORDER = 13                                           # J_n, Y_n for n = 0 .. 12 (Nm = 10 needs H'_11, i.e. H_12)


def _extended():
    eps = np.finfo(LD).eps
    assert eps <= 2.0 ** -63, "numpy.longdouble is no wider than fp64 here (eps = %g): no independent reference" % eps


def used(x, ref, env):
    """max over the entries of |x - ref| / (eps env); an entry with env == 0 has to be exactly zero (else inf)."""
    err = np.abs(np.asarray(x).astype(ref.dtype) - ref)
    env = np.asarray(env, dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(env > 0, err / (LD(EPS) * env), np.where(err == 0, LD(0), LD(np.inf)))
    return float(np.max(f)) if f.size else 0.0


# ---------------------------------------------------------------------------------------------- slender body
def qtf_slender_ref(tab, Xi, beta, w, k, h, rho, g, M_struc, kay=None):
    """(qtf, E) [nw,nw,6]: oracle.qtf_oracle.qtf_slender_body in clongdouble and its envelope."""
    _extended()
    kay = None if kay is None else np.asarray(kay, dtype=CLD)
    return qtf_oracle.qtf_slender_body(tab, np.asarray(Xi, dtype=CLD), beta, w, k, h, rho, g, M_struc, kay, dtype=CLD,
                                       return_envelope=True)


# ---------------------------------------------------------------------------------------------- Kim & Yue
KAY_DEPTH = 50.0
KAY_X_SPECIAL = (1.0, 2.0, 3.0, 5.0, 8.0, 10.0, 12.0)     # x = k R of the large column (R = 4) at libm's branch points
KAY_R = (4.0, 0.5)                                         # x from 8e-3 to 12 and from 1e-3 to 1.5
KAY_NW_MASTER = 129


def kay_grid(nw2, g=9.81, h=KAY_DEPTH):
    """(w, k) of nw2 bins out of ONE master grid of 129 wave numbers: log-spaced 2e-3 .. 3 1/m plus k = x / 4 for the x of
    KAY_X_SPECIAL (exact in binary, so that k R is exactly 2, 8, n).  Every smaller grid is a subset that keeps the
    special points, so the fixture holds J_n, Y_n at 129 arguments per radius."""
    special = np.array(KAY_X_SPECIAL[:-1]) / KAY_R[0]
    k = np.unique(np.concatenate([np.geomspace(2e-3, KAY_X_SPECIAL[-1] / KAY_R[0], KAY_NW_MASTER - len(special)), special]))
    assert len(k) == KAY_NW_MASTER and k[-1] * KAY_R[0] == 12.0
    keep = list(np.nonzero(np.isin(k, np.concatenate([special, k[[0, -1]]])))[0])
    if nw2 == 1:
        keep = [int(np.nonzero(k == 0.5)[0][0])]                                   # x = 2 exactly
    for i in list(np.round(np.linspace(0, KAY_NW_MASTER - 1, nw2)).astype(int)) + list(range(KAY_NW_MASTER)):
        if len(keep) >= nw2:
            break
        if i not in keep:
            keep.append(int(i))
    k = k[np.sort(np.array(keep[:nw2]))]
    w = np.sqrt(g * k * np.tanh(k * h))
    assert len(k) == nw2 and np.all(np.diff(w) > 0)
    return w, k


def _column(x, y, z_nodes, R, tilt=0.0):
    """kay_geom record of one MacCamy-Fuchs column through (x, y, 0) with strip nodes at z_nodes"""
    z = np.asarray(z_nodes, dtype=float)
    r = np.stack([x + tilt * z, y + 0.0 * z, z], axis=1)
    q = np.array([tilt, 0.0, 1.0]) / np.hypot(tilt, 1.0)
    p1 = np.cross(np.array([0.0, 1.0, 0.0]), q)
    p1 /= np.linalg.norm(p1)
    return dict(rA=r[0], rB=r[-1], r=r, ds=np.full(len(z), 2.0 * R), dls=np.ones(len(z)), p1=p1, p2=np.cross(q, p1))


def kay_geometry(which):
    """'two': two members in one set -- a large column (waterline item + two segment items, R = 4) and a slender tilted one
    (waterline item + one segment, R = 0.5);  'wl': the large column with a single strip node, which kay_items turns
    into ONE waterline item and no segment;  'below' / 'mid' / 'above': the large column (waterline item + one segment)
    with R one ulp below 4, 4, one ulp above 4;  'none': no member."""
    if which == "two":
        return [_column(5.0, -3.0, [-20.0, -8.0, 4.0, 10.0], KAY_R[0]), _column(-12.0, 7.0, [-6.0, 3.0], KAY_R[1], tilt=0.1)]
    if which == "none":
        return []
    if which == "wl":
        col = _column(5.0, -3.0, [-20.0, 4.0], KAY_R[0])
        col.update(r=col["r"][:1], ds=col["ds"][:1], dls=col["dls"][:1])         # rA, rB still cross the waterline
        return [col]
    R = {"mid": KAY_R[0], "below": np.nextafter(KAY_R[0], 0.0), "above": np.nextafter(KAY_R[0], 8.0)}[which]
    return [_column(5.0, -3.0, [-20.0, 4.0], R)]


KAY_BRANCH_K = np.array([0.25, 0.5, 2.0, 3.0])             # with R = 4 -+ 1 ulp: x within one ulp of 1, 2, 8, 12


def kay_fixture_arguments():
    """Every x = k R (float64 product, as the kernel forms it) the Kim & Yue tests evaluate J_n, Y_n at."""
    _, k = kay_grid(KAY_NW_MASTER)
    xs = [k * R for R in KAY_R]
    xs += [KAY_BRANCH_K * R for R in (np.nextafter(KAY_R[0], 0.0), np.nextafter(KAY_R[0], 8.0))]
    return np.unique(np.concatenate(xs))


_bessel = {}


def bessel(x):
    """(J, Y) [len(x), 13] in longdouble at the float64 arguments x, from the fixture; x must be stored bit for bit."""
    if not _bessel:
        with np.load(GOLDEN) as z:
            _bessel["x"] = z["x"]
            _bessel["J"] = z["J_hi"].astype(LD) + z["J_lo"].astype(LD)
            _bessel["Y"] = z["Y_hi"].astype(LD) + z["Y_lo"].astype(LD)
    x = np.ascontiguousarray(x, dtype=np.float64)
    i = np.clip(np.searchsorted(_bessel["x"], x), 0, len(_bessel["x"]) - 1)
    assert np.array_equal(_bessel["x"][i].view(np.uint64), x.view(np.uint64)), "argument not in tests/golden/kay_hankel_ref.npz"
    return _bessel["J"][i], _bessel["Y"][i]


def kay_ref(items, w, k, beta, h, rho, g, Nm):
    """(table, envelope) [nw,nw,6] of one set: sum over its item records (raft_amd.qtf.kay_items) of Member.correction_KAY.
    Envelope: sum over items, orders n and the two halves of Omega_n of |coefficient x half x weight_n| (before Re(2i .)
    is taken), carried to the six DOFs with |pforce_j| and, for the moments, |arm_a| |pforce_b| per product."""
    _extended()
    nw = len(w)
    wl, kl = np.asarray(w, dtype=LD), np.asarray(k, dtype=LD)
    h, rho, g, beta = LD(h), LD(rho), LD(g), LD(beta)
    pi = LD(4) * np.arctan(LD(1))
    out = np.zeros((nw, nw, 6), dtype=CLD)
    env = np.zeros((nw, nw, 6), dtype=LD)
    w1, w2, k1, k2 = wl[:, None], wl[None, :], kl[:, None], kl[None, :]
    same = w1 == w2
    k1h, k2h = k1 * h, k2 * h
    pre = k1h * k2h / np.sqrt(k1h * np.tanh(k1h)) / np.sqrt(k2h * np.tanh(k2h)) / np.cosh(k1h) / np.cosh(k2h)
    for rec in np.asarray(items, dtype=np.float64).reshape(-1, 12):
        R64, seg = rec[0], rec[1] != 0.0
        R, z1, z2 = LD(rec[0]), LD(rec[2]), LD(rec[3])
        arm, pf = rec[4:7].astype(LD), rec[7:10].astype(LD)
        J, Y = bessel(np.asarray(k, dtype=np.float64) * R64)
        H = J + CLD(1j) * Y                                                     # [nw, 13]
        Hm = np.concatenate([-H[:, 1:2], H], axis=1)                           # orders -1 .. 12; H_-1 = -H_1
        inv = 1 / (LD(0.5) * (Hm[:, 0:Nm + 2] - Hm[:, 2:Nm + 4]))               # 1 / H'_n, n = 0 .. Nm+1
        x1, x2 = k1 * R, k2 * R
        coef = rho * g * R * 2 / pi / (x1 * x2)                                # times i
        if seg:
            def shs(z, sign):
                d = k1 + sign * k2
                with np.errstate(divide="ignore", invalid="ignore"):
                    v = np.sinh(d * (z + h)) / (d * h)
                return np.where(same, (z + h) / h, v) if sign < 0 else v
            sp2, sp1, sm2, sm1 = shs(z2, 1), shs(z1, 1), shs(z2, -1), shs(z1, -1)
            Im = LD(0.5) * (sp2 - sm2 - sp1 + sm1)
            Ip = LD(0.5) * (sp2 + sm2 - sp1 - sm1)
        S = np.zeros((nw, nw), dtype=CLD)
        eS = np.zeros((nw, nw), dtype=LD)
        for n in range(Nm + 1):
            A = inv[:, None, n + 1] * np.conj(inv[None, :, n])
            B = inv[:, None, n] * np.conj(inv[None, :, n + 1])
            wgt = pre * (Im + Ip * (n * (n + 1)) / x1 / x2) if seg else LD(-1)
            S = S + CLD(1j) * coef * (A - B) * wgt
            eS = eS + np.abs(coef * wgt) * (np.abs(A) + np.abs(B))
        xi = np.cos(beta) * LD(rec[10]) + np.sin(beta) * LD(rec[11])
        Fs = S.real * np.exp(CLD(-1j) * ((k1 - k2) * xi))
        g6 = np.concatenate([pf, np.cross(arm, pf)])
        a, p = np.abs(arm), np.abs(pf)
        e6 = np.concatenate([p, [a[1] * p[2] + a[2] * p[1], a[2] * p[0] + a[0] * p[2], a[0] * p[1] + a[1] * p[0]]])
        out += Fs[:, :, None] * g6
        env += eS[:, :, None] * e6
    out = np.where((k1 < k2)[:, :, None], np.conj(out), out)
    up = (w2 >= w1)[:, :, None]
    return np.where(up, out, 0), np.where(up, env, 0)


# ---------------------------------------------------------------------------------------------- second-order force
def qtf_force_ref(qtf, w2, w, dw, S0):
    """(f [6,nw], f_mean [6], env_mean [6]) of one set; env_mean = 2 dw sum_i |S0_i| |Re Q_j(w_i, w_i)|."""
    _extended()
    q = np.asarray(qtf, dtype=CLD)
    w2, w, S, dw = np.asarray(w2, dtype=LD), np.asarray(w, dtype=LD), np.asarray(S0, dtype=LD), LD(dw)
    n2, nw = len(w2), len(w)
    i = np.clip(np.searchsorted(w2, w, side="left") - 1, 0, n2 - 2)            # interval [w2_i, w2_i+1] of every bin
    t = (w - w2[i]) / (w2[i + 1] - w2[i])
    inside = (w >= w2[0]) & (w <= w2[-1])
    ia, ib, ta, tb = i[:, None], i[None, :], t[:, None, None], t[None, :, None]
    Q = (1 - ta) * (1 - tb) * q[ia, ib] + (1 - ta) * tb * q[ia, ib + 1] + ta * (1 - tb) * q[ia + 1, ib] + ta * tb * q[ia + 1, ib + 1]
    Q = np.where((inside[:, None] & inside[None, :])[:, :, None], Q, 0)        # [nw,nw,6]
    P = (S[:, None] * S[None, :])[:, :, None] * (Q.real * Q.real + Q.imag * Q.imag)
    f = np.zeros((6, nw), dtype=LD)
    for mu in range(1, nw):
        f[:, mu - 1] = 4 * np.sqrt(np.trace(P, offset=mu, axis1=0, axis2=1)) * dw      # stored one bin lower (:2241-2245)
    d = np.diagonal(Q.real, axis1=0, axis2=1)                                   # [6,nw]
    return f, 2 * (S * d).sum(axis=1) * dw, 2 * (np.abs(S) * np.abs(d)).sum(axis=1) * dw
