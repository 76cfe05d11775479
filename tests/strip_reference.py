"""Independent evaluation of the first-order Morison strip sweeps from a packed strip table: the reference of
tests/test_strip_reference.py and tests/test_hip_strip_reference.py.

``strip_sweep(strips, cm, w, k, depth, rho, g, zeta, beta, Xi)`` walks the 32-double records of include/raftx.h (and the
MacCamy-Fuchs ``Cm`` rows [nRows,2,nw] of the design) for ONE design and ONE sea state in ``numpy.longdouble`` /
``clongdouble`` (or in plain fp64 with ``dtype=np.float64``: the host restatement the gate's constant is measured with)
and returns, each with its envelope ``*_E`` and its dust array ``*_D``,

    u, ud [nHead,S,3,nw], pDyn [nHead,S,nw]   wave kinematics per strip                         helpers.py:188-236
    F_iner [nHead,6,nw]                       inertial excitation about the reduced-DOF point   raft_member.py:1965-1991
    Bmat [S,3,3], B_drag [6,6]                the drag linearisation about Xi [6,nw], heading 0 raft_member.py:2039-2118
    F_exc [nHead,S,3,nw], F_drag [nHead,6,nw] Bmat u of every heading, and its 3 -> 6 sum       raft_member.py:2122-2152

The branch decisions of the kinematics (``k == 0``, ``k*h > 89.4``) are taken in fp64 exactly as helpers.py:211-218
writes them; only the arithmetic after the decision is extended.  A table holds WET strips only (z < 0): that is the
ABI's contract (raft_amd/strips.py keeps ``r[:,2] < 0``, raft_member.py:1979,2058) and the oracle's; a strip with z > 0
gets the zero kinematics of helpers.py:206 here, and no library is asked about one.

Envelope.  ``E`` is the sum of the absolute values of EVERY addend of an entry -- the 3x3 products of Imat ud and Bmat u
term by term (one per unit-vector dyad), the pressure term, each product of the 3 -> 6 translation (an arm component
times the ENVELOPE of the force component: an error of the force is bounded by its envelope, not by its value) -- each
strip's addends weighted by ``1 + kappa + n_s``:

    kappa = |k| (|x cos beta| + |y sin beta| + |z|)   the conditioning of the phase and decay arguments: an fp64
                                                      evaluation cannot do better than kappa eps on a strip's term;
    n_s   = an upper bound on the unit rotor steps since the run start of a library that advances the kinematics along
            straight members: 2 x the strip's index inside its streak of consecutive strips with bit-equal q, capped at
            126 (a run is a sub-streak of at most 64 strips with at most 2 units per step, so this never undercounts).

The drag coefficients go through vRMS = sqrt(0.5 sum |v|^2): with env_j = (1 + kappa + n_s)|u_j| + sum |addends of the
node velocity_j| per component and bin, propagated through the projections on q, p1, p2 by the triangle inequality,
vRMS_env = sqrt(0.5 sum env^2) >= vRMS (2-norm triangle inequality), and Bmat, B_drag, F_drag use vRMS_env.

``shallow=True`` (a derived weight): in the finite-depth branch a library that builds
sinh k(z+h) / sinh kh from decaying exponentials, (e^{kz} - e^{-k(z+2h)}) / (1 - e^{-2kh}), loses coth k(z+h) <= 1 +
1/(k(z+h)) on the difference (the denominator is an expm1: no loss); the addends that carry Sh (the vertical velocity and
acceleration) are then weighted by (1 + kappa + n_s) coth k(z+h).

``ratio_form=True`` (the conditioning of helpers.py:219-222 AS WRITTEN): an fp64 evaluation of sinh k(z+h) / sinh kh rounds
the two arguments separately, each as large as k h however shallow the strip, so the weight of a strip's addends in the
finite-depth branch is 1 + kappa + n_s + k (2h + z).  The recorded values of the live reference, the oracle library and the
fp64 mode of this file are of that form and are measured with it; the rotor-scheme model and the device, which work with
e^{kz} and e^{-k(z+2h)}, are held to the plain weight.

Dust.  A library may leave out products with a unit-vector component below 1e-15 (the rounding dust of a member's
rotation matrix): any addend with a factor 0 < |component| < 1e-15 ALSO adds its full (unweighted) magnitude to ``D``.

Gate (``gate_multiples``), no entry left out:  |x - ref| <= C eps E + 2 D;  where E == 0 the result must be exactly 0
(bins with zeta == 0 are such entries); where the reference is NaN the result must be NaN.

Nothing here is shared with raft_amd or the kernels.
"""
from types import SimpleNamespace

import numpy as np

F_X, F_AX, F_Q, F_P1, F_P2 = 0, 3, 6, 9, 12
F_IQ, F_IP1, F_IP2, F_AI = 15, 16, 17, 18
F_DQ, F_DP1, F_DP2, F_DEND, F_CIRC, F_MCF, F_RHOV = 19, 20, 21, 22, 23, 24, 25
NFIELD = 32
EPS = float(np.finfo(np.float64).eps)
DUST = 1e-15

# C = the worst CPU-side multiple x 16, rounded up to a power of two; the host implementations stay inside C / 4.
# Measured by tests/test_strip_reference.py (figures: DESIGN.md section 4).
GATE_C = 128          # sums and per-strip envelopes: F_iner, B_drag, F_drag, Bmat, F_exc (worst CPU multiple 4.69: F_iner of the rotor model on two 64-strip vertical columns)
GATE_CK = 64          # single terms, relative: u, ud, pDyn (worst CPU multiple 3.19: ud of the model's exponential form)


def _ctype(T):
    return np.clongdouble if T is np.longdouble else np.complex128


def run_steps(strips):
    """n_s [S]: 2 x the index of a strip inside its streak of consecutive strips with bit-equal q, capped at 126."""
    strips = np.asarray(strips, dtype=np.float64).reshape(-1, NFIELD)
    n = np.zeros(len(strips))
    for s in range(1, len(strips)):
        if np.array_equal(strips[s, F_Q:F_Q + 3], strips[s - 1, F_Q:F_Q + 3]):
            n[s] = n[s - 1] + 1
    return np.minimum(2 * n, 126.0)


def wave_kinematics(strips, w, k, depth, rho, g, zeta, beta, dtype=np.longdouble, shallow=False, ratio_form=False):
    """helpers.py:188-236 for every (heading, strip, bin).  Returns u, ud [nHead,S,3,nw], pDyn [nHead,S,nw] and the
    weights W [nHead,S,nw] = 1 + kappa + n_s, Wz (W, or W coth k(z+h) in the finite-depth branch with ``shallow``)."""
    T, CT = dtype, _ctype(dtype)
    strips = np.asarray(strips, dtype=np.float64).reshape(-1, NFIELD)
    w64, k64 = np.asarray(w, dtype=np.float64), np.asarray(k, dtype=np.float64)
    zeta = np.asarray(zeta, dtype=np.float64).reshape(-1, len(w64))
    beta = np.asarray(beta, dtype=np.float64).reshape(-1)
    nH, S, nw = len(beta), len(strips), len(w64)
    k0 = k64 == 0.0                                            # helpers.py:211, in fp64 as written
    deep = ~k0 & (k64 * np.float64(depth) > 89.4)              # helpers.py:215
    fin = ~k0 & ~deep
    wT, kT, h = w64.astype(T), k64.astype(T), T(depth)
    x, y, z = (strips[:, F_X + j].astype(T)[:, None] for j in range(3))
    Sh, Ch, Cc = (np.zeros((S, nw), dtype=T) for _ in range(3))
    coth = np.ones((S, nw), dtype=T)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        Sh[:, k0], Ch[:, k0], Cc[:, k0] = T(1), T(99999), T(99999)
        kd = kT[deep]
        Sh[:, deep] = np.exp(kd * z)
        Ch[:, deep] = np.exp(kd * z)
        Cc[:, deep] = np.exp(kd * z) + np.exp(-kd * (z + 2 * h))
        kf = kT[fin]
        Sh[:, fin] = np.sinh(kf * (z + h)) / np.sinh(kf * h)
        Ch[:, fin] = np.cosh(kf * (z + h)) / np.sinh(kf * h)
        Cc[:, fin] = np.cosh(kf * (z + h)) / np.cosh(kf * h)
        if shallow:
            coth[:, fin] = np.abs(np.cosh(kf * (z + h)) / np.sinh(kf * (z + h)))
    wet = (strips[:, F_X + 2] <= 0)[:, None]                   # helpers.py:206
    u = np.zeros((nH, S, 3, nw), dtype=CT)
    pDyn = np.zeros((nH, S, nw), dtype=CT)
    W = np.zeros((nH, S, nw), dtype=T)
    ns = run_steps(strips).astype(T)[:, None]
    for ih in range(nH):
        b = T(beta[ih])
        cb, sb = np.cos(b), np.sin(b)
        ph = kT * (cb * x + sb * y)
        zc = zeta[ih].astype(T) * (np.cos(ph) - CT(1j) * np.sin(ph))          # zeta0 e^{-i k (x cos beta + y sin beta)}
        zc = np.where(wet, zc, CT(0))
        u[ih, :, 0] = wT * zc * Ch * cb
        u[ih, :, 1] = wT * zc * Ch * sb
        u[ih, :, 2] = CT(1j) * wT * zc * Sh
        pDyn[ih] = T(rho) * T(g) * zc * Cc
        W[ih] = 1 + np.abs(kT) * (np.abs(x * cb) + np.abs(y * sb) + np.abs(z)) + ns
        if ratio_form:
            W[ih][:, fin] += kT[fin] * np.abs(2 * h + z)
    ud = CT(1j) * wT * u
    return u, ud, pDyn, W, W * coth[None]


def _dusty(c):
    return 0.0 < abs(float(c)) < DUST


def _translate(F3, E3, D3, r):
    """helpers.py:468-483 with envelopes: [.., 3, nw] -> [.., 6, nw]."""
    F6 = np.concatenate([F3, np.stack([r[1] * F3[..., 2, :] - r[2] * F3[..., 1, :],
                                       r[2] * F3[..., 0, :] - r[0] * F3[..., 2, :],
                                       r[0] * F3[..., 1, :] - r[1] * F3[..., 0, :]], axis=-2)], axis=-2)
    a = np.abs(r)
    out = [F6]
    for X in (E3, D3):
        out.append(np.concatenate([X, np.stack([a[1] * X[..., 2, :] + a[2] * X[..., 1, :],
                                                a[2] * X[..., 0, :] + a[0] * X[..., 2, :],
                                                a[0] * X[..., 1, :] + a[1] * X[..., 0, :]], axis=-2)], axis=-2))
    return out


def _matvec(terms, vec, avec, Wv, T, CT):
    """sum over dyad terms (coef, v) of coef v_a v_b vec_b: value, envelope (addends weighted by Wv[b]) and dust.
    vec, avec = |vec|, Wv: [nHead,3,nw]; coef scalar or [nw]."""
    nH, _, nw = vec.shape
    F = np.zeros((nH, 3, nw), dtype=CT)
    E = np.zeros((nH, 3, nw), dtype=T)
    D = np.zeros((nH, 3, nw), dtype=T)
    for coef, v in terms:
        ac = np.abs(coef)
        for a in range(3):
            for b in range(3):
                d = v[a] * v[b]
                F[:, a] += coef * d * vec[:, b]
                mag = ac * abs(d) * avec[:, b]
                E[:, a] += mag * Wv[:, b]
                if _dusty(v[a]) or _dusty(v[b]):
                    D[:, a] += mag
    return F, E, D


def strip_sweep(strips, cm, w, k, depth, rho, g, zeta, beta, Xi=None, dtype=np.longdouble, shallow=False, kin=None,
                keep_strips=True, ratio_form=False):
    """One design under one sea state (zeta [nHead,nw], beta [nHead]); see the module docstring.  ``kin`` = (u, ud, pDyn)
    replaces the exact kinematics (tests/strip_device_model.py: what a rotor scheme costs downstream); ``Xi`` None skips the
    linearisation."""
    T, CT = dtype, _ctype(dtype)
    strips = np.asarray(strips, dtype=np.float64).reshape(-1, NFIELD)
    w64 = np.asarray(w, dtype=np.float64)
    nw, S = len(w64), len(strips)
    zeta = np.asarray(zeta, dtype=np.float64).reshape(-1, nw)
    nH = len(zeta)
    u, ud, pDyn, W, Wz = wave_kinematics(strips, w, k, depth, rho, g, zeta, beta, dtype=dtype, shallow=shallow,
                                         ratio_form=ratio_form)
    if kin is not None:
        u, ud, pDyn = (np.asarray(a).astype(CT) for a in kin)
    out = SimpleNamespace(u=u, ud=ud, pDyn=pDyn, W=W, Wz=Wz)
    Wv = np.stack([W, W, Wz], axis=2)                            # per component of u / ud: [nHead,S,3,nw]
    au, aud, ap = np.abs(u), np.abs(ud), np.abs(pDyn)
    wT = w64.astype(T)

    # ---- inertial excitation, raft_member.py:1965-1991
    Fi, Ei, Di = (np.zeros((nH, 6, nw), dtype=t) for t in (CT, T, T))
    for s in range(S):
        rec = strips[s].astype(T)
        q, p1, p2, r = rec[F_Q:F_Q + 3], rec[F_P1:F_P1 + 3], rec[F_P2:F_P2 + 3], rec[F_AX:F_AX + 3]
        mcf = int(strips[s, F_MCF])
        terms = [(rec[F_IQ], q)]                                 # Imat_end, :1442
        if mcf >= 0:                                             # :1420, 1446: rho v (Cm_p1 p1 p1^T + Cm_p2 p2 p2^T)
            c = np.asarray(cm)[mcf].astype(CT)
            terms += [(rec[F_RHOV] * c[0], p1), (rec[F_RHOV] * c[1], p2)]
        else:                                                    # Imat_sides, :1423
            terms += [(rec[F_IP1], p1), (rec[F_IP2], p2)]
        F3, E3, D3 = _matvec(terms, ud[:, s], aud[:, s], Wv[:, s], T, CT)
        for a in range(3):                                       # + pDyn a_i q, :1988
            F3[:, a] += pDyn[:, s] * rec[F_AI] * q[a]
            mag = ap[:, s] * abs(rec[F_AI] * q[a])
            E3[:, a] += mag * W[:, s]
            if _dusty(q[a]):
                D3[:, a] += mag
        F6, E6, D6 = _translate(F3, E3, D3, r)                   # :1991
        Fi += F6
        Ei += E6
        Di += D6
    out.F_iner, out.F_iner_E, out.F_iner_D = Fi, Ei, Di
    if Xi is None:
        return out

    # ---- drag linearisation about Xi, heading 0: raft_member.py:2039-2118, helpers.py:178-181, 396-402
    Xi = np.asarray(Xi, dtype=np.complex128).reshape(6, nw).astype(CT)
    aX = np.abs(Xi)
    Bmat, Bmat_E, Bmat_D = (np.zeros((S, 3, 3), dtype=T) for _ in range(3))
    Bd, Bd_E, Bd_D = (np.zeros((6, 6), dtype=T) for _ in range(3))
    Fd, Fd_E, Fd_D = (np.zeros((nH, 6, nw), dtype=t) for t in (CT, T, T))
    Fx, Fx_E, Fx_D = (np.zeros((nH, S, 3, nw), dtype=t) if keep_strips else None for t in (CT, T, T))
    for s in range(S):
        rec = strips[s].astype(T)
        q, p1, p2, r = rec[F_Q:F_Q + 3], rec[F_P1:F_P1 + 3], rec[F_P2:F_P2 + 3], rec[F_AX:F_AX + 3]
        th = Xi[3:]
        dr = [Xi[0] + (-th[2] * r[1] + th[1] * r[2]), Xi[1] + (th[2] * r[0] - th[0] * r[2]),
              Xi[2] + (-th[1] * r[0] + th[0] * r[1])]
        adr = [aX[0] + aX[5] * abs(r[1]) + aX[4] * abs(r[2]), aX[1] + aX[5] * abs(r[0]) + aX[3] * abs(r[2]),
               aX[2] + aX[4] * abs(r[0]) + aX[3] * abs(r[1])]
        vrel = [u[0, s, j] - CT(1j) * wT * dr[j] for j in range(3)]                 # :2075
        env = [Wv[0, s, j] * au[0, s, j] + wT * adr[j] for j in range(3)]

        def project(v):
            """sum |(vrel . v) v_j|^2, its envelope squared and the dust part of the envelope squared"""
            pr = vrel[0] * v[0] + vrel[1] * v[1] + vrel[2] * v[2]
            pe = env[0] * abs(v[0]) + env[1] * abs(v[1]) + env[2] * abs(v[2])
            pdust = sum(env[j] * abs(v[j]) for j in range(3) if _dusty(v[j])) + T(0) * pe
            comp = [pr * v[j] for j in range(3)]
            cenv = [pe * abs(v[j]) for j in range(3)]
            cdust = [(pe if _dusty(v[j]) else pdust) * abs(v[j]) for j in range(3)]
            return comp, cenv, cdust

        def rms(comp):
            return np.sqrt(T(0.5) * sum(np.sum(c.real * c.real + c.imag * c.imag) if np.iscomplexobj(c) else np.sum(c * c)
                                         for c in comp))

        cq, eq, dq_ = project(q)
        c1, e1, d1 = project(p1)
        c2, e2, d2 = project(p2)
        vq, vq_e, vq_d = rms(cq), rms(eq), rms(dq_)
        if strips[s, F_CIRC] != 0:                               # :2085-2087: the whole transverse velocity
            perp = [vrel[j] - cq[j] for j in range(3)]
            perp_e = [env[j] + eq[j] for j in range(3)]
            v1 = v2 = rms(perp)
            v1_e = v2_e = rms(perp_e)
            v1_d = v2_d = rms(dq_)
        else:
            v1, v1_e, v1_d = rms(c1), rms(e1), rms(d1)
            v2, v2_e, v2_d = rms(c2), rms(e2), rms(d2)
        bterms = [(rec[F_DQ] * vq, rec[F_DQ] * vq_e, rec[F_DQ] * vq_d, q), (rec[F_DP1] * v1, rec[F_DP1] * v1_e, rec[F_DP1] * v1_d, p1),
                  (rec[F_DP2] * v2, rec[F_DP2] * v2_e, rec[F_DP2] * v2_d, p2), (rec[F_DEND] * vq, rec[F_DEND] * vq_e, rec[F_DEND] * vq_d, q)]
        for a in range(3):                                       # :2093-2113
            for b in range(3):
                for val, e_, d_, v in bterms:
                    dy = v[a] * v[b]
                    Bmat[s, a, b] += val * dy
                    Bmat_E[s, a, b] += abs(e_ * dy)
                    Bmat_D[s, a, b] += abs(e_ * dy) if (_dusty(v[a]) or _dusty(v[b])) else abs(d_ * dy)
        # helpers.py:537-560 translateMatrix3to6DOF with getH (:428-437)
        H = np.array([[0, r[2], -r[1]], [-r[2], 0, r[0]], [r[1], -r[0], 0]], dtype=T)
        aH = np.abs(H)
        for M, out6, absolute in ((Bmat[s], Bd, False), (Bmat_E[s], Bd_E, True), (Bmat_D[s], Bd_D, True)):
            Hm = aH if absolute else H
            MH = M @ Hm
            out6[:3, :3] += M
            out6[:3, 3:] += MH
            out6[3:, :3] += MH.T
            out6[3:, 3:] += Hm @ M @ Hm.T
        # F_exc_drag = Bmat u[ih] (:2122, 2146) and its translation (:2152)
        F3, E3, D3 = (np.zeros((nH, 3, nw), dtype=t) for t in (CT, T, T))
        for a in range(3):
            for b in range(3):
                F3[:, a] += Bmat[s, a, b] * u[:, s, b]
                E3[:, a] += Bmat_E[s, a, b] * au[:, s, b] * Wv[:, s, b]
                D3[:, a] += Bmat_D[s, a, b] * au[:, s, b]
        if keep_strips:
            Fx[:, s], Fx_E[:, s], Fx_D[:, s] = F3, E3, D3
        F6, E6, D6 = _translate(F3, E3, D3, r)
        Fd += F6
        Fd_E += E6
        Fd_D += D6
    out.Bmat, out.Bmat_E, out.Bmat_D = Bmat, Bmat_E, Bmat_D
    out.B_drag, out.B_drag_E, out.B_drag_D = Bd, Bd_E, Bd_D
    out.F_drag, out.F_drag_E, out.F_drag_D = Fd, Fd_E, Fd_D
    out.F_exc, out.F_exc_E, out.F_exc_D = Fx, Fx_E, Fx_D
    return out


def gate_multiples(x, ref, E, D=None):
    """(|x - ref| - 2 D)+ / (eps E) per entry: the gate holds where this is <= C.  Entries with E == 0 give 0 where x is
    exactly 0 and inf otherwise; where the reference is NaN the entry gives 0 if x is NaN too and inf otherwise.  No entry is
    left out."""
    x = np.asarray(x)
    ref = np.asarray(ref)
    CT = np.clongdouble if (np.iscomplexobj(x) or np.iscomplexobj(ref)) else np.longdouble
    x, ref = x.astype(CT), ref.astype(CT)
    E = np.asarray(E, dtype=np.longdouble)
    D = np.zeros(E.shape, dtype=np.longdouble) if D is None else np.asarray(D, dtype=np.longdouble)
    assert x.shape == ref.shape == E.shape == D.shape, (x.shape, ref.shape, E.shape, D.shape)
    out = np.full(ref.shape, np.inf)
    nan = np.isnan(ref)
    out[nan & np.isnan(x)] = 0.0
    zero = ~nan & (E == 0)
    out[zero & (x == 0)] = 0.0
    ok = ~nan & ~zero & np.isfinite(x)
    err = np.maximum(np.abs(x[ok] - ref[ok]) - 2 * D[ok], 0)
    out[ok] = (err / (EPS * E[ok])).astype(np.float64)
    return out


def relative_multiples(x, ref, W):
    """Single terms: |x - ref| / (eps W |ref|) per entry, W = 1 + kappa (+ n_s) broadcast to ref; exact zeros where the
    reference is 0, NaN where it is NaN."""
    ref = np.asarray(ref)
    return gate_multiples(x, ref, np.asarray(W, dtype=np.longdouble) * np.abs(ref).astype(np.longdouble))
