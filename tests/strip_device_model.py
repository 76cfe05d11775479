"""TEST INFRASTRUCTURE -- fp64 numpy model of the SCHEME the strip sweeps of raft_amd/csrc/raftx_kernels.h evaluate the wave
kinematics with (the header of that file), written from that description and importing nothing from
the kernels:

    a = e^{-i k (x cos beta + y sin beta)},  P = e^{kz},  Q = e^{-k (z + 2h)}   at a RUN START, evaluated exactly (libm here);
    along a run of equally spaced collinear strips the three are advanced by the rotors of ONE unit step
    e^{-i k du}, e^{k dz}, e^{-k dz}, applied once or twice per strip;
    u = (cb t1, sb t1, t2),  t1 = c1 a (P + Q),  t2 = i c1 a (P - Q),  c1 = w zeta0 / (1 - e^{-2kh})   [an expm1];
    pDyn = rho g zeta0 a (P + Q) / (1 + e^{-2kh});
    deep water (k h > 89.4): both depth constants 1, Q = 0 in the velocities and kept in the pressure (helpers.py:215-218);
    k == 0: P = 50000, Q = 49999, constants 1 (Sh = 1, Ch = Cc = 99999, helpers.py:211-214).

Its only purpose is to measure, on the CPU, what the scheme itself costs against tests/strip_reference.py -- rotor drift along
runs of up to 64 strips, the exponential form of the depth factors -- and to carry the seeded errors the gate must reject
(``faults``).  ``run_steps`` restates the run rules of the library's upload (straight, equally spaced, one triad and section
kind per run, at most 64 strips, steps of 1 or 2 units) from the ABI records alone.
"""
import numpy as np

from tests.strip_reference import (F_AI, F_AX, F_CIRC, F_IP1, F_IP2, F_IQ, F_MCF, F_P1, F_P2, F_Q, F_RHOV, F_X, NFIELD)

MAX_RUN = 64


def run_steps(strips):
    """(m [S], unit [S,3]): m = 0 at a run start, else the unit steps (1, 2) from the previous strip; unit = unit * q."""
    strips = np.asarray(strips, dtype=np.float64).reshape(-1, NFIELD)
    S = len(strips)
    m = np.zeros(S, dtype=int)
    unit_vec = np.zeros((S, 3))
    s = 0
    while s < S:
        e, proj = s + 1, []
        while e < S and e - s < MAX_RUN:
            pr, cr = strips[e - 1], strips[e]
            dv = cr[F_X:F_X + 3] - pr[F_X:F_X + 3]
            pj = float(np.dot(dv, cr[F_Q:F_Q + 3]))
            if not np.array_equal(pr[F_Q:F_Q + 3], cr[F_Q:F_Q + 3]) or not pj > 0.0 or not np.isfinite(pj):
                break
            perp = dv - pj * cr[F_Q:F_Q + 3]
            if np.sqrt(np.sum(perp * perp)) > 1e-10 * (1.0 + np.sum(np.abs(cr[F_X:F_X + 3]))):
                break
            proj.append(pj)
            e += 1
        unit = min(proj) if proj else 0.0
        for i in range(s, e):
            rec = strips[i]
            unit_vec[i] = unit * rec[F_Q:F_Q + 3]
            if i == s or unit <= 0.0:
                continue
            ratio = proj[i - s - 1] / unit
            mi = int(np.floor(ratio + 0.5))
            pr = strips[i - 1]
            ok = 1 <= mi <= 2 and abs(ratio - mi) < 1e-9
            ok = ok and np.all(np.abs(pr[F_X:F_X + 3] + mi * unit * rec[F_Q:F_Q + 3] - rec[F_X:F_X + 3])
                               <= 1e-10 * (1.0 + np.abs(rec[F_X:F_X + 3])))
            ok = ok and np.array_equal(pr[F_P1:F_P2 + 3], rec[F_P1:F_P2 + 3])
            ok = ok and (pr[F_CIRC] != 0) == (rec[F_CIRC] != 0) and (pr[F_MCF] >= 0) == (rec[F_MCF] >= 0)
            da, dx = rec[F_AX:F_AX + 3] - pr[F_AX:F_AX + 3], rec[F_X:F_X + 3] - pr[F_X:F_X + 3]
            ok = ok and np.all(np.abs(da - dx) <= 1e-9 * (1.0 + np.abs(rec[F_X:F_X + 3]) + np.abs(rec[F_AX:F_AX + 3])))
            m[i] = mi if ok else 0
        s = e
    return m, unit_vec


def kinematics(strips, w, k, depth, rho, g, zeta, beta, faults=None, rotors=True):
    """u, ud [nHead,S,3,nw], pDyn [nHead,S,nw] (complex128) by the rotor scheme; rotors=False: every strip evaluated as a
    run start (the exponential form alone, what the per-strip exports of the library do).  faults (seeded errors):
    rotor_rel: every phase rotor times (1 + rotor_rel);  no_second_exp: the deep-water pressure loses Q;
    reanchor_late: the FIRST run start after strip 0 is reached with the previous run's rotor (one step) and the exact
    evaluation happens one strip later."""
    faults = faults or {}
    strips = np.asarray(strips, dtype=np.float64).reshape(-1, NFIELD)
    w, k = np.asarray(w, dtype=np.float64), np.asarray(k, dtype=np.float64)
    nw, S = len(w), len(strips)
    zeta = np.asarray(zeta, dtype=np.float64).reshape(-1, nw)
    beta = np.asarray(beta, dtype=np.float64).reshape(-1)
    nH = len(beta)
    m, uv = run_steps(strips)
    if not rotors:
        m = np.zeros_like(m)
    late = -1
    if faults.get("reanchor_late"):
        starts = [s for s in range(1, S - 1) if m[s] == 0 and m[s + 1] != 0]
        late = starts[0]
    k0 = k == 0.0
    deep = ~k0 & (k * depth > 89.4)
    fin = ~k0 & ~deep
    csh, cch = np.ones(nw), np.ones(nw)
    csh[fin] = 1.0 / (-np.expm1(-2.0 * k[fin] * depth))
    cch[fin] = 1.0 / (1.0 + np.exp(-2.0 * k[fin] * depth))
    u = np.zeros((nH, S, 3, nw), dtype=np.complex128)
    pDyn = np.zeros((nH, S, nw), dtype=np.complex128)
    for ih in range(nH):
        cb, sb = np.cos(beta[ih]), np.sin(beta[ih])
        c1 = w * zeta[ih] * csh
        sp = rho * g * zeta[ih] * cch
        a = P = Q = rot = rp = rq = None
        for s in range(S):
            x, y, z = strips[s, F_X:F_X + 3]
            if (m[s] == 0 and s != late) or (late >= 0 and s == late + 1):
                with np.errstate(over="ignore"):
                    a = np.exp(-1j * (k * (cb * x + sb * y)))
                    P = np.where(k0, 50000.0, np.exp(k * z))
                    Q = np.where(k0, 49999.0, np.exp(-(k * (z + 2.0 * depth))))
                    du = cb * uv[s, 0] + sb * uv[s, 1]
                    rot = np.exp(-1j * (k * du)) * (1.0 + faults.get("rotor_rel", 0.0))
                    rp, rq = np.exp(k * uv[s, 2]), np.exp(-(k * uv[s, 2]))
            else:
                for _ in range(max(int(m[s]), 1)):
                    a, P, Q = a * rot, P * rp, Q * rq
            Qv = np.where(deep, 0.0, Q)
            Qp = np.where(deep, 0.0, Q) if faults.get("no_second_exp") else Q
            t1 = c1 * a * (P + Qv)
            u[ih, s, 0], u[ih, s, 1], u[ih, s, 2] = cb * t1, sb * t1, 1j * (c1 * a * (P - Qv))
            pDyn[ih, s] = sp * a * (P + Qp)
    return u, 1j * w * u, pDyn


def excitation(strips, cm, w, k, depth, rho, g, zeta, beta, faults=None):
    """F_iner [nHead,6,nw] (complex128) from the model's kinematics; plain fp64 sums strip after strip.  More faults:
    ip2 = (strip, rel): that strip's Ip2 term times (1 + rel);  arm_sign = strip: the product a_y F_z of that strip's roll
    moment with the wrong sign."""
    faults = faults or {}
    strips = np.asarray(strips, dtype=np.float64).reshape(-1, NFIELD)
    _, ud, pDyn = kinematics(strips, w, k, depth, rho, g, zeta, beta, faults)
    nH, S, _, nw = ud.shape
    F = np.zeros((nH, 6, nw), dtype=np.complex128)
    for s in range(S):
        rec = strips[s]
        q, p1, p2, r = rec[F_Q:F_Q + 3], rec[F_P1:F_P1 + 3], rec[F_P2:F_P2 + 3], rec[F_AX:F_AX + 3]
        mcf = int(rec[F_MCF])
        c1, c2 = (rec[F_RHOV] * cm[mcf][0], rec[F_RHOV] * cm[mcf][1]) if mcf >= 0 else (rec[F_IP1], rec[F_IP2])
        if faults.get("ip2", (-1, 0.0))[0] == s:
            c2 = c2 * (1.0 + faults["ip2"][1])
        aq = np.einsum("b,hbw->hw", q, ud[:, s]) * rec[F_IQ] + pDyn[:, s] * rec[F_AI]
        a1 = np.einsum("b,hbw->hw", p1, ud[:, s]) * c1
        a2 = np.einsum("b,hbw->hw", p2, ud[:, s]) * c2
        F3 = [aq * q[a] + a1 * p1[a] + a2 * p2[a] for a in range(3)]
        sg = -1.0 if faults.get("arm_sign", -1) == s else 1.0
        F[:, 0] += F3[0]
        F[:, 1] += F3[1]
        F[:, 2] += F3[2]
        F[:, 3] += sg * (r[1] * F3[2]) - r[2] * F3[1]
        F[:, 4] += r[2] * F3[0] - r[0] * F3[2]
        F[:, 5] += r[0] * F3[1] - r[1] * F3[0]
    return F
