"""The Morison strip sweeps on the device -- k_excitation, k_linearize, the per-strip exports and the same device functions
inside the fused fixed point (k_solve_dynamics / raftx_kp_f*) -- held entry by entry to the extended-precision evaluation
of tests/strip_reference.py:  |x - ref| <= C eps E + 2 D, E the non-cancelling envelope weighted by 1 + kappa + n_s, D the
dust a kernel may drop; exact zeros where E == 0, NaN where the reference is NaN, no entry left out.
C and C_k are measured on the CPU (tests/test_strip_reference.py); nothing here is fitted to the device.

Shapes: every launch shape of pick_shape (nw 1, 64 | 65, 128 | 129, 200, 256 | 257 | 513, 1025, 1537, 2048; S <= 24 from
513 up), strip counts 0, 1, 63, 64, 65, 130, one and three headings, two sea states, tables free of runs and the run cases of
tests/strip_cases.py.  The reference is computed once per (table, sea state, linearisation point) and shared.

Bounds that are not the plain gate:
  * raftx_strip_kinematics (single terms): relative, C_k eps (1 + kappa) |ref|;
  * the seabed case (depth 20, k h from 0.03, strips within 0.5 m of the bed): the kernels form sinh k(z+h) / sinh kh as
    (e^{kz} - e^{-k(z+2h)}) / (1 - e^{-2kh}) and lose coth k(z+h) on the difference; the vertical velocity alone is held with
    that derived weight there (``shallow=True``), the sums with the plain envelope -- the limit is stated in DESIGN.md.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import strip_cases as sc
from tests import strip_reference as sr
from tests.util import random_matrices

pytestmark = pytest.mark.gpu
C, CK = sr.GATE_C, sr.GATE_CK
RHO, G = 1025.0, 9.81
KF_OUTF, KF_MULTI, KF_ALL = 4, 32, 127
NW_ALL = [1, 64, 65, 128, 129, 200, 256, 257, 513, 1025, 1537, 2048]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ batches and their shared references
@functools.lru_cache(maxsize=None)
def designs(kind, nw):
    """(names, tables, cm tables or None) of a batch: 'full' = every strip count and run case, 'mid' = what fits the shapes
    up to 257 bins in a second of reference time, 'small' = S <= 24."""
    runs = sc.run_designs()
    mcf_t, mcf_cm = sc.mcf_design(nw)
    if kind == "full":
        d = [("S%d" % S, sc.free_table(S), None) for S in (0, 1, 63, 64, 65, 130)]
        d += [(n, t, None) for n, t in runs.items()] + [("mcf", mcf_t, mcf_cm)]
    elif kind == "mid":
        d = [("S0", sc.free_table(0), None), ("S1", sc.free_table(1), None), ("S65", sc.free_table(65), None),
             ("vertical", runs["vertical"], None), ("steps", runs["steps"], None), ("mcf", mcf_t, mcf_cm)]
    elif kind == "runs":
        d = [(n, t, None) for n, t in runs.items()] + [("S65", sc.free_table(65), None)]
    else:
        d = [("S0", sc.free_table(0), None), ("S1", sc.free_table(1), None), ("S24", sc.free_table(24), None),
             ("steps", runs["steps"], None), ("mcf", mcf_t, mcf_cm)]
    return d


class Batch:
    def __init__(self, kind, nw, nCase, nHead, depth=200.0, tables=None, shallow=False, **sea):
        self.d = designs(kind, nw) if tables is None else tables
        self.w, self.k, self.zeta, self.beta = sc.sea_states(nw, nCase, nHead, depth=depth, **sea)
        self.depth, self.nw, self.nC, self.nH, self.shallow = depth, nw, nCase, nHead, shallow
        self.key = (kind if tables is None else tuple(n for n, _, _ in tables), nw, nCase, nHead, depth, tuple(sorted(sea.items())))
        self.Xi = np.array([[sc.linearisation_point(nw, seed=7 * i + c) for c in range(nCase)] for i in range(len(self.d))])

    def upload(self, ctx, matrices=False):
        off, strips = sc.pack([t for _, t, _ in self.d])
        n = len(self.d)
        if matrices:
            M0, B0, C0, _ = random_matrices(np.random.default_rng(5), n)
        else:
            M0 = B0 = C0 = np.zeros((n, 6, 6))
        cms = [c for _, _, c in self.d if c is not None]
        cmoff = cm = None
        if cms:
            cmoff = np.concatenate([[0], np.cumsum([0 if c is None else len(c) for _, _, c in self.d])]).astype(np.int64)
            cm = np.concatenate(cms, axis=0)
        ctx.upload_designs_raw(off, strips, M0, B0, C0, self.nw, None, cmoff, cm)
        ctx.upload_cases(self.w, self.k, self.depth, RHO, G, self.zeta, self.beta)
        return off

    def ref(self, i, c, Xi="own"):
        """The longdouble reference of design i under sea state c about Xi ('own': this batch's point, None: excitation
        only, or an array [6,nw]); cached per batch key."""
        if isinstance(Xi, str):
            return _ref(self, i, c, "own", None)
        if Xi is None:
            return _ref(self, i, c, "none", None)
        return sr.strip_sweep(self.d[i][1], self.d[i][2], self.w, self.k, self.depth, RHO, G, self.zeta[c], self.beta[c],
                              Xi=Xi, shallow=self.shallow, keep_strips=False)


_REFS = {}


def _ref(b, i, c, mode, _):
    key = (b.key, i, c, mode, b.shallow)
    if key not in _REFS:
        _REFS[key] = sr.strip_sweep(b.d[i][1], b.d[i][2], b.w, b.k, b.depth, RHO, G, b.zeta[c], b.beta[c],
                                    Xi=b.Xi[i, c] if mode == "own" else None, shallow=b.shallow)
    return _REFS[key]


def gate(x, ref, E, D, what, mult=C):
    m = sr.gate_multiples(x, ref, E, D)
    worst = float(m.max()) if m.size else 0.0
    assert worst <= mult, (what, worst, mult, np.argwhere(m > mult)[:4].tolist())
    return worst


def report(what, worst):
    print("%s: worst multiples of eps E  %s" % (what, "  ".join("%s %.2f" % kv for kv in sorted(worst.items()))))


def check_excitation_and_linearize(ctx, b, what):
    b.upload(ctx)
    F = ctx.excitation()
    B, Fd = ctx.linearize(b.Xi)
    worst = {"F_iner": 0.0, "B_drag": 0.0, "F_drag": 0.0}
    for i, (name, t, _) in enumerate(b.d):
        for c in range(b.nC):
            r = b.ref(i, c)
            tag = "%s %s case %d" % (what, name, c)
            worst["F_iner"] = max(worst["F_iner"], gate(F[i, c], r.F_iner, r.F_iner_E, r.F_iner_D, tag + " F_iner"))
            worst["B_drag"] = max(worst["B_drag"], gate(B[i, c], r.B_drag, r.B_drag_E, r.B_drag_D, tag + " B_drag"))
            worst["F_drag"] = max(worst["F_drag"], gate(Fd[i, c], r.F_drag, r.F_drag_E, r.F_drag_D, tag + " F_drag"))
            if len(t) == 0:
                assert np.all(F[i, c] == 0) and np.all(B[i, c] == 0) and np.all(Fd[i, c] == 0), tag
    report(what, worst)
    return worst


# ------------------------------------------------------------------ raftx_excitation, raftx_linearize
@pytest.mark.parametrize("nw", NW_ALL)
def test_excitation_and_linearize_at_every_launch_shape(hip_ctx, nw):
    """nw 200: every table, three headings, two sea states; 65: every table, one heading; the other shapes: the tables
    that fit a second of reference time (S <= 24 from 513 bins up); one or three headings alternately."""
    if nw == 200:
        b = Batch("full", nw, 2, 3)
    elif nw == 65:
        b = Batch("full", nw, 1, 1)
    else:
        b = Batch("mid" if nw <= 257 else "small", nw, 2 if nw <= 257 else 1, 3 if NW_ALL.index(nw) % 2 else 1)
    check_excitation_and_linearize(hip_ctx, b, "nw %d, nHead %d" % (nw, b.nH))


def test_depth_branches_and_very_deep_strips(hip_ctx):
    """A bin with k == 0; depth 2000 with k h on either side of 89.4 inside the grid; strips down to k z = -650, alone and
    mixed with shallow ones (eps E stays a normal number: nothing is compared below the underflow threshold)."""
    b = Batch("runs", 200, 1, 3, k_zero=True)
    assert b.k[0] == 0.0
    check_excitation_and_linearize(hip_ctx, b, "k[0] == 0")
    deep = [(n, t, None) for n, t in sc.deep_designs().items()] + [("run130", sc.run_designs()["run130"], None),
                                                                    ("S24", sc.free_table(24), None)]
    b = Batch(None, 200, 2, 2, depth=2000.0, tables=deep)
    kh = b.k * 2000.0
    assert (kh > 89.4).any() and (kh < 89.4).any() and abs(b.k.max() * 1593.0 - 650.0) < 5.0
    E = b.ref(0, 0).F_iner_E
    assert float(E[E > 0].min()) * sr.EPS > 1e-300
    check_excitation_and_linearize(hip_ctx, b, "depth 2000")


def test_strips_at_the_seabed_in_shallow_water(hip_ctx):
    """Depth 20, w from 0.02 (k h = 0.03), strips within 0.5 m of the seabed: the sums under the PLAIN envelope; the
    vertical velocity of raftx_strip_kinematics with the derived weight coth k(z+h)."""
    t = [("seabed", sc.seabed_design(20.0), None)]
    b = Batch(None, 200, 1, 2, depth=20.0, tables=t, wmin=0.02)
    assert b.k[0] * 20.0 < 0.035
    check_excitation_and_linearize(hip_ctx, b, "seabed, plain envelope")
    bs = Batch(None, 200, 1, 2, depth=20.0, tables=t, shallow=True, wmin=0.02)
    check_strip_exports(hip_ctx, bs, "seabed, coth weight on u_z")
    r = b.ref(0, 0)
    u, _, _ = hip_ctx.strip_kinematics(0, len(t[0][1]))
    m = sr.relative_multiples(u[:, :, 2], r.u[:, :, 2], r.W - sr.run_steps(t[0][1])[None, :, None])
    print("seabed: u_z WITHOUT the coth weight %.1f eps (1 + kappa)|u_z| (C_k = %d)" % (m.max(), CK))


def test_circular_strips_with_a_purely_axial_relative_velocity(hip_ctx):
    """Still water, a translation along the axis of an inclined circular member: the transverse velocity is exactly zero
    in the reference (vrel - vrel_q component by component, raft_member.py:2079).  The kernels take |v_perp|^2 as
    |v|^2 - |v_q|^2 summed over the bins and clamp it at zero: with at most 16 eps sum |v|^2 of rounding in the difference
    (eight squares and the three-term projection, each bin) the spurious vRMS_p is at most sqrt(16 eps) vRMS_v, so
    Bmat may carry up to sqrt(16 eps) vRMS_v (b_p1 |p1 p1^T| + b_p2 |p2 p2^T|) on top of the gate -- a stated limit
    (DESIGN.md section 4), 6e-8 of the axial term.  Everything else of the entry keeps the plain gate."""
    nw = 200
    rng = np.random.default_rng(9)
    q = np.array([0.6, 0.0, 0.8])
    t = sc.member(rng, [3.0, -4.0, -30.0], q, [1] * 7, 1.5, circ=True)
    w, k, zeta, beta = sc.sea_states(nw, 1, 1)
    zeta[:] = 0.0
    amp = rng.uniform(0.2, 1.0, nw) * np.exp(1j * rng.uniform(0, 2 * np.pi, nw))
    Xi = np.zeros((6, nw), dtype=np.complex128)
    Xi[:3] = q[:, None] * amp
    S = len(t)
    z = np.zeros((1, 6, 6))
    hip_ctx.upload_designs_raw(np.array([0, S], dtype=np.int64), t, z, z, z, nw)
    hip_ctx.upload_cases(w, k, 200.0, RHO, G, zeta, beta)
    r = sr.strip_sweep(t, None, w, k, 200.0, RHO, G, zeta[0], beta[0], Xi=Xi)
    B, F = hip_ctx.linearize(Xi[None, None])
    assert np.all(F == 0)                                         # no waves: E == 0
    vrms = float(np.sqrt(0.5 * np.sum(np.abs(w * amp) ** 2)))   # |q| = 1: the whole velocity is axial
    slack6 = np.zeros((6, 6))
    worst = 0.0
    Bm, _ = hip_ctx.strip_drag(0, S, Xi)
    for s in range(S):
        p1, p2, a = t[s, sr.F_P1:sr.F_P1 + 3], t[s, sr.F_P2:sr.F_P2 + 3], t[s, sr.F_AX:sr.F_AX + 3]
        X = np.sqrt(16 * sr.EPS) * vrms * (t[s, sr.F_DP1] * np.abs(np.outer(p1, p1)) + t[s, sr.F_DP2] * np.abs(np.outer(p2, p2)))
        H = np.abs(np.array([[0, a[2], -a[1]], [-a[2], 0, a[0]], [a[1], -a[0], 0]]))
        slack6 += np.block([[X, X @ H], [(X @ H).T, H @ X @ H.T]])
        err = np.abs(Bm[s] - np.asarray(r.Bmat[s], dtype=np.float64))
        assert np.all(err <= C * sr.EPS * np.asarray(r.Bmat_E[s], dtype=np.float64) + X), (s, err, X)
        worst = max(worst, float((err / np.where(X > 0, X, np.inf)).max()))
    err6 = np.abs(B[0, 0] - np.asarray(r.B_drag, dtype=np.float64))
    print("axial relative velocity: spurious transverse drag %.3f of the sqrt(16 eps) bound per strip, %.3f in B_drag; "
          "plain gate alone: %.3g eps E" % (worst, float((err6 / np.where(slack6 > 0, slack6, np.inf)).max()), float(sr.gate_multiples(B[0, 0], r.B_drag, r.B_drag_E, r.B_drag_D).max())))
    assert np.all(err6 <= C * sr.EPS * np.asarray(r.B_drag_E, dtype=np.float64) + slack6)


# ------------------------------------------------------------------ raftx_strip_kinematics, raftx_strip_drag
def check_strip_exports(ctx, b, what):
    b.upload(ctx)
    worst = {}
    for i, (name, t, _) in enumerate(b.d):
        S = len(t)
        if S == 0:
            continue
        for c in range(b.nC):
            r = b.ref(i, c)
            u, ud, p = ctx.strip_kinematics(i, S, icase=c)
            W1 = r.W - sr.run_steps(t).astype(np.longdouble)[None, :, None]           # every strip evaluated directly: 1 + kappa
            Wv = np.stack([W1, W1, W1 * (r.Wz / r.W)], axis=2)
            for nm, x, ref, W in (("u", u, r.u, Wv), ("ud", ud, r.ud, Wv), ("pDyn", p, r.pDyn, W1)):
                m = sr.relative_multiples(x, ref, W)
                worst[nm] = max(worst.get(nm, 0.0), float(m.max()))
                assert m.max() <= CK, (what, name, c, nm, float(m.max()), np.argwhere(m > CK)[:4].tolist())
            for ih in range(b.nH):
                Bm, Fx = ctx.strip_drag(i, S, b.Xi[i, c], ih=ih, icase=c)
                worst["Bmat"] = max(worst.get("Bmat", 0.0), gate(Bm, r.Bmat, r.Bmat_E, r.Bmat_D, "%s %s Bmat" % (what, name)))
                worst["F_exc"] = max(worst.get("F_exc", 0.0),
                                     gate(Fx, r.F_exc[ih], r.F_exc_E[ih], r.F_exc_D[ih], "%s %s F_exc heading %d" % (what, name, ih)))
    report(what, worst)


@pytest.mark.parametrize("nw,kind", [(200, "full"), (257, "mid"), (1025, "small")])
def test_per_strip_exports(hip_ctx, nw, kind):
    """u, ud, pDyn: single terms, relative to their own magnitude with C_k; Bmat and Bmat u: sums of three dyads that can
    cancel, held to their envelopes with C (tests/test_strip_reference.py)."""
    check_strip_exports(hip_ctx, Batch(kind, nw, 2 if nw == 200 else 1, 3 if nw == 200 else 1), "exports nw %d" % nw)


# ------------------------------------------------------------------ the fused kernel, one pass about the constant XiStart
XI_START = 0.1


def fused_one_pass(ctx, b, extra, what):
    """nIter = 0: one linearisation about XiLast == XiStart in every DOF and bin; F_wave = F_extra + F_iner + F_drag(ih) and
    B_drag against the reference about that constant.  Returns (worst multiples, kernel flags)."""
    b.upload(ctx, matrices=True)
    n = len(b.d)
    Fx = None
    if extra:
        rng = np.random.default_rng(17)
        Fx = (rng.normal(size=(n, b.nC, b.nH, 6, b.nw)) + 1j * rng.normal(size=(n, b.nC, b.nH, 6, b.nw))) * 1e5
    out = ctx.solve_dynamics(0, tol=0.01, XiStart=XI_START, F_extra=Fx, want_Xi=True, want_B=True, want_F=True)
    flags = ctx.last_solve_kernel()
    Xi0 = np.full((6, b.nw), XI_START, dtype=np.complex128)
    worst = {"F_wave": 0.0, "B_drag": 0.0}
    for i, (name, t, _) in enumerate(b.d):
        for c in range(b.nC):
            key = (b.key, i, c, "start", b.shallow)
            if key not in _REFS:
                _REFS[key] = b.ref(i, c, Xi=Xi0)
            r = _REFS[key]
            ref, E = r.F_iner + r.F_drag, r.F_iner_E + r.F_drag_E
            if extra:
                ref, E = ref + Fx[i, c], E + np.abs(Fx[i, c])
            tag = "%s %s case %d" % (what, name, c)
            worst["F_wave"] = max(worst["F_wave"], gate(out["F_wave"][i, c], ref, E, r.F_iner_D + r.F_drag_D, tag + " F_wave"))
            worst["B_drag"] = max(worst["B_drag"], gate(out["B_drag"][i, c], r.B_drag, r.B_drag_E, r.B_drag_D, tag + " B_drag"))
    report("%s (kernel flags %d, %d waves per SIMD, %d cache slots)" % ((what,) + flags), worst)
    return worst, flags


@pytest.mark.parametrize("nHead,extra,expect", [(1, False, KF_OUTF), (3, False, KF_OUTF | KF_MULTI), (1, True, KF_ALL),
                                                (3, True, KF_ALL)])
def test_fused_one_pass_at_the_200_bin_shape(hip_ctx, nHead, extra, expect):
    """The lean KF_OUTF and KF_OUTF | KF_MULTI kernels (persistent form) and, with an extra excitation, the full-featured
    one; the tables without MacCamy-Fuchs rows (those ask for another specialisation: test_fused_one_pass_elsewhere)."""
    b = Batch("runs", 200, 2, nHead)
    _, flags = fused_one_pass(hip_ctx, b, extra, "fused one pass, nw 200, nHead %d%s" % (nHead, ", F_extra" if extra else ""))
    assert flags[0] == expect and flags[1] == (1 if expect == KF_ALL else 2)


@pytest.mark.parametrize("nw", [n for n in NW_ALL if n != 200])
def test_fused_one_pass_elsewhere(hip_ctx, nw):
    """Every other launch shape runs the full-featured kernel when F_wave is exported; MacCamy-Fuchs rows included."""
    b = Batch("mid" if nw <= 257 else "small", nw, 1, 3 if NW_ALL.index(nw) % 2 else 1)
    _, flags = fused_one_pass(hip_ctx, b, nw in (129, 1025), "fused one pass, nw %d" % nw)
    assert flags[0] == KF_ALL


def test_fused_one_pass_per_pair_launches_in_a_child_process():
    """RAFTX_PERSIST=0 is read once per process: the lean kernels as one workgroup per pair, in a fresh process."""
    env = dict(os.environ, RAFTX_PERSIST="0")
    p = subprocess.run([sys.executable, "-m", "tests.test_hip_strip_reference"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    print(p.stdout)
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res["flags"] == [KF_OUTF, KF_OUTF | KF_MULTI] and all(v <= C for v in res["worst"])


def _child():
    from raft_amd import backend
    ctx = backend.hip_library().context(0)
    flags, worst = [], []
    try:
        for nH in (1, 3):
            wr, fl = fused_one_pass(ctx, Batch("runs", 200, 2, nH), False, "per-pair launches, nHead %d" % nH)
            flags.append(fl[0])
            worst += list(wr.values())
    finally:
        ctx.close()
    print(json.dumps({"flags": flags, "worst": worst}))


# ------------------------------------------------------------------ the fused fixed point: its last linearisation point
@pytest.mark.parametrize("nw,nHead", [(200, 3), (65, 1), (513, 1)])
def test_fused_fixed_point_about_its_last_linearisation_point(hip_ctx, nw, nHead):
    """nIter = 8 with the linearisation point exported: B_drag and F_wave against the reference about exactly the XiLast the
    kernel linearised about last (it owes nothing to the solves: their result enters as the reference's input)."""
    b = Batch("runs" if nw == 200 else ("mid" if nw <= 257 else "small"), nw, 1, nHead)
    b.upload(hip_ctx, matrices=True)
    hip_ctx.set_linearisation_point(None, keep_last=True)
    out = hip_ctx.solve_dynamics(8, tol=0.01, XiStart=XI_START, want_Xi=True, want_B=True, want_F=True)
    assert hip_ctx.last_solve_kernel()[0] == KF_ALL
    XiLast = hip_ctx.fetch_linearisation_point()
    hip_ctx.set_linearisation_point(None, keep_last=False)
    assert np.all(np.isfinite(XiLast)) and np.all(out["niter"] >= 1)
    worst = {"F_wave": 0.0, "B_drag": 0.0}
    for i, (name, t, _) in enumerate(b.d):
        r = b.ref(i, 0, Xi=XiLast[i, 0])
        if len(t):
            assert not np.array_equal(XiLast[i, 0], np.full((6, nw), XI_START)), name      # it did iterate
        worst["F_wave"] = max(worst["F_wave"], gate(out["F_wave"][i, 0], r.F_iner + r.F_drag, r.F_iner_E + r.F_drag_E,
                                                    r.F_iner_D + r.F_drag_D, "%s F_wave" % name))
        worst["B_drag"] = max(worst["B_drag"], gate(out["B_drag"][i, 0], r.B_drag, r.B_drag_E, r.B_drag_D, "%s B_drag" % name))
    report("fixed point nIter 8, nw %d (iterations %s)" % (nw, out["niter"][:, 0].tolist()), worst)


if __name__ == "__main__":
    _child()
