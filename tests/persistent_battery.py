"""Inputs, runner and comparison shared by tests/test_persistent_reference.py (CPU, oracle only) and
tests/test_hip_persistent.py (GPU): the battery that makes a workgroup of the persistent fused kernel (raftx_kp_f<FLAGS>,
raftx_kpg_f0) solve pair after pair.  Everything is at nw = 200, the only shape with persistent twins.

(a) twin_batch(flags): nine designs x three sea states = 27 pairs for each of the twelve flag sets of RAFTX_PERSIST128:
    per = 4, slab 6 of the claim holds three positions and slab 7 none.  Neighbouring pairs differ in strip count (0 and 1
    included), sea state (amplitudes more than an order of magnitude apart), iteration count and heading count; design
    NAN_D is singular (all-zero M0, B0, C0, no strips) and sits between two ordinary designs.
(b) edge_batch(nl): the plain kernel with nl = 1, 2, 7, 8, 9, 17 pairs at one sea state per design.
(c) reuse_batch(): nine pairs and two sets of sea states, launched 2 x 64 + 3 times in one context.
(d) the generating form: child_gen().

The runner is the same code for the oracle (the parent process, once) and for the device (a child process per setting of
RAFTX_KP_GRID / RAFTX_PERSIST, which are read once per process)."""
import functools
import os
import re

import numpy as np

from raft_amd._abi import FLAG_NAN, WANT_BDRAG, WANT_FWAVE
from tests.util import group_rel_err, rel_err, random_strips, random_matrices, synthetic_cases, add_mcf_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9                               # the gate of tests/test_hip_parity.py (asserted equal in test_persistent_reference.py)
NW = 200
SOLVER_TOL, XI_START = 0.01, 0.1
KF_FDEP, KF_OUTF, KF_EXTRA, KF_MCF, KF_MULTI = 1, 4, 8, 16, 32

# flags of the twin -> (frequency-dependent M/B, MacCamy-Fuchs fraction, headings, extra excitation, F_wave exported):
# the ten rows of test_featured_sweep_kernels_run_lean_and_match_the_oracle that select a lean kernel, and the two
# F_wave-exporting ones of test_fused_one_pass_at_the_200_bin_shape
TWINS = {
    0: (False, 0.0, 1, False, False),
    KF_FDEP: (True, 0.0, 1, False, False),
    KF_MCF: (False, 0.3, 1, False, False),
    KF_MULTI: (False, 0.0, 3, False, False),
    KF_FDEP | KF_EXTRA: (True, 0.0, 1, True, False),
    KF_FDEP | KF_MCF: (True, 0.3, 1, False, False),
    KF_FDEP | KF_MULTI: (True, 0.0, 2, False, False),
    KF_MCF | KF_MULTI: (False, 0.3, 2, False, False),
    KF_FDEP | KF_EXTRA | KF_MULTI: (True, 0.0, 2, True, False),
    KF_FDEP | KF_MCF | KF_MULTI: (True, 0.3, 2, False, False),
    KF_OUTF: (False, 0.0, 1, False, True),
    KF_OUTF | KF_MULTI: (False, 0.0, 3, False, True),
}
S_LIST = [53, 0, 47, 60, 1, 53, 38, 0, 12]      # strips asked for (member runs of ten: 50, 0, 40, 60, 1, 50, 30, 0, 10 rows)
NAN_D = 1                                        # the singular design; design 7 is the ordinary one without strips
SEA_AMP = np.array([0.01, 0.3, 5.0])             # largest wave amplitude (m) of the three sea states: the drawn spectra rescaled
N_ITER_A = 7                                     # cap of (a): from XiStart = 0.1 the pairs take 6 to 10 iterations, the slowest do not converge
N_ITER_A_OF = {KF_MULTI: 6, KF_OUTF | KF_MULTI: 6}    # (the batches whose slowest pair takes 8)
EDGE_NL = (1, 2, 7, 8, 9, 17)
EDGE_S = [53, 12, 0, 47, 1, 60, 38, 22, 9, 53, 60, 0, 31, 44, 5, 18, 57]
N_ITER_B = 8
REUSE_LAUNCHES = 2 * 64 + 3                      # KP_RING = 64 counter sets: every set a third time


def persist128_flags():
    """the flag sets of RAFTX_PERSIST128 as the kernel header lists them"""
    src = open(os.path.join(ROOT, "raft_amd", "csrc", "raftx_kernels.h")).read()
    line = re.search(r"#define RAFTX_PERSIST128\(X\)(.*)", src).group(1)
    return [int(v) for v in re.findall(r"X\((\d+)\)", line)]


def grid_for_pairs(n):
    return ((n + 7) // 8) * 8


def _tables(rng, S_list):
    from tests.test_hip_parity import _member_run_table
    return [_member_run_table(rng, S // 10, 10) if S >= 10 else random_strips(rng, S) for S in S_list]


class Batch:
    def __init__(self, name, flags, tables, mats, cases, Fe, want_F, nIter):
        self.name, self.flags, self.tables, self.want_F, self.nIter, self.Fe = name, flags, tables, want_F, nIter, Fe
        self.M0, self.B0, self.C0, self.MBw = mats
        self.w, self.k, self.zeta, self.beta = cases
        self.nD, self.nC, self.nH = len(tables), self.zeta.shape[0], self.zeta.shape[1]
        self.pairs = self.nD * self.nC
        self.keys = ("Xi", "niter", "flags", "B_drag") + (("F_wave",) if want_F else ())


@functools.lru_cache(maxsize=None)
def twin_batch(flags):
    fdep, mcf, nH, extra, want_F = TWINS[flags]
    rng = np.random.default_rng(9100 + flags)
    tables = _tables(rng, S_LIST)
    if mcf:
        tables = add_mcf_rows(rng, tables, mcf, NW)
    M0, B0, C0, MBw = random_matrices(rng, len(S_LIST), NW, fdep)
    M0[NAN_D] = B0[NAN_D] = C0[NAN_D] = 0.0
    if MBw is not None:
        MBw[NAN_D] = 0.0
    w, k, zeta, beta = synthetic_cases(rng, len(SEA_AMP), nH, NW)
    zeta = zeta * (SEA_AMP / zeta.max(axis=(1, 2)))[:, None, None]
    Fe = None
    if extra:
        shape = (len(S_LIST), len(SEA_AMP), nH, 6, NW)
        Fe = 2e4 * (rng.normal(size=shape) + 1j * rng.normal(size=shape)) * SEA_AMP[None, :, None, None, None]
    return Batch("a%d" % flags, flags, tables, (M0, B0, C0, MBw), (w, k, zeta, beta), Fe, want_F, N_ITER_A_OF.get(flags, N_ITER_A))


@functools.lru_cache(maxsize=None)
def edge_batch(nl):
    rng = np.random.default_rng(7300)                    # one pool of designs: nl takes its first nl
    tables = _tables(rng, EDGE_S)[:nl]
    M0, B0, C0, _ = random_matrices(rng, len(EDGE_S), NW, False)
    w, k, zeta, beta = synthetic_cases(np.random.default_rng(7300 + nl), 1, 1, NW)
    return Batch("b%d" % nl, 0, tables, (M0[:nl], B0[:nl], C0[:nl], None), (w, k, zeta, beta), None, False, N_ITER_B)


@functools.lru_cache(maxsize=None)
def reuse_batch():
    """(batch of the first sea-state set, (zeta, beta) of the second)"""
    rng = np.random.default_rng(7400)
    tables = _tables(rng, [53, 0, 47])
    M0, B0, C0, _ = random_matrices(rng, 3, NW, False)
    w, k, zeta, beta = synthetic_cases(rng, 3, 1, NW)
    _, _, zeta2, beta2 = synthetic_cases(rng, 3, 1, NW)
    return Batch("c", 0, tables, (M0, B0, C0, None), (w, k, zeta, beta), None, False, N_ITER_B), (0.5 * zeta2, beta2)


def all_batches():
    return [twin_batch(f) for f in TWINS] + [edge_batch(n) for n in EDGE_NL]


# ------------------------------------------------------------------ the runner (oracle and device alike)
def upload_designs(ctx, b):
    ctx.upload_designs(b.tables, b.M0, b.B0, b.C0, NW, b.MBw)


def solve(ctx, b, amp=1.0, tol=SOLVER_TOL, zeta=None, beta=None, XiLast0=None):
    """One launch on the resident designs with the batch's sea states (amplitudes x amp); the results the batch exports."""
    ctx.upload_cases(b.w, b.k, 200.0, 1025.0, 9.81, amp * (b.zeta if zeta is None else zeta), b.beta if beta is None else beta)
    if XiLast0 is not None:
        ctx.set_linearisation_point(XiLast0, keep_last=False)
    ctx.solve_dynamics_device(b.nIter, tol, XI_START, F_extra=b.Fe, want_mask=WANT_BDRAG | (WANT_FWAVE if b.want_F else 0))
    out = ctx.fetch_results(want_Xi=True, want_B=True, want_F=b.want_F)
    return {key: out[key] for key in b.keys}


def run(ctx, b, prewash, **kw):
    """upload + solve; prewash: the same batch with all wave amplitudes tripled first -- the results stay resident in the
    context, and a pair that the checked launch never claims then shows those numbers, not the right ones from last time"""
    upload_designs(ctx, b)
    if prewash:
        solve(ctx, b, amp=3.0)
    return solve(ctx, b, **kw)


@functools.lru_cache(maxsize=None)
def oracle_reference(name, amp=1.0, tol_scale=1.0):
    """the oracle's results of batch `name` ("a<flags>" / "b<nl>"), computed once per process"""
    from raft_amd._abi import RaftxLib
    from tests.conftest import _build_oracle
    b = twin_batch(int(name[1:])) if name[0] == "a" else edge_batch(int(name[1:]))
    ctx = RaftxLib(_build_oracle()).context(0)
    try:
        return run(ctx, b, False, amp=amp, tol=SOLVER_TOL * tol_scale)
    finally:
        ctx.close()


# ------------------------------------------------------------------ the comparisons
def compare_with_oracle(got, ref, what=""):
    """niter and flags equal; group_rel_err(Xi) < TOL per design; B_drag and F_wave to rel_err < TOL per pair, where
    exported.  A pair the reference flags NaN is held to niter and flags (its numbers are NaN / inf on both sides).
    Returns (covered [nD,nC] bool: the pairs that took part, worst error seen)."""
    assert np.array_equal(got["niter"], ref["niter"]), (what, "niter", got["niter"].tolist(), ref["niter"].tolist())
    assert np.array_equal(got["flags"], ref["flags"]), (what, "flags", got["flags"].tolist(), ref["flags"].tolist())
    nD, nC = ref["niter"].shape
    nan = (ref["flags"] & FLAG_NAN) != 0
    covered = nan.copy()
    worst = 0.0
    for d in range(nD):
        ok = ~nan[d]
        if ok.any():
            e = group_rel_err(got["Xi"][d][ok], ref["Xi"][d][ok])
            worst = max(worst, e)
            assert e < TOL, (what, "Xi of design %d" % d, e)
        for c in np.flatnonzero(ok):
            for key in ("B_drag", "F_wave"):
                if ref.get(key) is not None:
                    e = rel_err(got[key][d, c], ref[key][d, c])
                    worst = max(worst, e)
                    assert e < TOL, (what, "%s of pair (%d, %d)" % (key, d, c), e)
            covered[d, c] = True
    return covered, worst


def differing_keys(a, b, keys):
    """the keys whose arrays differ in any bit"""
    return [key for key in keys if a[key].shape != b[key].shape or not np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8))]


def largest_group_rel_err(a, b):
    """max over designs of group_rel_err(Xi) between two runs (pairs NaN in either left out)"""
    nan = ((a["flags"] | b["flags"]) & FLAG_NAN) != 0
    worst = 0.0
    for d in range(a["Xi"].shape[0]):
        ok = ~nan[d]
        if ok.any():
            worst = max(worst, group_rel_err(a["Xi"][d][ok], b["Xi"][d][ok]))
    return worst


# ------------------------------------------------------------------ the child process of one setting
def expected_launch(pairs):
    """(persistent, grid) this process must report for a whole launch of `pairs` pairs, from its own environment"""
    if os.environ.get("RAFTX_PERSIST") == "0":
        return 0, grid_for_pairs(pairs)
    g = int(os.environ.get("RAFTX_KP_GRID", "0"))
    # (the default grid is what the chip holds at once, four workgroups per CU: more than any batch here has pairs)
    return 1, (min(g, grid_for_pairs(pairs)) if g > 0 else grid_for_pairs(pairs))


def _check_launch(ctx, b, diag):
    flags, waves, _ = ctx.last_solve_kernel()
    persistent, grid, pairs = ctx.last_solve_launch()
    assert (flags, waves) == (b.flags, 2), (b.name, "kernel", flags, waves)
    assert (persistent, grid) == expected_launch(b.pairs) and pairs == b.pairs, (b.name, "launch", persistent, grid, pairs)
    diag.append([b.flags, persistent, grid, pairs])


def child_main(path):
    """(a), (b), (c) on the device in this process's setting -> path (.npz)"""
    from raft_amd import backend
    ctx = backend.hip_library().context(0)
    out, diag = {}, []
    try:
        for b in all_batches():
            res = run(ctx, b, True)
            _check_launch(ctx, b, diag)
            for key in b.keys:
                out["%s_%s" % (b.name, key)] = res[key]
        b, (zeta2, beta2) = reuse_batch()
        upload_designs(ctx, b)
        first, differ = {}, []
        for i in range(REUSE_LAUNCHES):
            s = i % 2
            res = solve(ctx, b, zeta=zeta2 if s else None, beta=beta2 if s else None)
            if s not in first:
                first[s] = res
                _check_launch(ctx, b, diag)
                for key in b.keys:
                    out["c%d_%s" % (s, key)] = res[key]
            elif differing_keys(res, first[s], b.keys):
                differ.append(i)
        out["c_differ"] = np.array(differ, dtype=np.int64)
        out["diag"] = np.array(diag, dtype=np.int64)
    finally:
        ctx.close()
    np.savez(path, **out)


def child_gen(path):
    """(d): crossings of 7, 1 and 64 C3 variants streamed through three slots, tables generated as RAFTX_FUSED_GEN says"""
    from raft_amd import backend
    from tests import test_geometry as tg
    C3 = tg.C3
    fused = os.environ.get("RAFTX_FUSED_GEN") == "1"
    sizes = (7, 1, 64)
    batches = [tg._c3_crossing_inputs(n) for n in sizes]
    fixed = (C3["w"], C3["k"], float(C3["depth"]), np.asarray(C3["zeta"])[None], np.asarray(C3["beta"])[None], int(C3["nIter"]), 0.01,
             float(C3["XiStart"]))
    ctx = backend.hip_library().context(0)
    out = {}
    try:
        sub = lambda i: ctx.sweep_prepare(i % 3, *batches[i], *fixed, want_Xi=True)
        hs = {0: sub(0), 1: sub(1)}
        ctx.sweep_launch(hs[0])
        for i in range(len(batches)):
            if i + 2 < len(batches):
                hs[i + 2] = sub(i + 2)
            if i + 1 < len(batches):
                ctx.sweep_launch(hs[i + 1])
            g = ctx.sweep_wait(hs.pop(i))
            nf, nb = g["generation_fused_blocks"]
            assert nb >= 1 and nf == (nb if fused else 0), (sizes[i], "generation", nf, nb)
            assert int(g["niter"].min()) >= 1 and not np.isnan(g["std"]).any()
            for key in ("Xi", "std", "niter", "flags", "strip_off"):
                out["d%d_%s" % (sizes[i], key)] = np.asarray(g[key])
        persistent, grid, pairs = ctx.last_solve_launch()              # the last block launched: the 64 designs
        assert (persistent, grid) == expected_launch(pairs) and persistent == 1 and pairs == sizes[-1], (persistent, grid, pairs)
        # (no flags here: raftx_last_solve_kernel speaks of the solving context, and a crossing's blocks hand back only the
        # launch form; that the generating specialisation ran is what generation_fused_blocks says)
        out["diag"] = np.array([[persistent, grid, pairs]], dtype=np.int64)
    finally:
        ctx.close()
    np.savez(path, **out)
