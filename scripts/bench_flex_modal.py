#!/usr/bin/env python
"""Cost of the eigen analysis of units with flexible members (include/raftx_flex_modal.h) on the two committed decks, n = 150
(tests/golden/flex_volturnus.npz) and n = 240 (tests/golden/flex_mcf.npz), in stiffness / mass variants:

* raftx_flex_modal_batch on batches of 64, 256 and 1 024 systems with nModes = 12: the kernel's window on the device
  (raftx_last_kernel_ms) and the call (H2D, kernel, D2H);
* the batch of 1 024 as a call with nModes = 0, 12 and n;
* the batch of 1 024 with the grid forced to 256, 768 and 1 024 workgroups (RAFTX_FLEX_MODAL_GRID; the default is 2 per CU);
* for context, on the same box: numpy.linalg.eig(numpy.linalg.solve(M, C)) per system on one core and over a pool of 16
  processes.

Writes the table to --out (default profiles/flex_modal.txt) and prints one JSON line.  --kernels-only runs the device batches
alone, for a profiler run of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_flex_modal.py --kernels-only
"""
import argparse
import json
import multiprocessing
import os
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):     # one BLAS thread per process: the host figures are per core
    os.environ[_v] = "1"

import numpy as np                                                       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import flex_modal_cases as fmc                                # noqa: E402

DECKS = ((150, "flex_volturnus.npz"), (240, "flex_mcf.npz"))
BATCHES = (64, 256, 1024)


def variants(fixture, n_sys):
    """Stiffness and mass variants of a deck: C scaled by 0.7 .. 1.3, M by 0.95 .. 1.05 (seeded)."""
    M, C = fmc.deck_matrices(fixture)
    rng = np.random.default_rng(len(M))
    return (np.ascontiguousarray(M[None] * rng.uniform(0.95, 1.05, size=(n_sys, 1, 1))),
            np.ascontiguousarray(C[None] * np.linspace(0.7, 1.3, n_sys)[:, None, None]))


def timed(ctx, f, reps):
    f()
    ts, ks = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(1e3 * (time.perf_counter() - t0))
        ks.append(ctx.last_kernel_ms())
    return dict(call_ms=float(np.median(ts)), kernel_ms=float(np.median(ks)))


def _host_one(args):
    M, C = args
    return np.linalg.eig(np.linalg.solve(M, C))[0][0].real


def host_context(M, C):
    """ms per system on one core (64 systems), ms for the whole batch over 16 processes."""
    t0 = time.perf_counter()
    for i in range(64):
        _host_one((M[i], C[i]))
    one = 1e3 * (time.perf_counter() - t0) / 64
    with multiprocessing.get_context("fork").Pool(16) as pool:
        pool.map(_host_one, [(M[i], C[i]) for i in range(32)])            # (the workers are up)
        t0 = time.perf_counter()
        pool.map(_host_one, [(M[i], C[i]) for i in range(len(M))], chunksize=8)
        allp = 1e3 * (time.perf_counter() - t0)
    return one, allp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flex_modal.txt"))
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    host = {}
    if not a.kernels_only:                                               # before the GPU is opened: the pool forks
        for n, fixture in DECKS:
            M, C = variants(fixture, BATCHES[-1])
            host[n] = host_context(M, C)
    from raft_amd import backend
    ctx = backend.default_context(0)
    out = {"metric": "flex_modal"}
    lines = ["raftx_flex_modal_batch (k_flex_modal: one workgroup of 256 threads per system, H | X | Z in a global workspace per workgroup)",
             "kernel ms: the kernel's window on the device (raftx_last_kernel_ms); call ms: H2D + kernel + D2H; medians of %d" % a.reps, ""]
    for n, fixture in DECKS:
        M, C = variants(fixture, BATCHES[-1])
        for nb in BATCHES:
            r = timed(ctx, lambda: ctx.flex_modal_batch(M[:nb], C[:nb], n_modes=12), a.reps)
            out["n%d_batch%d" % (n, nb)] = r
            lines.append("n = %3d  batch %4d  nModes 12   kernel %9.2f ms  (%7.3f ms per system)   call %9.2f ms"
                         % (n, nb, r["kernel_ms"], r["kernel_ms"] / nb, r["call_ms"]))
        if a.kernels_only:
            continue
        for m in (0, 12, n):
            r = timed(ctx, lambda: ctx.flex_modal_batch(M, C, n_modes=m), a.reps)
            fl = ctx.flex_modal_batch(M, C, n_modes=0)["flags"]
            out["n%d_batch%d_modes%d" % (n, BATCHES[-1], m)] = r
            lines.append("n = %3d  batch %4d  nModes %3d  kernel %9.2f ms                           call %9.2f ms   (flagged systems: %d)"
                         % (n, BATCHES[-1], m, r["kernel_ms"], r["call_ms"], int(np.count_nonzero(fl & ~1))))
        for g in (256, 768, 1024):
            os.environ["RAFTX_FLEX_MODAL_GRID"] = str(g)
            r = timed(ctx, lambda: ctx.flex_modal_batch(M, C, n_modes=12), a.reps)
            del os.environ["RAFTX_FLEX_MODAL_GRID"]
            out["n%d_batch%d_grid%d" % (n, BATCHES[-1], g)] = r
            lines.append("n = %3d  batch %4d  nModes  12  kernel %9.2f ms  with RAFTX_FLEX_MODAL_GRID=%d" % (n, BATCHES[-1], r["kernel_ms"], g))
        one, allp = host[n]
        out["n%d_numpy" % n] = dict(one_core_ms_per_system=one, pool16_ms_per_batch=allp)
        lines.append("n = %3d  context, same box: numpy.linalg.eig(numpy.linalg.solve(M, C)) %.2f ms per system on one core; "
                     "the batch of %d over a pool of 16 processes %.1f ms" % (n, one, BATCHES[-1], allp))
        lines.append("")
    if not a.kernels_only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
