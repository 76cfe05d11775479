#!/usr/bin/env python
"""Cost of the eigen analysis of moored arrays (include/raftx_array_modal.h): raftx_array_modal_batch on 1 000 arrays of
nUnit = 2, 4, 6 as a call (H2D, kernel, D2H) and as kernel time, raftx_array_modal_moored on 1 000 copies of the pair, square4
and ring6 cases of tests/array_mooring_cases.py at their start poses, and for context the host loop of
numpy.linalg.eig(numpy.linalg.solve(M, C)) over the same batch on the same box (BENCH_ARRAY_MODAL_NO_HOST=1 leaves it out,
for a profiler run:

    BENCH_ARRAY_MODAL_NO_HOST=1 rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_array_modal.py

).  One JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raft_amd import backend                                             # noqa: E402
from tests import array_modal_cases as amc                               # noqa: E402
from tests import array_mooring_cases as ac                              # noqa: E402


def timed(f, reps=7):
    f()
    ts, ks = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(1e3 * (time.perf_counter() - t0))
        ks.append(timed.ctx.last_kernel_ms())
    return dict(call_ms=float(np.median(ts)), kernel_ms=float(np.median(ks)))


def main():
    n = int(os.environ.get("BENCH_ARRAY_MODAL_N", 1000))
    ctx = timed.ctx = backend.default_context(0)
    gold = amc.golden()["cases"]
    rng = np.random.default_rng(0)
    out = {"metric": "array_modal", "n_array": n}
    for nU in (2, 4, 6):
        rec = gold["synthetic%d" % nU]
        M = np.repeat(np.asarray(rec["M"])[None], n, axis=0) * rng.uniform(0.9, 1.1, size=(n, 1, 1))
        C = np.repeat(np.asarray(rec["C"])[None], n, axis=0) * (1 + 1e-3 * rng.uniform(-1, 1, size=(n, 6 * nU, 6 * nU)))
        r = timed(lambda: ctx.array_modal_batch(M, C))
        if not os.environ.get("BENCH_ARRAY_MODAL_NO_HOST"):
            t0 = time.perf_counter()
            for i in range(n):
                np.linalg.eig(np.linalg.solve(M[i], C[i]))
            r["numpy_host_loop_ms"] = 1e3 * (time.perf_counter() - t0)
        out["batch_nUnit%d" % nU] = r
    for name in ("pair", "square4", "ring6"):
        c = ac.cases()[name]
        nU = len(c["K_hs"])
        rep = lambda a: np.ascontiguousarray(np.repeat(np.asarray(a)[None], n, axis=0))
        M_unit = rep(np.asarray(gold[name]["M"])[:6, :6][None].repeat(nU, axis=0))
        out["moored_" + name] = timed(lambda: ctx.array_modal_moored(M_unit, rep(c["K_hs"]), rep(c["lines"]), rep(c["x_ref"]), ac.DEPTH))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
