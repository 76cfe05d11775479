#!/usr/bin/env python
"""Cost of the mean current loads (include/raftx_current.h) on the C3 stream: 10 000 VolturnUS-S variants x 200 bins per
batch, as bench.py's default, two batches in flight on rotating slots.  Rounds with and without current=dict(..) (three
currents) alternate in one process after a warm-up; then raftx_current_loads alone on the resident 10 000 designs (the
kernel's own time from the library's events).  One JSON line.

The kernel time comes from a run of its own under the profiler (a few steps are enough):
    BENCH_CURRENT_STEPS=3 BENCH_CURRENT_ROUNDS=1 rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_current.py
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raft_amd import backend                                             # noqa: E402
from tests.test_hip_modal import _variant_sweep                          # noqa: E402

CUR = dict(speed=[2.0, 0.6, 1.2], heading=[15.0, -70.0, 90.0])


def stream(ctx, sw, draws, current, steps):
    """ms per batch of a stream of ``steps`` batches (the next one submitted before the last one is waited for)."""
    h = sw.submit_crossing(ctx, 0, current=current)
    t0 = time.perf_counter()
    for b in range(steps):
        sw.set_params(draws[b % len(draws)])
        h_next = sw.submit_crossing(ctx, (b + 1) % 2, current=current)
        sw.wait_crossing(ctx, h)
        h = h_next
    sw.wait_crossing(ctx, h)
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    n, steps, rounds = 10000, int(os.environ.get("BENCH_CURRENT_STEPS", 10)), int(os.environ.get("BENCH_CURRENT_ROUNDS", 4))
    ctx = backend.default_context(0)
    sw = _variant_sweep(n, seed=0)
    draws = [_variant_sweep(n, seed=s).params for s in (1, 2, 3)]
    stream(ctx, sw, draws, None, 4)
    stream(ctx, sw, draws, CUR, 4)
    base, cur = [], []
    for _ in range(rounds):
        base.append(stream(ctx, sw, draws, None, steps))
        cur.append(stream(ctx, sw, draws, CUR, steps))
    sw.upload(ctx)
    sw.run_current(ctx, CUR["speed"], CUR["heading"])
    ts, ks = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        sw.run_current(ctx, CUR["speed"], CUR["heading"])
        ts.append(time.perf_counter() - t0)
        ks.append(ctx.last_kernel_ms())
    print(json.dumps({"metric": "c3_stream_current", "n_design": n, "nw": 200, "n_current": len(CUR["speed"]), "steps": steps,
                      "rounds": rounds, "ms_per_step_plain": base, "ms_per_step_current": cur,
                      "median_plain_ms": float(np.median(base)), "median_current_ms": float(np.median(cur)),
                      "resident_call_ms": 1e3 * min(ts), "resident_kernel_ms": float(np.median(ks))}))


if __name__ == "__main__":
    main()
