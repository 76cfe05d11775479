#!/usr/bin/env python
"""Cost of the eigen analysis (include/raftx_modal.h) on the C3 stream: 10 000 VolturnUS-S variants x 200 bins per batch,
as bench.py's default, two batches in flight on rotating slots.  Steps with and without modal=True alternate in one
process after a warm-up; then raftx_modal_batch alone on 10 000 and 100 000 systems.  One JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raft_amd import backend                                             # noqa: E402
from tests.test_hip_modal import _variant_sweep, _realistic              # noqa: E402


def stream(ctx, sw, draws, modal, steps):
    """ms per batch of a stream of ``steps`` batches (the next one submitted before the last one is waited for)."""
    h = sw.submit_crossing(ctx, 0, modal=modal)
    t0 = time.perf_counter()
    for b in range(steps):
        sw.set_params(draws[b % len(draws)])
        h_next = sw.submit_crossing(ctx, (b + 1) % 2, modal=modal)
        sw.wait_crossing(ctx, h)
        h = h_next
    sw.wait_crossing(ctx, h)
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    n, steps, rounds = 10000, int(os.environ.get("BENCH_MODAL_STEPS", 10)), int(os.environ.get("BENCH_MODAL_ROUNDS", 4))
    ctx = backend.default_context(0)
    sw = _variant_sweep(n, seed=0)
    draws = [_variant_sweep(n, seed=s).params for s in (1, 2, 3)]
    stream(ctx, sw, draws, False, 4)
    stream(ctx, sw, draws, True, 4)
    base, mod = [], []
    for _ in range(rounds):
        base.append(stream(ctx, sw, draws, False, steps))
        mod.append(stream(ctx, sw, draws, True, steps))
    rates = {}
    rng = np.random.default_rng(0)
    for m in (10000, 100000):
        M, C = _realistic(rng, m)
        ctx.modal_batch(M, C)
        ts, ks = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            ctx.modal_batch(M, C)
            ts.append(time.perf_counter() - t0)
            ks.append(ctx.last_kernel_ms())
        rates[m] = dict(call_designs_per_s=m / min(ts), kernel_ms=float(np.median(ks)))
    print(json.dumps({"metric": "c3_stream_modal", "n_design": n, "nw": 200, "steps": steps, "rounds": rounds,
                      "ms_per_step_plain": base, "ms_per_step_modal": mod,
                      "median_plain_ms": float(np.median(base)), "median_modal_ms": float(np.median(mod)),
                      "modal_batch_10k": rates[10000], "modal_batch_100k": rates[100000]}))


if __name__ == "__main__":
    main()
