#!/usr/bin/env python
"""Cost of the output channels of a crossing (include/raftx_channels.h) on the C3 stream: 10 000 VolturnUS-S variants x 200
bins per batch, as bench.py's default.  Three arms alternate, round by round, in one process after a warm-up:
    plain      the stream as bench.py runs it, two batches in flight on rotating slots
    channels   the same with channels=dict(L=..): the ten shared rows of a one-rotor unit with six line-end tensions
               (three hub accelerations, the tower-base moment, six rows of a tension Jacobian)
    want_Xi    what a caller had to do before: the responses out (192 MB per batch) into page-locked arrays on four
               rotating slots, two batches in flight -- the host arithmetic that would follow is not counted
Median and range of the ms per batch of every arm.  One JSON line.

The kernel time comes from a run of its own under the profiler (a few steps are enough), k_sweep_channels beside
k_motion_stats, which reads the same responses:
    BENCH_CHANNELS_STEPS=3 BENCH_CHANNELS_ROUNDS=1 rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_channels.py
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


def unit_rows():
    """Ten rows with the structure and magnitudes of dropin.sweep_output_rows of a 15 MW unit with three lines."""
    zhub, m, h, zcg, icg = 150.0, 2.3e6, 80.0, 95.0, 4.0e9
    L = np.zeros((10, 3, 6))
    L[0, 2, [0, 4]] = 1.0, zhub                               # AxRNA: surge + zhub pitch, on (i w)^2
    L[1, 2, [1, 3]] = 1.0, -zhub
    L[2, 2, 2] = 1.0
    L[3, 0, 4] = m * 9.81 * h                                 # Mbase: weight, inertial reaction
    L[3, 2, 0] = -m * h
    L[3, 2, 4] = -(m * h * zcg + icg)
    L[4:, 0, :] = np.random.default_rng(0).normal(size=(6, 6)) * np.array([1e5, 1e5, 1e5, 1e6, 1e6, 1e6])
    return L


def stream(ctx, sw, draws, steps, channels=None, Xi=None):
    """ms per batch of a stream of ``steps`` batches (the next one submitted before the last one is waited for); Xi: the
    page-locked response arrays of the slots, which then rotate over all of them."""
    nslot = 2 if Xi is None else len(Xi)
    kw = lambda s: dict(channels=channels, Xi_out=None if Xi is None else Xi[s])
    h = sw.submit_crossing(ctx, 0, **kw(0))
    t0 = time.perf_counter()
    for b in range(steps):
        sw.set_params(draws[b % len(draws)])
        s = (b + 1) % nslot
        h_next = sw.submit_crossing(ctx, s, **kw(s))
        sw.wait_crossing(ctx, h)
        h = h_next
    sw.wait_crossing(ctx, h)
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    n, steps, rounds = 10000, int(os.environ.get("BENCH_CHANNELS_STEPS", 10)), int(os.environ.get("BENCH_CHANNELS_ROUNDS", 4))
    ctx = backend.default_context(0)
    sw = _variant_sweep(n, seed=0)
    draws = [_variant_sweep(n, seed=s).params for s in (1, 2, 3)]
    CH = dict(L=unit_rows())
    Xi = [ctx.pinned_empty((n, 1, 1, 6, sw.nw)) for _ in range(4)]
    arms = {"plain": {}, "channels": dict(channels=CH), "want_Xi": dict(Xi=Xi)}
    for kw in arms.values():
        stream(ctx, sw, draws, 6, **kw)
    ms = {name: [] for name in arms}
    for _ in range(rounds):
        for name, kw in arms.items():
            ms[name].append(stream(ctx, sw, draws, steps, **kw))
    out = {"metric": "c3_stream_channels", "n_design": n, "nw": int(sw.nw), "n_channel": 10, "steps": steps, "rounds": rounds}
    for name in arms:
        out["ms_per_step_" + name] = ms[name]
        out["median_%s_ms" % name] = float(np.median(ms[name]))
        out["range_%s_ms" % name] = [float(min(ms[name])), float(max(ms[name]))]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
