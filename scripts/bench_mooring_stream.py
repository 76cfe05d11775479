#!/usr/bin/env python
"""Cost of the quasi-static mooring lines (include/raftx_mooring.h) on the C3 stream: 10 000 VolturnUS-S variants x 200
bins per batch, 3 lines per variant with the fairleads on the outer columns, two batches in flight on rotating slots.
Rounds alternate in one process after a warm-up between
  plain    the stream without a request,
  mooring  mooring=dict(program=..): lines from the batch's parameters on the device, C_moor into C0, T_std,
  host     what the request replaces, as far as this repository can make it: C_moor and the [nD,6,3,6] tension rows are
           given (computed once, outside the timing -- MoorPy's own time is not part of it), added / laid out on the host
           per batch and uploaded with channels=.
Then raftx_mooring_lines / raftx_mooring_expand as calls, and the two kernels alone from the library's events.  One JSON
line.  Kernel placement: rocprofv3 --kernel-trace in a run of its own with BENCH_MOORING_STEPS=3 BENCH_MOORING_ROUNDS=1."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raft_amd import backend, geometry as G                              # noqa: E402
from raft_amd import snapshot as standin                                 # noqa: E402
from raft_amd.sweep import VariantSweep                                  # noqa: E402


def make_sweep(n, seed):
    fg = standin.load_fixture("geom_units.npz")
    c3 = standin.load_fixture("c3_variants.npz")
    base = json.loads(fg["c3_base_json"])
    u0 = [u for u in fg["units"] if u["name"] == "C3-variant-0"][0]
    M_rna = np.asarray(u0["M_struc"]) - np.asarray(u0["M_struc_bare"])
    C_rest = np.asarray(u0["C_struc"]) - np.asarray(u0["C_struc_bare"])
    params = G.volturnus_params(np.random.default_rng(seed).uniform(0.75, 1.25, size=(n, 5)))
    rep = lambda a: np.repeat(a[None], n, axis=0)
    return VariantSweep(G.volturnus_program(base), params, rep(M_rna), np.zeros((n, 6, 6)), rep(C_rest), c3["w"], c3["k"],
                        float(c3["depth"]), np.asarray(c3["zeta"])[None], np.asarray(c3["beta"])[None], int(c3["nIter"]),
                        float(c3["XiStart"]))


def stream(ctx, sw, draws, steps, submit):
    h = submit(0, draws[0])
    t0 = time.perf_counter()
    for b in range(steps):
        h_next = submit((b + 1) % 2, draws[(b + 1) % len(draws)])
        sw.wait_crossing(ctx, h)
        h = h_next
    sw.wait_crossing(ctx, h)
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    n = int(os.environ.get("BENCH_MOORING_N", 10000))
    steps, rounds = int(os.environ.get("BENCH_MOORING_STEPS", 10)), int(os.environ.get("BENCH_MOORING_ROUNDS", 4))
    ctx = backend.default_context(0)
    sw = make_sweep(n, 0)
    moor = json.loads(str(np.load(os.path.join(standin.GOLDEN_DIR, "refgold_mooring.npz"))["VolturnUS-S/design"]))
    mp = G.volturnus_mooring_program(moor)
    MOOR = dict(program=mp)
    draws = [make_sweep(n, s).params for s in (1, 2, 3)]
    C_base = sw.C0
    sw.wait_crossing(ctx, sw.submit_crossing(ctx, 0, mooring=MOOR))          # installs both programs
    given = []
    for p in draws:                                                        # the host route's inputs, outside the timing
        m = ctx.mooring_lines(ctx.mooring_expand(p), sw.depth, want=("C", "J"))
        given.append((m["C"], m["J"]))

    def plain(slot, p):
        sw.set_params(p)
        return sw.submit_crossing(ctx, slot)

    def mooring(slot, p):
        sw.set_params(p)
        return sw.submit_crossing(ctx, slot, mooring=MOOR)

    def host(slot, p):
        sw.set_params(p)
        Cm, J = given[[i for i, q in enumerate(draws) if q is p][0]]
        sw.C0 = C_base + Cm
        L = np.zeros((n, J.shape[1], 3, 6))
        L[:, :, 0, :] = J
        h = sw.submit_crossing(ctx, slot, channels=dict(L=L))
        sw.C0 = C_base
        return h

    forms = (("plain", plain), ("mooring", mooring), ("host", host))
    for _, f in forms:
        stream(ctx, sw, draws, 4, f)
    ms = {k: [] for k, _ in forms}
    for _ in range(rounds):
        for k, f in forms:
            ms[k].append(stream(ctx, sw, draws, steps, f))
    lines = ctx.mooring_expand(draws[0])
    te, tk, tc = [], [], []
    for _ in range(9):
        t0 = time.perf_counter()
        lines = ctx.mooring_expand(draws[0])
        te.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        res = ctx.mooring_lines(lines, sw.depth, want=("C", "J"))
        tc.append(time.perf_counter() - t0)
        tk.append(ctx.last_kernel_ms())
    assert not res["flags"].any()
    print(json.dumps({"metric": "c3_stream_mooring", "n_design": n, "n_line": 3, "nw": len(sw.w), "steps": steps, "rounds": rounds,
                      "ms_per_step": ms, "median_ms": {k: float(np.median(v)) for k, v in ms.items()},
                      "kernels_ms": float(np.median(tk)), "kernels_ms_range": [min(tk), max(tk)],
                      "call_C_and_J_ms": 1e3 * float(np.median(tc)), "expand_call_ms": 1e3 * float(np.median(te))}))


if __name__ == "__main__":
    main()
