#!/usr/bin/env python
"""Screening a stream of VolturnUS-S candidates on their natural periods as well as their motions, all on one MI355X:

    python examples/modal_screen.py [n_designs_per_batch] [n_batches]

As examples/variant_stream.py (five parameters per candidate in, statistics out), but every batch also carries its eigen
analysis (modal=True: raftx_sweep_modal on the batch's generated M_struc + A_morison + RNA and C_struc + C_hydro +
mooring).  A candidate whose heave, roll or pitch period falls inside the wave band (5-25 s) is rejected on the device's
numbers, as an optimiser constraining omdao_raft.py's rigid_body_periods would; the smallest pitch std among the
admissible candidates is tracked.  Runs on the committed fixtures (no reference tree needed)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raft_amd import backend, geometry as G                              # noqa: E402
from raft_amd.sweep import VariantSweep, periods                         # noqa: E402
from raft_amd import snapshot as standin                                 # noqa: E402

BAND = (5.0, 25.0)                    # wave band [s]
HEAVE, ROLL, PITCH = 2, 3, 4


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    n_batches = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    fg = standin.load_fixture("geom_units.npz")
    c3 = standin.load_fixture("c3_variants.npz")
    base = json.loads(fg["c3_base_json"])
    u0 = [u for u in fg["units"] if u["name"] == "C3-variant-0"][0]
    M_rna = np.asarray(u0["M_struc"]) - np.asarray(u0["M_struc_bare"])
    C_rest = np.asarray(u0["C_struc"]) - np.asarray(u0["C_struc_bare"]) + np.diag([7e4, 7e4, 0, 0, 0, 1e8])
    rng = np.random.default_rng(2)
    draw = lambda: G.volturnus_params(rng.uniform(0.75, 1.25, size=(n, 5)))
    rep = lambda a: np.repeat(a[None], n, axis=0)
    sweep = VariantSweep(G.volturnus_program(base), draw(), rep(M_rna), np.zeros((n, 6, 6)), rep(C_rest), c3["w"], c3["k"],
                         float(c3["depth"]), np.asarray(c3["zeta"])[None], np.asarray(c3["beta"])[None], int(c3["nIter"]),
                         float(c3["XiStart"]))
    ctx = backend.default_context(0)
    for _ in range(4):                                                    # untimed: the process's start is not the stream's rate
        sweep.wait_crossing(ctx, sweep.submit_crossing(ctx, 0, modal=True))
        sweep.set_params(draw())
    best = (np.inf, None, None)
    seen = admissible = 0
    params_in_flight = {0: sweep.params}
    t0 = time.perf_counter()
    h = sweep.submit_crossing(ctx, 0, modal=True)
    for b in range(n_batches):
        h_next = None
        if b + 1 < n_batches:
            sweep.set_params(draw())
            params_in_flight[(b + 1) % 2] = sweep.params
            h_next = sweep.submit_crossing(ctx, (b + 1) % 2, modal=True)
        out = sweep.wait_crossing(ctx, h)
        T = periods(out["fn"])                                            # NaN where the device flagged the system
        in_band = np.any((T[:, [HEAVE, ROLL, PITCH]] >= BAND[0]) & (T[:, [HEAVE, ROLL, PITCH]] <= BAND[1]), axis=1)
        ok = (out["modal_flags"] == 0) & ~in_band & (out["flags"][:, 0] & 1).astype(bool)
        seen += n
        admissible += int(ok.sum())
        pitch = np.where(ok, out["std"][:, 0, PITCH], np.inf)
        i = int(np.argmin(pitch))
        if pitch[i] < best[0]:
            best = (float(pitch[i]), params_in_flight[b % 2][i].copy(), T[i].copy())
        h = h_next
    dt = time.perf_counter() - t0
    print("%d batches x %d candidates in %.1f ms (%.2f ms per batch, statistics + eigen analysis); %d of %d admissible"
          % (n_batches, n, 1e3 * dt, 1e3 * dt / n_batches, admissible, seen))
    if best[1] is not None:
        print("smallest admissible pitch std %.3f deg for (ccD, ocD, T, ocR, pH) = %s, periods [s] %s"
              % (best[0], np.round(best[1], 2), np.round(best[2], 1)))


if __name__ == "__main__":
    main()
