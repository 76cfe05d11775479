#!/usr/bin/env python
"""The variant stream of examples/variant_stream.py with the mooring FOLLOWING the candidates, as raft/parametersweep.py
moves the three fairleads with the outer columns (:64-68, 79-83):

    python examples/moored_sweep.py [n_designs_per_batch] [n_batches]

The mooring edits go to the device once as a program (geometry.volturnus_mooring_program -> raftx_mooring_program); every
batch then carries mooring=dict(program=..): the library evaluates each candidate's three catenary lines from the batch's
parameters (raftx_sweep_mooring, include/raftx_mooring.h), adds C_moor to the candidate's stiffness on the device ahead of
the add-up -- in place of the constant diag(7e4, 7e4, 0, 0, 0, 1e8) every candidate used to be solved on -- and returns the
mean tensions and the standard deviations of J Xi beside the motions.  Printed: mean + 3 sigma of the worst line tension of
the candidate with the smallest pitch, beside that pitch.

Runs on the committed fixtures (no reference tree needed)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raft_amd import backend, geometry as G                              # noqa: E402
from raft_amd.sweep import VariantSweep                                  # noqa: E402
from raft_amd import snapshot as standin                                 # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    n_batches = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    fg = standin.load_fixture("geom_units.npz")
    c3 = standin.load_fixture("c3_variants.npz")
    base = json.loads(fg["c3_base_json"])
    moor = json.loads(str(np.load(os.path.join(standin.GOLDEN_DIR, "refgold_mooring.npz"))["VolturnUS-S/design"]))
    u0 = [u for u in fg["units"] if u["name"] == "C3-variant-0"][0]
    M_rna = np.asarray(u0["M_struc"]) - np.asarray(u0["M_struc_bare"])
    C_rest = np.asarray(u0["C_struc"]) - np.asarray(u0["C_struc_bare"])             # no mooring constant: C_moor per candidate
    depth = float(c3["depth"])
    rng = np.random.default_rng(2)
    draw = lambda: G.volturnus_params(rng.uniform(0.75, 1.25, size=(n, 5)))
    rep = lambda a: np.repeat(a[None], n, axis=0)
    sweep = VariantSweep(G.volturnus_program(base), draw(), rep(M_rna), np.zeros((n, 6, 6)), rep(C_rest), c3["w"], c3["k"],
                         depth, np.asarray(c3["zeta"])[None], np.asarray(c3["beta"])[None], int(c3["nIter"]), float(c3["XiStart"]))
    ctx = backend.default_context(0)
    MOOR = dict(program=G.volturnus_mooring_program(moor))
    for s_ in range(2):                                                  # warm-up: code objects, buffers, the chip's clock
        sweep.wait_crossing(ctx, sweep.submit_crossing(ctx, s_, mooring=MOOR))
        sweep.set_params(draw())
    best = (np.inf, None, None)
    t0 = time.perf_counter()
    cur = (sweep.submit_crossing(ctx, 0, mooring=MOOR), sweep.params)
    for b in range(n_batches):
        nxt = None
        if b + 1 < n_batches:
            sweep.set_params(draw())
            nxt = (sweep.submit_crossing(ctx, (b + 1) % 2, mooring=MOOR), sweep.params)
        h, params = cur
        out = sweep.wait_crossing(ctx, h)
        good = (out["flags"][:, 0] & 1).astype(bool) & (out["moor_flags"] == 0)   # converged, and every line solved
        pitch = np.where(good, out["std"][:, 0, 4], np.inf)                # Max_PtfmPitch's ingredient: the pitch std of the case
        t3 = out["T_mean"] + 3.0 * out["T_std"][:, 0, :]                   # mean + 3 sigma of every line end
        i = int(np.argmin(pitch))
        if pitch[i] < best[0]:
            best = (float(pitch[i]), params[i].copy(), float(t3[i].max()))
        cur = nxt
    dt = time.perf_counter() - t0
    print("%d batches x %d candidates with their own mooring in %.1f ms: %.2f ms per batch" % (n_batches, n, 1e3 * dt, 1e3 * dt / n_batches))
    print("smallest pitch std %.3f deg for (ccD, ocD, T, ocR, pH) = %s; worst line tension mean + 3 sigma %.3g N"
          % (best[0], np.round(best[1], 2), best[2]))


if __name__ == "__main__":
    main()
