#!/usr/bin/env python
"""The variant stream of examples/moored_sweep.py with every mooring line ending in a two-leg bridle on neighbouring columns:

    python examples/bridle_mooring_sweep.py [n_designs_per_batch] [n_batches]

raft_amd.geometry.volturnus_bridle_program turns the VolturnUS-S deck into three bridles -- per bridle a stem row and two leg
rows (include/raftx_mooring.h) -- whose leg fairleads follow the outer columns from the batch's parameters, as the single
lines' fairleads do in geometry.volturnus_mooring_program.  Every candidate's bridles are solved on the device (the junction of
each by its own Newton iteration), C_moor -- condensed through the junctions, the fairleads of a bridle coupled -- enters the
candidate's stiffness ahead of the add-up, and the mean tensions and the standard deviations of J Xi come back for both ends
of every row.  The same batches are crossed with the single-line deck.  Printed for a handful of candidates: the yaw stiffness
C_moor[5,5] and mean + 3 sigma of the worst leg tension, beside the single-line deck's yaw stiffness and worst line tension.

Runs on the committed fixtures (no reference tree needed)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raft_amd import backend, geometry as G                              # noqa: E402
from raft_amd.mooring import ML_LEG                                      # noqa: E402
from raft_amd.sweep import VariantSweep                                  # noqa: E402
from raft_amd import snapshot as standin                                 # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    n_batches = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    fg = standin.load_fixture("geom_units.npz")
    c3 = standin.load_fixture("c3_variants.npz")
    base = json.loads(fg["c3_base_json"])
    moor = json.loads(str(np.load(os.path.join(standin.GOLDEN_DIR, "refgold_mooring.npz"))["VolturnUS-S/design"]))
    bridles, singles = G.volturnus_bridle_program(moor), G.volturnus_mooring_program(moor)
    legs = np.flatnonzero(bridles.lines[:, ML_LEG] != 0)
    leg_ends = np.concatenate([legs, bridles.n + legs])                  # ends A (junction) and B (fairlead) of the leg rows
    u0 = [u for u in fg["units"] if u["name"] == "C3-variant-0"][0]
    M_rna = np.asarray(u0["M_struc"]) - np.asarray(u0["M_struc_bare"])
    C_rest = np.asarray(u0["C_struc"]) - np.asarray(u0["C_struc_bare"])             # no mooring constant: C_moor per candidate
    rng = np.random.default_rng(2)
    draw = lambda: G.volturnus_params(rng.uniform(0.75, 1.25, size=(n, 5)))
    rep = lambda a: np.repeat(a[None], n, axis=0)
    sweep = VariantSweep(G.volturnus_program(base), draw(), rep(M_rna), np.zeros((n, 6, 6)), rep(C_rest), np.asarray(c3["w"]),
                         np.asarray(c3["k"]), float(c3["depth"]), np.asarray(c3["zeta"])[None], np.asarray(c3["beta"])[None],
                         int(c3["nIter"]), float(c3["XiStart"]))
    ctx = backend.default_context(0)
    for s_, prog in enumerate((bridles, singles)):                       # warm-up: code objects, buffers, the chip's clock
        sweep.wait_crossing(ctx, sweep.submit_crossing(ctx, s_, mooring=dict(program=prog)))
    shown, flagged, t_bridle = [], 0, 0.0
    for b in range(n_batches):
        sweep.set_params(draw())
        t0 = time.perf_counter()
        hb = sweep.submit_crossing(ctx, 0, mooring=dict(program=bridles))
        hs = sweep.submit_crossing(ctx, 1, mooring=dict(program=singles))
        ob = sweep.wait_crossing(ctx, hb)
        t_bridle += time.perf_counter() - t0
        os_ = sweep.wait_crossing(ctx, hs)
        flagged += int(np.count_nonzero(ob["moor_flags"]))
        good = np.flatnonzero((ob["moor_flags"] == 0) & (os_["moor_flags"] == 0))
        for i in good[:2]:
            t3b = (ob["T_mean"] + 3.0 * ob["T_std"][:, 0, :])[i, leg_ends].max()
            t3s = (os_["T_mean"] + 3.0 * os_["T_std"][:, 0, :])[i].max()
            shown.append((sweep.params[i].copy(), ob["C_moor"][i, 5, 5], t3b, os_["C_moor"][i, 5, 5], t3s))
    print("%d batches x %d candidates, three bridles (%d rows) and the single-line deck: %.2f ms per bridle batch; %d candidates flagged"
          % (n_batches, n, bridles.n, 1e3 * t_bridle / n_batches, flagged))
    print("(ccD, ocD, T, ocR, pH)                    yaw stiffness C_moor[5,5] [N m/rad]     worst tension, mean + 3 sigma [N]")
    print("                                          bridles        single lines            worst leg      worst single line")
    for p, cb, tb, c1, t1 in shown:
        print("%-40s  %.4g      %.4g               %.4g      %.4g" % (np.round(p, 2), cb, c1, tb, t1))


if __name__ == "__main__":
    main()
