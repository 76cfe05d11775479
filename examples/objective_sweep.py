#!/usr/bin/env python
"""The quantities a platform optimisation steers on, for a stream of VolturnUS-S candidates on one MI355X:

    python examples/objective_sweep.py [n_designs_per_batch] [n_batches]

As examples/variant_stream.py (five parameters per candidate in, statistics out), but every batch also carries its output
channels (channels=dict(L=..): raftx_sweep_channels): the nacelle accelerations and the tower-base bending moment of every
(candidate, sea state), 8 B per channel instead of the responses.  Per batch the script prints what omdao_raft.py:870-876
aggregates -- Max_PtfmPitch, max_nac_accel, max_tower_base, each the largest mean + 3 sigma over the sea states
(raft_fowt.py:2428-2431, 2534-2535) -- of the candidate with the smallest nacelle acceleration, and the batch's range.

The rows are those of raft_amd.dropin.sweep_output_rows of the base unit (one turbine on every variant: shared rows), as
recorded in tests/golden/refgold_sweep_outputs.npz; the means are host scalars of the base unit -- at the mean pitch
PITCH0 the nacelle sees |sin(PITCH0)| g and the tower base the weight moment L[Mbase,0,pitch] sin(PITCH0).
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

PITCH0 = np.deg2rad(0.0)              # mean pitch of the base unit in these sea states (no wind: upright)
GRAV = 9.81


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    n_batches = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    fg = standin.load_fixture("geom_units.npz")
    c3 = standin.load_fixture("c3_variants.npz")
    rows = standin.load_fixture("refgold_sweep_outputs.npz")["rows"]
    names, L = list(rows["names"]), np.asarray(rows["L"])
    iAx, iMb = names.index("AxRNA[0]"), names.index("Mbase[0]")
    mean_pitch, mean_acc, mean_mbase = np.rad2deg(PITCH0), abs(np.sin(PITCH0)) * GRAV, L[iMb, 0, 4] * np.sin(PITCH0)
    base = json.loads(fg["c3_base_json"])
    u0 = [u for u in fg["units"] if u["name"] == "C3-variant-0"][0]
    M_rna = np.asarray(u0["M_struc"]) - np.asarray(u0["M_struc_bare"])
    C_rest = np.asarray(u0["C_struc"]) - np.asarray(u0["C_struc_bare"]) + np.diag([7e4, 7e4, 0, 0, 0, 1e8])
    zeta = np.stack([np.asarray(c3["zeta"]), 0.5 * np.asarray(c3["zeta"])])          # two sea states
    beta = np.stack([np.asarray(c3["beta"]), np.asarray(c3["beta"]) + 0.4])
    rng = np.random.default_rng(2)
    draw = lambda: G.volturnus_params(rng.uniform(0.75, 1.25, size=(n, 5)))
    rep = lambda a: np.repeat(a[None], n, axis=0)
    sweep = VariantSweep(G.volturnus_program(base), draw(), rep(M_rna), np.zeros((n, 6, 6)), rep(C_rest), c3["w"], c3["k"],
                         float(c3["depth"]), zeta, beta, int(c3["nIter"]), float(c3["XiStart"]))
    CH = dict(L=L)
    ctx = backend.default_context(0)
    for _ in range(4):                                                    # untimed: the process's start is not the stream's rate
        sweep.wait_crossing(ctx, sweep.submit_crossing(ctx, 0, channels=CH))
        sweep.set_params(draw())
    t0 = time.perf_counter()
    h = sweep.submit_crossing(ctx, 0, channels=CH)
    for b in range(n_batches):
        h_next = None
        if b + 1 < n_batches:
            sweep.set_params(draw())
            h_next = sweep.submit_crossing(ctx, (b + 1) % 2, channels=CH)
        out = sweep.wait_crossing(ctx, h)
        ok = np.all(out["flags"] & 1, axis=1)                             # converged in every sea state
        pitch = np.max(mean_pitch + 3 * out["std"][:, :, 4], axis=1)      # Max_PtfmPitch [deg]
        acc = np.max(mean_acc + 3 * out["chan_std"][:, :, iAx], axis=1)   # max_nac_accel [m/s^2]
        mbase = np.max(mean_mbase + 3 * out["chan_std"][:, :, iMb], axis=1)   # max_tower_base [N m]
        i = int(np.argmin(np.where(ok, acc, np.inf)))
        print("batch %2d: %5d of %d converged | best candidate: Max_PtfmPitch %.2f deg, max_nac_accel %.3f m/s^2, max_tower_base %.3e N m"
              " | batch: %.2f-%.2f deg, %.3f-%.3f m/s^2, %.2e-%.2e N m"
              % (b, int(ok.sum()), n, pitch[i], acc[i], mbase[i], pitch[ok].min(), pitch[ok].max(), acc[ok].min(), acc[ok].max(),
                 mbase[ok].min(), mbase[ok].max()))
        h = h_next
    dt = time.perf_counter() - t0
    print("%d batches x %d candidates x 2 sea states in %.1f ms (%.2f ms per batch, motion statistics + %d output channels)"
          % (n_batches, n, 1e3 * dt, 1e3 * dt / n_batches, len(names)))


if __name__ == "__main__":
    main()
