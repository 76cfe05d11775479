#!/usr/bin/env python
"""The mean offset of every candidate of a VolturnUS-S sweep under a thrust-like load (Model.solveStatics for every
candidate in one launch; include/raftx_statics.h):

    python examples/mean_offset_sweep.py [n_designs] [thrust_N] [current_m_per_s]

The candidates' hydrostatics come from the geometry generator (the resident design set of the sweep, ballast trimmed),
their three lines from the mooring program fed the candidates' parameters (the fairleads follow the outer columns), the
load is a thrust at hub height and, with a current speed, the candidates' own mean current load (raftx_current_loads).
Printed: the range of the mean surge offset and pitch, the worst line tension at the offset pose, and the candidate with
the smallest offset.

Runs on the committed fixtures (no reference tree needed)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raft_amd import backend, geometry as G, statics                     # noqa: E402
from raft_amd.sweep import VariantSweep                                  # noqa: E402
from raft_amd import snapshot as standin                                 # noqa: E402

HUB_HEIGHT = 150.0


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    thrust = float(sys.argv[2]) if len(sys.argv) > 2 else 1.5e6
    current = float(sys.argv[3]) if len(sys.argv) > 3 else 0.0
    fg = standin.load_fixture("geom_units.npz")
    c3 = standin.load_fixture("c3_variants.npz")
    base = json.loads(fg["c3_base_json"])
    moor = json.loads(str(np.load(os.path.join(standin.GOLDEN_DIR, "refgold_mooring.npz"))["VolturnUS-S/design"]))
    u0 = [u for u in fg["units"] if u["name"] == "C3-variant-0"][0]
    M_rna = np.asarray(u0["M_struc"]) - np.asarray(u0["M_struc_bare"])             # rotor-nacelle assembly: not geometry
    C_rna = np.asarray(u0["C_struc"]) - np.asarray(u0["C_struc_bare"])
    W_rna = np.asarray(u0["W_struc"]) - np.asarray(u0["W_struc_bare"])
    depth = float(c3["depth"])
    params = G.volturnus_params(np.random.default_rng(3).uniform(0.85, 1.15, size=(n, 5)))
    rep = lambda a: np.repeat(a[None], n, axis=0)
    sweep = VariantSweep(G.volturnus_program(base), params, rep(M_rna), np.zeros((n, 6, 6)), np.zeros((n, 6, 6)), c3["w"], c3["k"],
                         depth, np.asarray(c3["zeta"])[None], np.asarray(c3["beta"])[None], int(c3["nIter"]), float(c3["XiStart"]),
                         add_mask=G.ADD_MORISON | G.ADD_HYDROSTATIC | G.ADD_INERTIA | G.TRIM_BALLAST)
    ctx = backend.default_context(0)
    sweep.upload(ctx)                                                    # the candidates become the resident design set
    cur = dict(speed=current, heading=0.0, depth=depth) if current > 0 else None
    K_hs, F0, F_env = statics.hydrostatics(ctx, C_extra=C_rna, F_extra=W_rna, current=cur)
    load = np.array([thrust, 0.0, 0.0, 0.0, HUB_HEIGHT * thrust, 0.0])
    F_env = np.repeat(load[None], n, axis=0) + (0.0 if F_env is None else F_env)
    program = G.volturnus_mooring_program(moor)
    statics.mean_pose(ctx, K_hs, F0, depth=depth, program=program, params=params, F_env=F_env)      # warm-up
    t0 = time.perf_counter()
    res = statics.mean_pose(ctx, K_hs, F0, depth=depth, program=program, params=params, F_env=F_env)
    dt = time.perf_counter() - t0
    ok = res.ok
    print("%d candidates: mean pose in %.2f ms (kernel %.3f ms), %d..%d Newton steps, %d flagged"
          % (n, 1e3 * dt, ctx.last_kernel_ms(), res.iterations[ok].min(), res.iterations[ok].max(), (~ok).sum()))
    for d in np.flatnonzero(~ok)[:5]:
        print("   candidate %d: %s" % (d, ", ".join(res.describe_flags(d))))
    surge, pitch, worst = res.pose[ok, 0], np.rad2deg(res.pose[ok, 4]), res.T[ok].max(axis=1)
    print("mean surge %.2f .. %.2f m, heave %.2f .. %.2f m, pitch %.2f .. %.2f deg; worst line tension %.3g .. %.3g N"
          % (surge.min(), surge.max(), res.pose[ok, 2].min(), res.pose[ok, 2].max(), pitch.min(), pitch.max(), worst.min(), worst.max()))
    i = np.flatnonzero(ok)[int(np.argmin(np.hypot(res.pose[ok, 0], res.pose[ok, 1])))]
    print("smallest offset %.2f m (pitch %.2f deg, worst tension %.3g N, residual %.2g N) for (ccD, ocD, T, ocR, pH) = %s"
          % (np.hypot(*res.pose[i, :2]), np.rad2deg(res.pose[i, 4]), res.T[i].max(), np.abs(res.F_res[i, :3]).max(), np.round(params[i], 2)))


if __name__ == "__main__":
    main()
