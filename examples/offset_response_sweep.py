#!/usr/bin/env python
"""Extreme pitch and line tension of every candidate of a VolturnUS-S sweep under a thrust-like load, each candidate linearised
at ITS OWN mean offset -- the reference's order solveStatics, setPosition, solveDynamics, mean + 3 sigma -- with no host work
per candidate:

    python examples/offset_response_sweep.py [n_designs_per_batch] [n_batches] [thrust_N]

Every batch is its candidates' five parameters.  Inside the crossing the library builds the candidates (ballast trimmed) at the
undisplaced pose, assembles their hydrostatics, solves the mean pose under the load with the lines of the mooring program
(raftx_sweep_mean_pose), runs the member pass again at that pose -- several degrees of pitch change which strips are wet --,
evaluates the lines there (raftx_sweep_mooring: C_moor into the stiffness, mean tensions, tension statistics) and solves the
fixed point.  The means come from the pose, the standard deviations from the crossing at it.  Two batches in flight.

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

HUB_HEIGHT = 150.0


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    n_batches = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    thrust = float(sys.argv[3]) if len(sys.argv) > 3 else 1.5e6
    fg = standin.load_fixture("geom_units.npz")
    c3 = standin.load_fixture("c3_variants.npz")
    base = json.loads(fg["c3_base_json"])
    moor = json.loads(str(np.load(os.path.join(standin.GOLDEN_DIR, "refgold_mooring.npz"))["VolturnUS-S/design"]))
    u0 = [u for u in fg["units"] if u["name"] == "C3-variant-0"][0]
    M_rna = np.asarray(u0["M_struc"]) - np.asarray(u0["M_struc_bare"])             # rotor-nacelle assembly: not geometry
    C_rna = np.asarray(u0["C_struc"]) - np.asarray(u0["C_struc_bare"])
    W_rna = np.asarray(u0["W_struc"]) - np.asarray(u0["W_struc_bare"])
    rng = np.random.default_rng(3)
    draw = lambda: G.volturnus_params(rng.uniform(0.85, 1.15, size=(n, 5)))
    rep = lambda a: np.repeat(a[None], n, axis=0)
    sweep = VariantSweep(G.volturnus_program(base), draw(), rep(M_rna), np.zeros((n, 6, 6)), rep(C_rna), c3["w"], c3["k"],
                         float(c3["depth"]), np.asarray(c3["zeta"])[None], np.asarray(c3["beta"])[None], int(c3["nIter"]),
                         float(c3["XiStart"]), add_mask=G.ADD_MORISON | G.ADD_HYDROSTATIC | G.ADD_INERTIA | G.TRIM_BALLAST)
    program = G.volturnus_mooring_program(moor)
    load = np.array([thrust, 0.0, 0.0, 0.0, HUB_HEIGHT * thrust, 0.0])
    sweep.mean_pose = dict(program=program, C_extra=C_rna, F_extra=W_rna, F_env=rep(load))     # standing requests of the sweep
    sweep.mooring = dict(program=program)
    ctx = backend.default_context(0)
    sweep.wait_crossing(ctx, sweep.submit_crossing(ctx, 0))               # the first batch of a process also pays for its start
    best = (np.inf, None, None)
    params_in_flight = {0: sweep.params}
    flagged = 0
    t0 = time.perf_counter()
    h = sweep.submit_crossing(ctx, 0)
    for b in range(n_batches):
        h_next = None
        if b + 1 < n_batches:
            sweep.set_params(draw())
            params_in_flight[(b + 1) % 2] = sweep.params
            h_next = sweep.submit_crossing(ctx, (b + 1) % 2)
        out = sweep.wait_crossing(ctx, h)
        ok = (out["pose_flags"] == 0) & (out["flags"][:, 0] & 1).astype(bool)        # a pose, and a converged fixed point
        flagged += int((~ok).sum())
        pitch = np.abs(np.rad2deg(out["pose"][:, 4])) + 3.0 * out["std"][:, 0, 4]    # deg: mean from the pose, sigma at it
        tension = (out["T_mean"] + 3.0 * out["T_std"][:, 0]).max(axis=1)             # N, worst line end
        pitch = np.where(ok, pitch, np.inf)
        i = int(np.argmin(pitch))
        if pitch[i] < best[0]:
            best = (float(pitch[i]), float(tension[i]), params_in_flight[b % 2][i].copy())
        if b == 0:
            print("first batch: mean pitch %.2f .. %.2f deg, mean + 3 sigma %.2f .. %.2f deg; worst tension mean + 3 sigma %.3g .. %.3g N; "
                  "%d .. %d Newton steps" % (np.rad2deg(out["pose"][ok, 4]).min(), np.rad2deg(out["pose"][ok, 4]).max(), pitch[ok].min(),
                                             pitch[ok].max(), tension[ok].min(), tension[ok].max(), out["pose_iterations"][ok].min(),
                                             out["pose_iterations"][ok].max()))
        h = h_next
    dt = time.perf_counter() - t0
    print("%d batches x %d candidates at their own mean pose in %.1f ms: %.2f ms per batch; %d candidates without a pose or a "
          "converged fixed point" % (n_batches, n, 1e3 * dt, 1e3 * dt / n_batches, flagged))
    print("smallest mean + 3 sigma pitch %.2f deg (worst tension %.3g N) for (ccD, ocD, T, ocR, pH) = %s"
          % (best[0], best[1], np.round(best[2], 2)))


if __name__ == "__main__":
    main()
