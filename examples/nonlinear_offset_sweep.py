#!/usr/bin/env python
"""The mean offset of VolturnUS-S candidates over a thrust range, with the hydrostatics linearised at the zero pose
(staticsMod 0) and re-evaluated at every iterate (staticsMod 1), side by side (include/raftx_statics.h):

    python examples/nonlinear_offset_sweep.py [n_designs] [n_thrusts]

The candidates are ballast trimmed at the zero pose; staticsMod 0 takes K_hs and F0 of that pose from the resident design
set, staticsMod 1 takes the candidates' parameters, the trim's density correction and the rotor-nacelle assembly as a point
mass, and evaluates buoyancy and weight itself at every step.  A candidate on which the staticsMod 1 iteration does not
settle within the step cap is counted as flagged.

Runs on the committed fixtures (no reference tree needed)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raft_amd import backend, geometry as G, statics                     # noqa: E402
from raft_amd.sweep import VariantSweep                                  # noqa: E402
from raft_amd import snapshot as standin                                 # noqa: E402

HUB_HEIGHT, GRAV = 150.0, 9.81


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 500
    n_thrust = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    fg, c3 = standin.load_fixture("geom_units.npz"), standin.load_fixture("c3_variants.npz")
    base = json.loads(fg["c3_base_json"])
    moor = json.loads(str(np.load(os.path.join(standin.GOLDEN_DIR, "refgold_mooring.npz"))["VolturnUS-S/design"]))
    u0 = [u for u in fg["units"] if u["name"] == "C3-variant-0"][0]
    M_rna = np.asarray(u0["M_struc"]) - np.asarray(u0["M_struc_bare"])             # rotor-nacelle assembly: not geometry
    C_rna = np.asarray(u0["C_struc"]) - np.asarray(u0["C_struc_bare"])
    W_rna = np.asarray(u0["W_struc"]) - np.asarray(u0["W_struc_bare"])
    m = -W_rna[2] / GRAV                                                           # ... and as a point mass (m, x, y, z)
    rna = np.array([[m, W_rna[4] / (m * GRAV), -W_rna[3] / (m * GRAV), -C_rna[3, 3] / (m * GRAV)]])
    depth = float(c3["depth"])
    params = G.volturnus_params(np.random.default_rng(3).uniform(0.85, 1.15, size=(n, 5)))
    rep = lambda a: np.repeat(a[None], n, axis=0)
    sweep = VariantSweep(G.volturnus_program(base), params, rep(M_rna), np.zeros((n, 6, 6)), np.zeros((n, 6, 6)), c3["w"], c3["k"],
                         depth, np.asarray(c3["zeta"])[None], np.asarray(c3["beta"])[None], int(c3["nIter"]), float(c3["XiStart"]),
                         add_mask=G.ADD_MORISON | G.ADD_HYDROSTATIC | G.ADD_INERTIA | G.TRIM_BALLAST)
    ctx = backend.default_context(0)
    sweep.upload(ctx)                                                    # the candidates become the resident design set
    K_hs, F0, _ = statics.hydrostatics(ctx, C_extra=C_rna, F_extra=W_rna)
    drho = ctx.fetch_statics()["props"][:, G.SP_DRHO].copy()
    program = G.volturnus_mooring_program(moor)
    print("%d candidates; thrust at %g m.  surge [m] and pitch [deg]: median (min .. max) over the candidates both modes solve" % (n, HUB_HEIGHT))
    print("%10s | %-44s | %-44s | %s" % ("thrust MN", "staticsMod 0", "staticsMod 1", "flagged 0 / 1"))
    for thrust in np.linspace(0.2e6, 1.5e6, n_thrust):
        F_env = rep(np.array([thrust, 0.0, 0.0, 0.0, HUB_HEIGHT * thrust, 0.0]))
        lin = statics.mean_pose(ctx, K_hs, F0, depth=depth, program=program, params=params, F_env=F_env)
        non = statics.mean_pose(ctx, depth=depth, program=program, statics_mod=1, designs=params, point_masses=rna, drho=drho, F_env=F_env)
        ok = lin.ok & non.ok
        cell = lambda r: "n/a" if not ok.any() else "%6.2f (%6.2f .. %6.2f)  %5.2f (%5.2f .. %5.2f)" % (
            np.median(r.pose[ok, 0]), r.pose[ok, 0].min(), r.pose[ok, 0].max(),
            np.rad2deg(np.median(r.pose[ok, 4])), np.rad2deg(r.pose[ok, 4].min()), np.rad2deg(r.pose[ok, 4].max()))
        print("%10.2f | %-44s | %-44s | %d / %d" % (thrust / 1e6, cell(lin), cell(non), (~lin.ok).sum(), (~non.ok).sum()))


if __name__ == "__main__":
    main()
