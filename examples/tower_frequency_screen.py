#!/usr/bin/env python
"""Screening stiffness variants of a FLEXIBLE tower on its first bending frequencies, on one MI355X: the reference's
VolturnUS-S-flexible deck (beam pontoons and a beam tower: 150 reduced degrees of freedom) with its elastic stiffness scaled,
the eigen analysis of every variant in ONE call (raft_amd.flex.FlexSweep.natural_modes, raftx_flex_modal_batch):

    python examples/tower_frequency_screen.py [n_variants]

1. the live model comes from the committed fixture (tests/golden/flex_volturnus.npz);
2. a variant is the unit with C_struc + C_hydro + C_moor + s C_elast, s from 0.5 to 1.5;
3. device: eig(solve(M_tot, C_tot)) of every variant, ascending, the twelve lowest modes returned;
4. host: the first two modes above the six rigid-body ones are the tower's first bending pair; the node motions T v say which
   is fore-aft (x) and which side-side (y); each is held against the rotor's 1P and 3P bands with a 10 % margin.

What the reference does one variant at a time with numpy.linalg.eig (FOWT.solveEigen, raft_fowt.py:1705-1714)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raft_amd import backend, dropin                                     # noqa: E402
from raft_amd.flex import FlexSweep, FlexUnit                            # noqa: E402
from raft_amd.snapshot import load_model_fixture, case_from_fixture      # noqa: E402

RPM = (5.0, 7.56)                        # operating range of the IEA 15 MW rotor
MARGIN = 0.10


def bands():
    one = np.array(RPM) / 60.0
    return {"1P": one * [1 - MARGIN, 1 + MARGIN], "3P": 3 * one * [1 - MARGIN, 1 + MARGIN]}


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    fx, model = load_model_fixture("flex_volturnus.npz")
    one = dropin.flex_sweep_from_models([model], [case_from_fixture(fx["cases"][0])])
    u0 = one.units[0]
    fowt = fx["model"]["fowts"][0]
    C_elast, T = np.asarray(fowt["C_elast"], dtype=float), np.asarray(fowt["T"], dtype=float)
    stiff = np.linspace(0.5, 1.5, n)
    units = [FlexUnit(u0.tables, u0.Tn, u0.M, u0.B, u0.C + (s - 1.0) * C_elast) for s in stiff]
    sweep = FlexSweep(units, one.w, one.k, one.depth, one.zeta, one.beta, one.nIter, one.XiStart, one.tol)
    ctx = backend.default_context(0)
    sweep.natural_modes(ctx)                                             # first call of the process: library start-up
    t0 = time.perf_counter()
    out = sweep.natural_modes(ctx, n_modes=12)
    dt = time.perf_counter() - t0
    print("%d variants x 150 DOFs: %.1f ms for the call, %.1f ms on the device; flagged: %d"
          % (n, 1e3 * dt, ctx.last_kernel_ms(), int(np.count_nonzero(out["flags"] & ~1))))
    print("bands with %.0f %% margin: " % (100 * MARGIN) + ", ".join("%s %.3f-%.3f Hz" % (k, b[0], b[1]) for k, b in bands().items()))
    for i in sorted(set(np.linspace(0, n - 1, min(n, 9)).astype(int).tolist())):
        pair = {}
        for j in (6, 7):                                                 # the first two modes above the rigid-body six
            node = (T @ out["modes"][i][:, j]).reshape(-1, 6)
            pair["fore-aft" if np.abs(node[:, 0]).sum() >= np.abs(node[:, 1]).sum() else "side-side"] = out["fn"][i, j]
        hits = [k for k, b in bands().items() for f in pair.values() if b[0] <= f <= b[1]]
        print("  elastic stiffness x %.2f: " % stiff[i] + ", ".join("%s %.4f Hz" % kv for kv in sorted(pair.items()))
              + ("   INSIDE " + "/".join(sorted(set(hits))) if hits else "   clear of 1P / 3P"))


if __name__ == "__main__":
    main()
