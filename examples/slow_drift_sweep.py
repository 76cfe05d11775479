#!/usr/bin/env python
"""Slow drift of a handful of VolturnUS-S candidates on one MI355X, from five parameters per candidate:

    python examples/slow_drift_sweep.py [n_designs]

The reference's potSecOrder == 1 flow (raft_model.py:1108-1131; FOWT.calcQTF_slenderBody, raft_fowt.py:1988-2078) for a
VariantSweep: the first-order tables AND the second-order strip / member records are generated on the device from the
parameters (VariantSweep.run_second_order with qtf_tables=None: raftx_qtf_tables_build_variants +
raftx_qtf_slender_resident), no FOWT object is built per candidate.  Per candidate the script prints the standard
deviations of surge and pitch of the first-order solution against the solution with the second-order force -- the slow
drift Max_Offset and Max_PtfmPitch of omdao_raft.py:870-872 are sensitive to.
Runs on the committed fixtures (no reference tree needed)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raft_amd import backend, geometry as G, waves                        # noqa: E402
from raft_amd.sweep import VariantSweep                                  # noqa: E402
from raft_amd import snapshot as standin                                 # noqa: E402


def sigma(Xi):
    """Standard deviations [nD,nCase,6] of response amplitudes Xi [nD,nCase,nHead,6,nw] (helpers.py getRMS)."""
    return np.sqrt(0.5 * np.sum(np.abs(Xi) ** 2, axis=(2, 4)))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    fg = standin.load_fixture("geom_units.npz")
    c3 = standin.load_fixture("c3_variants.npz")
    base = json.loads(fg["c3_base_json"])
    u0 = [u for u in fg["units"] if u["name"] == "C3-variant-0"][0]
    M_rna = np.asarray(u0["M_struc"]) - np.asarray(u0["M_struc_bare"])
    C_rest = np.asarray(u0["C_struc"]) - np.asarray(u0["C_struc_bare"]) + np.diag([7e4, 7e4, 0, 0, 0, 1e8])
    w, k, depth = np.asarray(c3["w"]), np.asarray(c3["k"]), float(c3["depth"])
    zeta = np.stack([np.asarray(c3["zeta"]), 0.5 * np.asarray(c3["zeta"])])           # two sea states
    beta = np.stack([np.asarray(c3["beta"]), np.asarray(c3["beta"]) + 0.4])
    dw = float(w[1] - w[0])
    S0 = 0.5 * np.abs(zeta[:, 0, :]) ** 2 / dw                                        # the spectra the amplitudes came from
    w2 = np.linspace(w[0], min(w[-1], 1.6), 40)                                       # second-order grid (min_freq2nd .. max_freq2nd)
    k2 = np.array([waves.wave_number(x, depth) for x in w2])
    params = G.volturnus_params(np.random.default_rng(2).uniform(0.85, 1.15, size=(n, 5)))
    rep = lambda a: np.repeat(a[None], n, axis=0)
    sweep = VariantSweep(G.volturnus_program(base), params, rep(M_rna), np.zeros((n, 6, 6)), rep(C_rest), w, k, depth, zeta, beta,
                         max(int(c3["nIter"]), 15), float(c3["XiStart"]))         # enough iterations for both stages
    ctx = backend.default_context(0)
    first = sweep.run(ctx)
    both = sweep.run_second_order(ctx, None, None, w2, k2, S0)
    s1, s2 = sigma(first["Xi"]), sigma(both["Xi"])
    print("%d candidates x %d sea states, %d-point second-order grid; sigma first order -> with the second-order force" % (n, 2, len(w2)))
    for d in range(n):
        for c in range(2):
            print("candidate %2d sea state %d: surge %.3f -> %.3f m   pitch %.3f -> %.3f deg   (|F2| max %.3e N)%s"
                  % (d, c, s1[d, c, 0], s2[d, c, 0], np.rad2deg(s1[d, c, 4]), np.rad2deg(s2[d, c, 4]),
                     np.abs(both["Fhydro_2nd"][d, c, 0]).max(), "" if both["flags"][d, c] & 1 else "   not converged"))


if __name__ == "__main__":
    main()
