"""Second-order tables from descriptors, measured once (profiles/qtf_tables_ab.txt):

    python scripts/bench_qtf_tables.py [n_designs] [nw2] [reps]

For n C3 variants (default 10 000), a second-order grid of nw2 points (default 40) and one sea state, device events around
each of
  * raftx_qtf_tables_build_variants: parameters in, records resident (the three generator kernels, the scan, the
    expansion of the descriptors and the read-back of the offsets between the passes),
  * raftx_qtf_slender_resident on them (set -> table index, k_qtf_tables, k_qtf_pairs; Xi given, no Kim & Yue members),
  * the upload of the SAME records (fetched once) from page-locked host memory to the device,
each repeated `reps` times after a warm-up, median and spread.  Prints one JSON line.  Kernel names for a trace:
k_qtfgen_member, k_qtfgen_design, k_qtfgen_scan, k_qtfgen_write, k_geom_expand, k_qtfgen_sets, k_qtf_tables, k_qtf_pairs."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raft_amd import backend, geometry as G, waves                        # noqa: E402
from raft_amd import snapshot as standin                                 # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    nw2 = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    import torch
    fg = standin.load_fixture("geom_units.npz")
    P = G.volturnus_program(json.loads(fg["c3_base_json"]))
    params = G.volturnus_params(np.random.default_rng(2).uniform(0.75, 1.25, size=(n, 5)))
    ctx = backend.default_context(0)
    ctx.variant_program(P)
    w2 = np.linspace(0.15, 1.6, nw2)
    k2 = np.array([waves.wave_number(x, 200.0) for x in w2])
    rng = np.random.default_rng(5)
    amp = np.array([1.0, 0.3, 0.7, 0.01, 0.02, 0.004])[None, :, None] / (1.0 + (w2[None, None, :] / 0.6) ** 2)
    Xi = amp * np.exp(1j * (rng.uniform(0, 6, (n, 6, 1)) + 1.5 * w2[None, None, :]))
    Ms = np.repeat(np.asarray(fg["units"][4]["M_struc"])[None], n, axis=0)
    t_build, t_qtf, t_wall = [], [], []
    for i in range(reps + 1):                                             # the first round is the warm-up
        t0 = time.perf_counter()
        soff, moff = ctx.qtf_tables_build_variants(params)
        t_wall.append(1e3 * (time.perf_counter() - t0))
        t_build.append(ctx.last_kernel_ms())
        ctx.qtf_slender_resident(Xi, [0.3], w2, k2, 200.0, 1025.0, 9.81, Ms, Nm=0, fetch=False)
        t_qtf.append(ctx.last_kernel_ms())
    _, strips, _, members, _, _ = ctx.qtf_tables_fetch(raw=True)
    hs, hm = torch.from_numpy(strips).pin_memory(), torch.from_numpy(members).pin_memory()
    ds, dm = torch.empty_like(hs, device="cuda"), torch.empty_like(hm, device="cuda")
    t_up = []
    for i in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ds.copy_(hs, non_blocking=True)
        dm.copy_(hm, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        t_up.append(e0.elapsed_time(e1))
    med = lambda a: float(np.median(a[1:]))
    rng_ = lambda a: [float(np.min(a[1:])), float(np.max(a[1:]))]
    print(json.dumps({"n_designs": n, "nw2": nw2, "n_case": 1, "reps": reps, "strips": int(soff[-1]), "members": int(moff[-1]),
                      "record_bytes": int(strips.nbytes + members.nbytes),
                      "tables_build_device_ms": med(t_build), "tables_build_device_ms_range": rng_(t_build),
                      "tables_build_call_wall_ms": med(t_wall),
                      "qtf_slender_resident_device_ms": med(t_qtf), "qtf_slender_resident_device_ms_range": rng_(t_qtf),
                      "records_upload_pinned_ms": med(t_up), "records_upload_pinned_ms_range": rng_(t_up)}))


if __name__ == "__main__":
    main()
