#!/usr/bin/env python
"""Cost of raftx_mooring_lines and raftx_mean_pose on SINGLE-ROW batches -- the batch of profiles/mooring_ab.txt and
profiles/mean_pose_ab.txt: 10 000 VolturnUS-S variants x 3 lines with the fairleads on the outer columns, the deck's
hydrostatics and a thrust-like load per variant -- for an A/B of two builds of the library (RAFTX_HIP_LIB selects one; run
the two alternately, one process each), and with BENCH_CHAINS=1 the same variants with every line cut into 3 rows of its own
properties (9 rows per design) for the record.  Reported per entry point: the kernel time between the library's events and
the call time, min / median / max over the rounds after a warm-up.  One JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raft_amd import backend, geometry as G                              # noqa: E402
from raft_amd import snapshot as standin                                 # noqa: E402


def main():
    n = int(os.environ.get("BENCH_N", 10000))
    rounds = int(os.environ.get("BENCH_ROUNDS", 9))
    ctx = backend.default_context(0)
    base = json.loads(standin.load_fixture("geom_units.npz")["c3_base_json"])
    moor = json.loads(str(np.load(os.path.join(standin.GOLDEN_DIR, "refgold_mooring.npz"))["VolturnUS-S/design"]))
    ctx.variant_program(G.volturnus_program(base))
    ctx.mooring_program(G.volturnus_mooring_program(moor))
    rng = np.random.default_rng(0)
    params = np.ascontiguousarray(G.volturnus_params(rng.uniform(0.75, 1.25, size=(n, 5))), dtype=float)
    stat = standin.load_fixture("refgold_statics.npz")["cases"][1]               # VolturnUS-S
    K_hs = np.repeat((np.asarray(stat["true_C_struc"]) + np.asarray(stat["true_C_hydro"]))[None], n, 0)
    F0 = np.repeat((np.asarray(stat["true_W_struc"]) + np.asarray(stat["true_W_hydro"]))[None], n, 0)
    thrust, head = rng.uniform(0.2e6, 1.5e6, n), np.deg2rad(rng.uniform(-45.0, 45.0, n))
    F_env = np.zeros((n, 6))
    F_env[:, 0], F_env[:, 1] = thrust * np.cos(head), thrust * np.sin(head)
    F_env[:, 3], F_env[:, 4] = -150.0 * F_env[:, 1], 150.0 * F_env[:, 0]
    depth = 200.0
    lines = ctx.mooring_expand(params)
    forms = {"single": lines}
    if os.environ.get("BENCH_CHAINS"):
        cut = np.zeros((n, 9, 16))
        for l in range(3):
            for i, f in enumerate((0.9, 0.05, 0.05)):         # the resting length stays inside the anchor-side row at every pose
                row = cut[:, 3 * l + i]
                row[:, 6], row[:, 7], row[:, 8] = f * lines[:, l, 6], lines[:, l, 7], lines[:, l, 8]
                if i:
                    row[:, 15] = 1.0
                else:
                    row[:, :6] = lines[:, l, :6]
        forms["chains"] = cut

    def lines_call(rec):
        t0 = time.perf_counter()
        r = ctx.mooring_lines(rec, depth, want=("C", "F", "T", "J"))
        return time.perf_counter() - t0, ctx.last_kernel_ms(), r

    def pose_call(rec):
        t0 = time.perf_counter()
        r = ctx.mean_pose(K_hs, F0, depth, lines=rec, F_env=F_env)
        return time.perf_counter() - t0, ctx.last_kernel_ms(), r

    out = {"metric": "mooring_chains_ab", "library": os.environ.get("RAFTX_HIP_LIB", "built"), "n_design": n, "rounds": rounds}
    for _ in range(3):
        for rec in forms.values():
            lines_call(rec), pose_call(rec)
    t = {(f, k): [] for f in forms for k in ("lines_kernel", "lines_call", "pose_kernel", "pose_call")}
    for _ in range(rounds):
        for f, rec in forms.items():
            a, b = lines_call(rec), pose_call(rec)
            assert not a[2]["flags"].any() and not b[2]["flags"].any(), (f, np.bincount(a[2]["flags"]), np.bincount(b[2]["flags"]))
            t[f, "lines_kernel"].append(a[1]); t[f, "lines_call"].append(1e3 * a[0])
            t[f, "pose_kernel"].append(b[1]); t[f, "pose_call"].append(1e3 * b[0])
    for (f, k), v in t.items():
        out["%s_%s_ms_min_med_max" % (f, k)] = [round(float(min(v)), 4), round(float(np.median(v)), 4), round(float(max(v)), 4)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
