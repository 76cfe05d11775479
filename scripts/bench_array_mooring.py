#!/usr/bin/env python
"""Cost of the array mooring entries (include/raftx_array_mooring.h) and, for an A/B of two builds of the library
(RAFTX_HIP_LIB selects one; run the two alternately, one process each), of the entry points that existed before them on the
batch of profiles/mooring_bridles_ab.txt: 10 000 VolturnUS-S variants x 3 single lines, raftx_mooring_lines (C, F, T, J) and
raftx_mean_pose under a thrust-like load per variant.  The new entries, where the library has them: 1 000 four-unit arrays
of 16 rows -- the square of tests/array_mooring_cases.py, every array with shared lines of its own length --
raftx_array_mooring_lines at the reference poses and raftx_array_mean_pose.  Reported per entry point: the kernel time
between the library's events and the call time, min / median / max over the rounds after a warm-up.  One JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raft_amd import backend, geometry as G, mooring                     # noqa: E402
from raft_amd import snapshot as standin                                 # noqa: E402


def timed(ctx, f):
    t0 = time.perf_counter()
    r = f()
    return 1e3 * (time.perf_counter() - t0), ctx.last_kernel_ms(), r


def main():
    n = int(os.environ.get("BENCH_N", 10000))
    n_arr = int(os.environ.get("BENCH_ARRAYS", 1000))
    rounds = int(os.environ.get("BENCH_ROUNDS", 9))
    ctx = backend.default_context(0)
    base = json.loads(standin.load_fixture("geom_units.npz")["c3_base_json"])
    moor = json.loads(str(np.load(os.path.join(standin.GOLDEN_DIR, "refgold_mooring.npz"))["VolturnUS-S/design"]))
    ctx.variant_program(G.volturnus_program(base))
    ctx.mooring_program(G.volturnus_mooring_program(moor))
    rng = np.random.default_rng(0)
    params = np.ascontiguousarray(G.volturnus_params(rng.uniform(0.75, 1.25, size=(n, 5))), dtype=float)
    stat = standin.load_fixture("refgold_statics.npz")["cases"][1]               # VolturnUS-S
    K1 = np.asarray(stat["true_C_struc"]) + np.asarray(stat["true_C_hydro"])
    F1 = np.asarray(stat["true_W_struc"]) + np.asarray(stat["true_W_hydro"])
    K_hs, F0 = np.repeat(K1[None], n, 0), np.repeat(F1[None], n, 0)
    thrust, head = rng.uniform(0.2e6, 1.5e6, n), np.deg2rad(rng.uniform(-45.0, 45.0, n))
    F_env = np.zeros((n, 6))
    F_env[:, 0], F_env[:, 1] = thrust * np.cos(head), thrust * np.sin(head)
    F_env[:, 3], F_env[:, 4] = -150.0 * F_env[:, 1], 150.0 * F_env[:, 0]
    depth = 200.0
    rec = ctx.mooring_expand(params)
    calls = {"lines": lambda: ctx.mooring_lines(rec, depth, want=("C", "F", "T", "J")),
             "pose": lambda: ctx.mean_pose(K_hs, F0, depth, lines=rec, F_env=F_env)}
    out = {"metric": "array_mooring_ab", "library": os.environ.get("RAFTX_HIP_LIB", "built"), "n_design": n, "rounds": rounds}
    if getattr(ctx.rlib, "has_array_mooring", False):
        deck, _ = mooring.lines_from_design(moor)
        side = 1600.0
        rad = side / np.sqrt(2.0)
        loc = np.round(rad * np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]]), 6)
        arrays = []
        for L in np.linspace(1488.0, 1494.0, n_arr):
            sh = []
            for i in range(4):
                d = (loc[(i + 1) % 4] - loc[i]) / side
                sh.append(dict(unitA=i, rA=(58.0 * d[0], 58.0 * d[1], -14.0), unitB=(i + 1) % 4, rB=(-58.0 * d[0], -58.0 * d[1], -14.0),
                               L=float(L), EA=2.0e8, w=300.0))
            arrays.append(mooring.array_lines([deck] * 4, loc, [0.0, 90.0, 180.0, 270.0], sh))
        arrays = np.ascontiguousarray(arrays)
        x_ref = np.zeros((n_arr, 4, 6))
        x_ref[:, :, :2] = loc
        Ka, Fa = np.ascontiguousarray(np.broadcast_to(K1, (n_arr, 4, 6, 6))), np.ascontiguousarray(np.broadcast_to(F1, (n_arr, 4, 6)))
        calls["array_lines"] = lambda: ctx.array_mooring_lines(arrays, x_ref, depth, want=("C", "F", "T", "J"))
        calls["array_pose"] = lambda: ctx.array_mean_pose(Ka, Fa, x_ref, depth, arrays)
        out.update(n_array=n_arr, array_units=4, array_rows=int(arrays.shape[1]))
    for _ in range(3):
        for f in calls.values():
            f()
    t = {(k, w): [] for k in calls for w in ("kernel", "call")}
    for _ in range(rounds):
        for k, f in calls.items():
            call, kern, r = timed(ctx, f)
            assert not r["flags"].any(), (k, np.bincount(r["flags"]))
            t[k, "kernel"].append(kern)
            t[k, "call"].append(call)
    for (k, w), v in t.items():
        out["%s_%s_ms_min_med_max" % (k, w)] = [round(float(min(v)), 4), round(float(np.median(v)), 4), round(float(max(v)), 4)]
    if "array_pose" in calls:
        out["array_pose_iterations_max"] = int(r["iterations"].max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
