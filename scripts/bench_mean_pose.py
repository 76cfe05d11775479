#!/usr/bin/env python
"""Cost of the mean-pose solve (include/raftx_statics.h): 10 000 VolturnUS-S variants x 3 lines with the fairleads on the
outer columns, the deck's hydrostatics and a thrust-like load of 0.2 .. 1.5 MN per variant.  Rounds alternate in one
process after a warm-up between
  device  raftx_mean_pose: the whole iteration in one launch,
  host    what a caller does without it: a Newton loop over raftx_mooring_lines (C_moor, F_moor at the current poses), the
          6 x 6 solves in numpy (batched), the step bounds, the same tolerances, as many rounds as the slowest design of
          the batch needs (every round evaluates the whole batch), and one more evaluation for T and J at the final poses.
Reported: the call times of both, the kernel time of the one launch between the library's events, the iteration counts,
and the largest difference between the two routes' poses.  One JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raft_amd import backend, geometry as G                              # noqa: E402
from raft_amd import snapshot as standin                                 # noqa: E402

CAPS = np.array([30.0, 30.0, 5.0, 0.1, 0.1, 0.1])
TOL = np.array([1e-9] * 3 + [1e-10] * 3)


def host_route(ctx, lines, depth, K_hs, F0, F_env, max_iter=40):
    n = len(K_hs)
    x = np.zeros((n, 6))
    rounds = 0
    while rounds < max_iter:
        m = ctx.mooring_lines(lines, depth, pose=x, want=("C", "F"))
        Y = F0 + F_env - np.einsum("dij,dj->di", K_hs, x) + m["F"]
        dX = np.linalg.solve(K_hs + m["C"], Y[:, :, None])[:, :, 0]
        s = np.minimum(1.0, (CAPS / np.maximum(np.abs(dX), 1e-300)).min(axis=1))
        dX *= s[:, None]
        x += dX
        rounds += 1
        if np.all(np.abs(dX) <= TOL):
            break
    m = ctx.mooring_lines(lines, depth, pose=x, want=("C", "F", "T", "J"))
    return x, m, rounds


def main():
    n = int(os.environ.get("BENCH_MEAN_POSE_N", 10000))
    rounds = int(os.environ.get("BENCH_MEAN_POSE_ROUNDS", 7))
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

    def device():
        t0 = time.perf_counter()
        r = ctx.mean_pose(K_hs, F0, depth, lines=lines, F_env=F_env)
        return time.perf_counter() - t0, ctx.last_kernel_ms(), r

    def device_program():
        t0 = time.perf_counter()
        r = ctx.mean_pose(K_hs, F0, depth, params=params, F_env=F_env)
        return time.perf_counter() - t0, ctx.last_kernel_ms(), r

    def host():
        t0 = time.perf_counter()
        x, m, nr = host_route(ctx, lines, depth, K_hs, F0, F_env)
        return time.perf_counter() - t0, nr, x

    for _ in range(2):
        device(), device_program(), host()
    td, tk, tp, th = [], [], [], []
    for _ in range(rounds):
        a = device()
        td.append(a[0]); tk.append(a[1])
        tp.append(device_program()[0])
        h = host()
        th.append(h[0])
    r = a[2]
    assert not r["flags"].any()
    ms = lambda v: [round(1e3 * float(min(v)), 4), round(1e3 * float(np.median(v)), 4), round(1e3 * float(max(v)), 4)]
    print(json.dumps({"metric": "mean_pose", "n_design": n, "n_line": 3, "rounds": rounds,
                      "device_call_ms_min_med_max": ms(td), "device_call_from_params_ms_min_med_max": ms(tp),
                      "device_kernel_ms_min_med_max": [round(float(min(tk)), 4), round(float(np.median(tk)), 4), round(float(max(tk)), 4)],
                      "host_route_ms_min_med_max": ms(th), "host_rounds": h[1],
                      "device_iterations_min_mean_max": [int(r["iterations"].min()), float(r["iterations"].mean()), int(r["iterations"].max())],
                      "max_pose_difference": float(np.abs(r["pose"] - h[2]).max()),
                      "max_surge_m": float(np.abs(r["pose"][:, 0]).max()), "max_pitch_deg": float(np.rad2deg(np.abs(r["pose"][:, 4]).max()))}))


if __name__ == "__main__":
    main()
