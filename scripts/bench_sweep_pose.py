#!/usr/bin/env python
"""Cost of the mean-pose request of a sweep crossing (raftx_sweep_mean_pose, include/raftx_statics.h) on the C3 stream:
batches of 10 000 VolturnUS-S variants x 200 bins, ballast trimmed, a thrust-like load of 0.2 .. 1.5 MN at 150 m per variant,
three lines with the fairleads on the outer columns.  Rounds alternate in one process after a warm-up between
  (a) the plain stream: the crossing at the reference pose, two batches in flight;
  (m) the stream with mooring= alone: the lines evaluated at the reference pose, C_moor in the stiffness -- the dynamics of (b)
      without its pose steps, so that (b) - (m) is what the pose costs;
  (b) the stream with mean_pose= + mooring=: hydrostatics, the solve, the second member pass and the lines at the solved pose
      inside the crossing, two batches in flight;
  (a3), (b3) as (a), (b) in the three-stage form -- launch(i+1), prepare(i+2), wait(i): a batch's phase 1, and with it the pose
      steps, is enqueued a whole step before its launch waits for the totals;
  (c) the host route (b) replaces, per batch: resident build at the reference pose, statics.hydrostatics (raftx_fetch_statics),
      statics.mean_pose, then the crossing with pose= that result and mooring=.  The variants' descriptors are expanded once,
      outside the timing (a route that draws new parameters per batch pays for that expansion too): a lower bound.
Reported per route: ms per batch (min / median / max over the rounds) and, for (a) and (b), the library's kernel times of the
last batch (generation incl. member passes | fused fixed point | statistics).  One JSON line."""
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


def main():
    n = int(os.environ.get("BENCH_SWEEP_POSE_N", 10000))
    rounds = int(os.environ.get("BENCH_SWEEP_POSE_ROUNDS", 7))
    nb = int(os.environ.get("BENCH_SWEEP_POSE_BATCHES", 6))
    fg = standin.load_fixture("geom_units.npz")
    c3 = standin.load_fixture("c3_variants.npz")
    base = json.loads(fg["c3_base_json"])
    moor = json.loads(str(np.load(os.path.join(standin.GOLDEN_DIR, "refgold_mooring.npz"))["VolturnUS-S/design"]))
    u0 = [u for u in fg["units"] if u["name"] == "C3-variant-0"][0]
    M_rna = np.asarray(u0["M_struc"]) - np.asarray(u0["M_struc_bare"])
    C_rna = np.asarray(u0["C_struc"]) - np.asarray(u0["C_struc_bare"])
    W_rna = np.asarray(u0["W_struc"]) - np.asarray(u0["W_struc_bare"])
    depth = float(c3["depth"])
    rng = np.random.default_rng(2)
    params = G.volturnus_params(rng.uniform(0.85, 1.15, size=(n, 5)))
    rep = lambda a: np.repeat(a[None], n, axis=0)
    sweep = VariantSweep(G.volturnus_program(base), params, rep(M_rna), np.zeros((n, 6, 6)), rep(C_rna), c3["w"], c3["k"], depth,
                         np.asarray(c3["zeta"])[None], np.asarray(c3["beta"])[None], int(c3["nIter"]), float(c3["XiStart"]),
                         add_mask=G.ADD_MORISON | G.ADD_HYDROSTATIC | G.ADD_INERTIA | G.TRIM_BALLAST)
    T = rng.uniform(0.2e6, 1.5e6, n)
    F_env = np.zeros((n, 6))
    F_env[:, 0], F_env[:, 4] = T, 150.0 * T
    mp = G.volturnus_mooring_program(moor)
    pose_req = dict(program=mp, C_extra=C_rna, F_extra=W_rna, F_env=F_env)
    ctx = backend.default_context(0)

    def stream(**kw):
        """nb batches, two in flight; (ms per batch, the last batch's results)."""
        t0 = time.perf_counter()
        h = sweep.submit_crossing(ctx, 0, **kw)
        for b in range(nb):
            h_next = sweep.submit_crossing(ctx, (b + 1) % 2, **kw) if b + 1 < nb else None
            out = sweep.wait_crossing(ctx, h)
            h = h_next
        return 1e3 * (time.perf_counter() - t0) / nb, out

    def stream3(**kw):
        """the same with the next batch but one prepared ahead: three slots"""
        t0 = time.perf_counter()
        cur = sweep.launch_crossing(ctx, sweep.prepare_crossing(ctx, 0, **kw))
        nxt = sweep.prepare_crossing(ctx, 1, **kw) if nb > 1 else None
        for b in range(nb):
            launched = sweep.launch_crossing(ctx, nxt) if nxt is not None else None
            nxt = sweep.prepare_crossing(ctx, (b + 2) % 3, **kw) if b + 2 < nb else None
            out = sweep.wait_crossing(ctx, cur)
            cur = launched
        return 1e3 * (time.perf_counter() - t0) / nb, out

    def host_route():
        t0 = time.perf_counter()
        for b in range(nb):
            sweep.pose = None
            sweep.upload(ctx)
            K_hs, F0, _ = statics.hydrostatics(ctx, C_extra=C_rna, F_extra=W_rna)
            res = statics.mean_pose(ctx, K_hs, F0, depth=depth, program=mp, params=params, F_env=F_env)
            sweep.pose = np.where(res.ok[:, None], res.pose, 0.0)
            out = sweep.wait_crossing(ctx, sweep.submit_crossing(ctx, 0, mooring=dict(program=mp)))
        sweep.pose = None
        return 1e3 * (time.perf_counter() - t0) / nb, out, res

    sweep.expanded_tables(ctx)                                            # (c)'s descriptors, once
    for _ in range(2):
        stream(), stream(mooring=dict(program=mp)), stream(mean_pose=pose_req, mooring=dict(program=mp)), host_route()
        stream3(), stream3(mean_pose=pose_req, mooring=dict(program=mp))
    ta, tm, tb, tc, ta3, tb3 = [], [], [], [], [], []
    for _ in range(rounds):
        a = stream()
        m = stream(mooring=dict(program=mp))
        tm.append(m[0])
        b = stream(mean_pose=pose_req, mooring=dict(program=mp))
        c = host_route()
        ta.append(a[0]); tb.append(b[0]); tc.append(c[0])
        ta3.append(stream3()[0])
        b3 = stream3(mean_pose=pose_req, mooring=dict(program=mp))
        tb3.append(b3[0])
    assert all(np.array_equal(b[1][k].view(np.uint8), b3[1][k].view(np.uint8)) for k in ("std", "niter", "pose", "T_std"))
    ok = b[1]["pose_flags"] == 0
    mmm = lambda v: [round(float(min(v)), 4), round(float(np.median(v)), 4), round(float(max(v)), 4)]
    print(json.dumps({"metric": "sweep_mean_pose", "n_design": n, "nw": len(c3["w"]), "batches_per_round": nb, "rounds": rounds,
                      "plain_stream_ms_per_batch_min_med_max": mmm(ta), "mooring_stream_ms_per_batch_min_med_max": mmm(tm),
                      "pose_stream_ms_per_batch_min_med_max": mmm(tb),
                      "plain_stream_three_stage_ms_per_batch_min_med_max": mmm(ta3),
                      "pose_stream_three_stage_ms_per_batch_min_med_max": mmm(tb3),
                      "host_route_ms_per_batch_min_med_max": mmm(tc),
                      "plain_last_batch_kernels_ms_gen_solve_stats": [round(float(v), 4) for v in a[1]["timing_ms"][1:]],
                      "mooring_last_batch_kernels_ms_gen_solve_stats": [round(float(v), 4) for v in m[1]["timing_ms"][1:]],
                      "fixed_point_iterations_mean_plain_mooring_pose": [float(a[1]["niter"].mean()), float(m[1]["niter"].mean()),
                                                                         float(b[1]["niter"][ok].mean())],
                      "strips_total_plain_pose": [int(a[1]["strip_off"][-1]), int(b[1]["strip_off"][-1])],
                      "pose_last_batch_kernels_ms_gen_solve_stats": [round(float(v), 4) for v in b[1]["timing_ms"][1:]],
                      "flagged": int((~ok).sum()),
                      "newton_steps_min_mean_max": [int(b[1]["pose_iterations"][ok].min()), float(b[1]["pose_iterations"][ok].mean()),
                                                    int(b[1]["pose_iterations"][ok].max())],
                      "max_surge_m": float(np.abs(b[1]["pose"][ok, 0]).max()),
                      "pitch_deg_min_max": [float(np.rad2deg(b[1]["pose"][ok, 4].min())), float(np.rad2deg(b[1]["pose"][ok, 4].max()))],
                      "strips_changed_designs": int((np.diff(a[1]["strip_off"]) != np.diff(b[1]["strip_off"])).sum())}))


if __name__ == "__main__":
    main()
