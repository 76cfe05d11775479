#!/usr/bin/env python
"""Cost of the mean-pose solve with hydrostatics at every iterate (raftx_mean_pose_nonlinear_variants, include/raftx_statics.h):
10 000 VolturnUS-S variants x 3 lines with the fairleads on the outer columns, ballast trimmed at the zero pose, the
rotor-nacelle assembly as a point mass, a thrust of 0.2 .. 1.5 MN at hub height per variant.  Rounds alternate in one process
after a warm-up between
  device  raftx_mean_pose_nonlinear_variants: the whole iteration in one launch,
  host    the route it replaces: per round raftx_build_designs(pose = the current poses) on the trimmed descriptors ->
          raftx_fetch_statics -> raftx_mooring_lines -> the point mass, the 6 x 6 solves and the step bounds in numpy, the
          same tolerances and step cap, as many rounds as the slowest design of the batch needs.
Reported: the call times of both, the kernel time of the one launch between the library's events, the iteration counts, the
flagged designs and the largest difference between the two routes' poses over the designs both converge on.  One JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raft_amd import backend, geometry as G                              # noqa: E402
from raft_amd import snapshot as standin                                 # noqa: E402
from raft_amd.sweep import VariantSweep                                  # noqa: E402

CAPS = np.array([30.0, 30.0, 5.0, 0.1, 0.1, 0.1])
TOL = np.array([1e-9] * 3 + [1e-10] * 3)
RHO, GRAV, HUB, DEPTH = 1025.0, 9.81, 150.0, 200.0


def point_mass(pm, x):
    """(W [n,6], C [n,6,6]) of ONE point mass pm = (m, r) at the poses x [n,6]: the formula of include/raftx_statics.h."""
    n = len(x)
    sr, cr, sp, cp, sy, cy = np.sin(x[:, 3]), np.cos(x[:, 3]), np.sin(x[:, 4]), np.cos(x[:, 4]), np.sin(x[:, 5]), np.cos(x[:, 5])
    R = np.array([[cy * cp, cy * sp * sr - cr * sy, sy * sr + cy * cr * sp], [cp * sy, cy * cr + sy * sp * sr, cr * sy * sp - cy * sr],
                  [-sp, cp * sr, cp * cr]]).transpose(2, 0, 1)
    r = np.asarray(pm[1:])
    a = R @ r
    f = np.zeros((n, 3))
    f[:, 2] = -pm[0] * GRAV
    W, C = np.zeros((n, 6)), np.zeros((n, 6, 6))
    W[:, :3], W[:, 3:] = f, np.cross(a, f)
    for j in range(3):
        tj = x[:, 3:].copy()
        tj[:, j] += 1.0
        C[:, 3:, 3 + j] -= np.cross(r + np.cross(tj, a) - a, f)
    return W, (C + C.transpose(0, 2, 1)) / 2


def host_route(ctx, T, lines, pm, F_env, max_iter):
    n = len(F_env)
    Z = np.zeros((n, 6, 6))
    x = np.zeros((n, 6))
    done = np.zeros(n, dtype=bool)
    rounds = 0
    while rounds < max_iter:
        ctx.build_designs(T.member_off, T.members, T.station_off, T.stations, Z, Z, Z, 1, pose=x, rho=RHO, g=GRAV, k=np.array([0.1]),
                          cap_off=T.cap_off, caps=T.caps)
        st = ctx.fetch_statics()
        m = ctx.mooring_lines(lines, DEPTH, pose=x, want=("C", "F"))
        Wp, Cp = point_mass(pm, x)
        Y = st["W_struc"] + st["W_hydro"] + Wp + F_env + m["F"]
        K = st["C_struc"] + st["C_hydro"] + Cp + m["C"]
        ok = np.all(np.isfinite(Y), axis=1) & np.all(np.isfinite(K), axis=(1, 2))
        K[~ok], Y[~ok] = np.eye(6), 0.0
        dX = np.linalg.solve(K, Y[:, :, None])[:, :, 0]
        dX *= np.minimum(1.0, (CAPS / np.maximum(np.abs(dX), 1e-300)).min(axis=1))[:, None]
        dX[done | ~ok] = 0.0                                      # (a finished design stays where it is, as on the device)
        x += dX
        rounds += 1
        done |= np.all(np.abs(dX) <= TOL, axis=1) & ok
        if done.all():
            break
    return x, done, rounds


def main():
    n = int(os.environ.get("BENCH_MEAN_POSE_N", 10000))
    rounds = int(os.environ.get("BENCH_MEAN_POSE_ROUNDS", 3))
    max_iter = int(os.environ.get("BENCH_MEAN_POSE_MAX_ITER", 40))
    ctx = backend.default_context(0)
    fg, c3 = standin.load_fixture("geom_units.npz"), standin.load_fixture("c3_variants.npz")
    base = json.loads(fg["c3_base_json"])
    moor = json.loads(str(np.load(os.path.join(standin.GOLDEN_DIR, "refgold_mooring.npz"))["VolturnUS-S/design"]))
    u0 = [u for u in fg["units"] if u["name"] == "C3-variant-0"][0]
    M_rna = np.asarray(u0["M_struc"]) - np.asarray(u0["M_struc_bare"])
    W_rna = np.asarray(u0["W_struc"]) - np.asarray(u0["W_struc_bare"])
    C_rna = np.asarray(u0["C_struc"]) - np.asarray(u0["C_struc_bare"])
    m_rna = -W_rna[2] / GRAV
    pm = np.array([m_rna, W_rna[4] / (m_rna * GRAV), -W_rna[3] / (m_rna * GRAV), -C_rna[3, 3] / (m_rna * GRAV)])
    rng = np.random.default_rng(0)
    params = np.ascontiguousarray(G.volturnus_params(rng.uniform(0.75, 1.25, size=(n, 5))), dtype=float)
    vp = G.volturnus_program(base)
    rep = lambda a: np.repeat(a[None], n, axis=0)
    sweep = VariantSweep(vp, params, rep(M_rna), np.zeros((n, 6, 6)), np.zeros((n, 6, 6)), c3["w"], c3["k"], DEPTH,
                         np.asarray(c3["zeta"])[None], np.asarray(c3["beta"])[None], int(c3["nIter"]), float(c3["XiStart"]),
                         add_mask=G.ADD_MORISON | G.ADD_HYDROSTATIC | G.ADD_INERTIA | G.TRIM_BALLAST)
    sweep.upload(ctx)                                             # the trim at the zero pose: drho of every variant
    drho = ctx.fetch_statics()["props"][:, G.SP_DRHO].copy()
    ctx.variant_program(vp)
    ctx.mooring_program(G.volturnus_mooring_program(moor))
    lines = ctx.mooring_expand(params)
    T = vp.tables(ctx.expand_variants(params), n)                 # the host route's descriptors, edited with the trim
    st = T.stations = np.array(T.stations)
    of_design = np.repeat(np.arange(n), np.diff(np.asarray(T.station_off)[np.asarray(T.member_off)]))
    st[st[:, G.GS_RHOFILL] == 0.0, G.GS_LFILL] = 0.0
    fill = st[:, G.GS_LFILL] > 0.0
    st[fill, G.GS_RHOFILL] += drho[of_design[fill]]
    thrust = rng.uniform(0.2e6, 1.5e6, n)
    F_env = np.zeros((n, 6))
    F_env[:, 0], F_env[:, 4] = thrust, HUB * thrust

    def device():
        t0 = time.perf_counter()
        r = ctx.mean_pose_nonlinear(DEPTH, params=params, rho=RHO, g=GRAV, drho=drho, point_masses=pm[None], F_env=F_env, max_iter=max_iter)
        return time.perf_counter() - t0, ctx.last_kernel_ms(), r

    def host():
        t0 = time.perf_counter()
        x, done, nr = host_route(ctx, T, lines, pm, F_env, max_iter)
        return time.perf_counter() - t0, nr, x, done

    device(), host()
    td, tk, th = [], [], []
    for _ in range(rounds):
        a = device()
        td.append(a[0]); tk.append(a[1])
        h = host()
        th.append(h[0])
    r = a[2]
    ok = (r["flags"] == 0) & h[3]
    it = r["iterations"][r["flags"] == 0]
    ms = lambda v: [round(1e3 * float(min(v)), 3), round(1e3 * float(np.median(v)), 3), round(1e3 * float(max(v)), 3)]
    flags, counts = np.unique(r["flags"], return_counts=True)
    print(json.dumps({"metric": "mean_pose_nonlinear", "n_design": n, "n_line": 3, "n_member": int(len(T.members) // n), "rounds": rounds,
                      "max_iter": max_iter, "device_call_ms_min_med_max": ms(td),
                      "device_kernel_ms_min_med_max": [round(float(min(tk)), 3), round(float(np.median(tk)), 3), round(float(max(tk)), 3)],
                      "host_route_ms_min_med_max": ms(th), "host_rounds": h[1],
                      "device_flags": {int(f): int(c) for f, c in zip(flags, counts)}, "host_converged": int(h[3].sum()),
                      "device_iterations_min_mean_max": [int(it.min()), round(float(it.mean()), 2), int(it.max())] if len(it) else None,
                      "max_pose_difference": float(np.abs(r["pose"][ok] - h[2][ok]).max()) if ok.any() else None,
                      "max_surge_m": float(np.abs(r["pose"][ok, 0]).max()) if ok.any() else None,
                      "max_pitch_deg": float(np.rad2deg(np.abs(r["pose"][ok, 4]).max())) if ok.any() else None}))


if __name__ == "__main__":
    main()
