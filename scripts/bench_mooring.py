#!/usr/bin/env python
"""A/B of two builds of the library on the mooring entry points (RAFTX_HIP_LIB selects one; run the two alternately, one
process each) -- the batch of profiles/mooring_ab.txt and its successors: 10 000 VolturnUS-S variants x 3 lines with the
fairleads on the outer columns, the deck's hydrostatics and a thrust-like load per variant.  The forms of that batch:
  single   the three single lines (always)
  chains   BENCH_CHAINS=1: every line cut into 3 rows of its own properties (9 rows per design)
  bridles  BENCH_BRIDLES=1: every line ending in a two-leg bridle on neighbouring columns (9 rows per design)
  arrays   where the library has the entry points: BENCH_ARRAYS (1 000; 0: none) four-unit arrays of 16 rows -- the square of
           tests/array_mooring_cases.py, every array with shared lines of its own length
each through its lines entry (raftx_mooring_lines / raftx_array_mooring_lines: C, F, T, J) and its pose entry (raftx_mean_pose
/ raftx_array_mean_pose).  Reported per form and entry: the kernel time between the library's events and the call time,
min / median / max over BENCH_ROUNDS (9; 0: no timing) rounds after three of warm-up.  One JSON line.

BENCH_DUMP=<file.npz> also runs the small batteries of tests/mooring_cases.py, mooring_chain_cases.py, mooring_bridle_cases.py
and array_mooring_cases.py (accuracy batches, mixed designs, flag cases) through the same entries and saves every output;
``--compare a.npz b.npz`` then reports, per key, whether two such files agree byte for byte (NaN payloads included)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    keys = sorted(set(a.files) | set(b.files))
    bad = 0
    for k in keys:
        if k not in a.files or k not in b.files:
            verdict = "only in %s" % (path_a if k in a.files else path_b)
        else:
            x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
            same = x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.reshape(-1).view(np.uint8), y.reshape(-1).view(np.uint8))
            verdict = "identical" if same else "DIFFERENT"
        bad += verdict != "identical"
        print("%-90s %s" % (k, verdict))
    print("%d keys, %d not identical" % (len(keys), bad))
    return 1 if bad else 0


def hydrostatics(standin):
    stat = standin.load_fixture("refgold_statics.npz")["cases"][1]               # VolturnUS-S
    return (np.asarray(stat["true_C_struc"]) + np.asarray(stat["true_C_hydro"]),
            np.asarray(stat["true_W_struc"]) + np.asarray(stat["true_W_hydro"]))


def dump(ctx, path, K1, F1):
    """Every output of the four entry points on the small batteries of the tests' case modules."""
    from tests import array_mooring_cases as ac, mooring_bridle_cases as bc, mooring_cases as mc, mooring_chain_cases as cc
    out = {}

    def unit(key, lines, pose, depth):
        lines = np.ascontiguousarray(lines, dtype=float)
        n = len(lines)
        pose = None if pose is None else np.ascontiguousarray(np.broadcast_to(pose, (n, 6)), dtype=float)
        for k, v in ctx.mooring_lines(lines, depth, pose=pose).items():
            out["%s/lines/%s" % (key, k)] = v
        r = ctx.mean_pose(np.repeat(K1[None], n, 0), np.repeat(F1[None], n, 0), depth, lines=lines, x_ref=pose)
        for k, v in r.items():
            out["%s/pose/%s" % (key, k)] = v

    for name, lines, pose, depth in mc.batches():
        unit("single/" + name, lines, pose, depth)
    for name, lines, pose, depth in cc.batches():
        unit("chains/" + name, lines, pose, depth)
    for name, rows, depth, _ in cc.flag_cases():
        unit("chains/flag/" + name, rows, None, depth)
    for (depth, nrow), group in bc.accuracy_batch().items():
        unit("bridles/accuracy-%g-%d" % (depth, nrow), [g[2] for g in group], np.array([g[3] for g in group]), depth)
    for name, (rows, depth) in (("mixed", bc.mixed_design()), ("two_singles", bc.bridle_two_singles())):
        unit("bridles/" + name, [rows] * len(bc.POSES), np.array(bc.POSES), depth)
    for name, (rows, depth, pose, _) in bc.FLAGS.items():
        unit("bridles/flag/" + name, [bc.ACCURACY["symmetric_200"][0], rows, bc.ACCURACY["clump"][0]], pose, depth)
    if getattr(ctx.rlib, "has_array_mooring", False):
        batches = [(n, ac.batch([n])) for n in ac.cases()] + [("pairs", ac.batch(["pair", "pair_thrust", "pair_grounded", "pair_yaw_pitch"]))]
        for name, b in batches:
            for k, v in ctx.array_mooring_lines(b["lines"], b["x_ref"], b["depth"]).items():
                out["arrays/%s/lines/%s" % (name, k)] = v
            for k, v in ctx.array_mean_pose(b["K_hs"], b["F0"], b["x_ref"], b["depth"], b["lines"], F_env=b["F_env"]).items():
                out["arrays/%s/pose/%s" % (name, k)] = v
    np.savez(path, **{k: np.asarray(v) for k, v in out.items() if v is not None})
    return len(out)


def main():
    from raft_amd import backend, geometry as G, mooring
    from raft_amd import snapshot as standin
    n = int(os.environ.get("BENCH_N", 10000))
    n_arr = int(os.environ.get("BENCH_ARRAYS", 1000))
    rounds = int(os.environ.get("BENCH_ROUNDS", 9))
    ctx = backend.default_context(0)
    # one set-up: the variant program, the hydrostatics, the thrust-like load
    base = json.loads(standin.load_fixture("geom_units.npz")["c3_base_json"])
    moor = json.loads(str(np.load(os.path.join(standin.GOLDEN_DIR, "refgold_mooring.npz"))["VolturnUS-S/design"]))
    ctx.variant_program(G.volturnus_program(base))
    ctx.mooring_program(G.volturnus_mooring_program(moor))
    rng = np.random.default_rng(0)
    params = np.ascontiguousarray(G.volturnus_params(rng.uniform(0.75, 1.25, size=(n, 5))), dtype=float)
    K1, F1 = hydrostatics(standin)
    K_hs, F0 = np.repeat(K1[None], n, 0), np.repeat(F1[None], n, 0)
    thrust, head = rng.uniform(0.2e6, 1.5e6, n), np.deg2rad(rng.uniform(-45.0, 45.0, n))
    F_env = np.zeros((n, 6))
    F_env[:, 0], F_env[:, 1] = thrust * np.cos(head), thrust * np.sin(head)
    F_env[:, 3], F_env[:, 4] = -150.0 * F_env[:, 1], 150.0 * F_env[:, 0]
    depth = 200.0
    lines = ctx.mooring_expand(params)
    out = {"metric": "mooring_ab", "library": os.environ.get("RAFTX_HIP_LIB", "built"), "n_design": n, "rounds": rounds}

    def unit_form(rec):
        return (lambda: ctx.mooring_lines(rec, depth, want=("C", "F", "T", "J")),
                lambda: ctx.mean_pose(K_hs, F0, depth, lines=rec, F_env=F_env))

    forms = {"single": unit_form(lines)}
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
        forms["chains"] = unit_form(cut)
    if os.environ.get("BENCH_BRIDLES"):
        forms["bridles"] = unit_form(G.volturnus_bridle_program(moor).expand(params))
    if n_arr > 0 and getattr(ctx.rlib, "has_array_mooring", False):
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
        forms["arrays"] = (lambda: ctx.array_mooring_lines(arrays, x_ref, depth, want=("C", "F", "T", "J")),
                           lambda: ctx.array_mean_pose(Ka, Fa, x_ref, depth, arrays))
        out.update(n_array=n_arr, array_units=4, array_rows=int(arrays.shape[1]))
    # one timing loop
    calls = [(f, e, fn) for f, pair in forms.items() for e, fn in zip(("lines", "pose"), pair)]
    if rounds > 0:
        for _ in range(3):
            for _, _, fn in calls:
                fn()
    t = {(f, e, w): [] for f, e, _ in calls for w in ("kernel", "call")}
    for _ in range(rounds):
        for f, e, fn in calls:
            t0 = time.perf_counter()
            r = fn()
            t[f, e, "call"].append(1e3 * (time.perf_counter() - t0))
            t[f, e, "kernel"].append(ctx.last_kernel_ms())
            assert not r["flags"].any(), (f, e, np.bincount(r["flags"]))
            if e == "pose":
                out["%s_pose_iterations_max" % f] = int(r["iterations"].max())
    for (f, e, w), v in t.items():
        if v:
            out["%s_%s_%s_ms_min_med_max" % (f, e, w)] = [round(float(min(v)), 4), round(float(np.median(v)), 4), round(float(max(v)), 4)]
    if os.environ.get("BENCH_DUMP"):
        out["dump_keys"] = dump(ctx, os.environ["BENCH_DUMP"], K1, F1)
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main()
