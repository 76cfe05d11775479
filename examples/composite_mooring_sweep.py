#!/usr/bin/env python
"""The variant stream of examples/moored_sweep.py in 600 m of water on chain - rope - chain lines with a clump weight:

    python examples/composite_mooring_sweep.py [n_designs_per_batch] [n_batches]

The VolturnUS-S mooring section is edited as a deep-water deck would be written: per line an anchor chain, a polyester rope and
a top chain joined at two ``free`` points, the lower of which carries a clump weight.  raft_amd.mooring.chains_from_design
turns it into row records -- a head row and two continuation rows per line (include/raftx_mooring.h) --, and the program moves
the head rows' fairleads with the outer columns as examples/moored_sweep.py does for single lines.  Every candidate's three
composite lines are then solved on the device from the batch's parameters, C_moor enters the candidate's stiffness ahead of
the add-up, and the mean tensions and the standard deviations of J Xi come back for BOTH ends of EVERY segment.  Printed:
mean + 3 sigma of the worst segment-end tension of the candidate with the smallest pitch, and which row and end it is.

Runs on the committed fixtures (no reference tree needed)."""
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raft_amd import backend, geometry as G                              # noqa: E402
from raft_amd.mooring import ML_CONT, MooringProgram, chains_from_design, tension_names   # noqa: E402
from raft_amd.sweep import VariantSweep                                  # noqa: E402
from raft_amd import snapshot as standin                                 # noqa: E402

DEPTH = 600.0


def deep_water_deck(design):
    """The deck's three lines as anchor chain 600 m - rope 1000 m - top chain 100 m in DEPTH, anchors at 1600 m."""
    d = copy.deepcopy(design)
    moor = d["mooring"]
    moor["water_depth"] = DEPTH
    moor["line_types"].append(dict(name="polyester", diameter=0.2, mass_density=63.0, stiffness=5.0e8))
    lines = []
    for k, head in enumerate((180.0, 60.0, 300.0), start=1):
        c, s = np.cos(np.deg2rad(head)), np.sin(np.deg2rad(head))
        for p in moor["points"]:
            if p["name"] == "line%d_anchor" % k:
                p["location"] = [1600.0 * c, 1600.0 * s, -DEPTH]
        # the free points' locations are MoorPy's starting guesses; the device does not need them
        moor["points"].append(dict(name="line%d_clump" % k, type="free", location=[1000.0 * c, 1000.0 * s, -DEPTH + 20.0], m=20000.0, v=2.5))
        moor["points"].append(dict(name="line%d_joint" % k, type="free", location=[150.0 * c, 150.0 * s, -100.0]))
        lines += [dict(name="line%d_anchor_chain" % k, endA="line%d_anchor" % k, endB="line%d_clump" % k, type="chain", length=600.0),
                  dict(name="line%d_rope" % k, endA="line%d_clump" % k, endB="line%d_joint" % k, type="polyester", length=1000.0),
                  dict(name="line%d_top_chain" % k, endA="line%d_joint" % k, endB="line%d_vessel" % k, type="chain", length=100.0)]
    moor["lines"] = lines
    return d


def mooring_program(rows):
    """The fairleads of the head rows on the outer face of the outer columns (geometry.volturnus_mooring_program)."""
    P = MooringProgram(rows, 5)
    c = lambda c0=0.0, ccD=0.0, ocD=0.0, T=0.0, ocR=0.0, pH=0.0: [c0, ccD, ocD, T, ocR, pH]
    const = lambda v: c(float(v))
    heads = [l for l in range(len(rows)) if rows[l, ML_CONT] == 0]
    for l, (cx, cy) in zip(heads, ((-1.0, None), (np.cos(np.deg2rad(60)), np.sin(np.deg2rad(60))),
                                   (np.cos(np.deg2rad(300)), np.sin(np.deg2rad(300))))):
        a, f = rows[l, 0:3], rows[l, 3:6]
        fy = const(f[1]) if cy is None else c(ocD=0.5 * cy, ocR=cy)
        P.ends(l, [const(a[0]), const(a[1]), const(a[2])], [c(ocD=0.5 * cx, ocR=cx), fy, const(f[2])])
    return P


def wave_numbers(w, depth, g=9.81):
    """k of w^2 = g k tanh(k depth), by Newton from the deep-water value."""
    w = np.asarray(w, dtype=float)
    k = w * w / g
    for _ in range(50):
        t = np.tanh(k * depth)
        k = k - (g * k * t - w * w) / (g * t + g * k * depth * (1 - t * t))
    return k


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    n_batches = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    fg = standin.load_fixture("geom_units.npz")
    c3 = standin.load_fixture("c3_variants.npz")
    base = json.loads(fg["c3_base_json"])
    moor = json.loads(str(np.load(os.path.join(standin.GOLDEN_DIR, "refgold_mooring.npz"))["VolturnUS-S/design"]))
    rows, depth, row_names = chains_from_design(deep_water_deck(moor))
    u0 = [u for u in fg["units"] if u["name"] == "C3-variant-0"][0]
    M_rna = np.asarray(u0["M_struc"]) - np.asarray(u0["M_struc_bare"])
    C_rest = np.asarray(u0["C_struc"]) - np.asarray(u0["C_struc_bare"])             # no mooring constant: C_moor per candidate
    rng = np.random.default_rng(2)
    draw = lambda: G.volturnus_params(rng.uniform(0.75, 1.25, size=(n, 5)))
    rep = lambda a: np.repeat(a[None], n, axis=0)
    w = np.asarray(c3["w"])
    sweep = VariantSweep(G.volturnus_program(base), draw(), rep(M_rna), np.zeros((n, 6, 6)), rep(C_rest), w, wave_numbers(w, depth),
                         depth, np.asarray(c3["zeta"])[None], np.asarray(c3["beta"])[None], int(c3["nIter"]), float(c3["XiStart"]))
    ctx = backend.default_context(0)
    MOOR = dict(program=mooring_program(rows))
    for s_ in range(2):                                                  # warm-up: code objects, buffers, the chip's clock
        sweep.wait_crossing(ctx, sweep.submit_crossing(ctx, s_, mooring=MOOR))
        sweep.set_params(draw())
    ends = tension_names(len(rows))
    best = (np.inf, None, None, None)
    flagged = 0
    t0 = time.perf_counter()
    cur = (sweep.submit_crossing(ctx, 0, mooring=MOOR), sweep.params)
    for b in range(n_batches):
        nxt = None
        if b + 1 < n_batches:
            sweep.set_params(draw())
            nxt = (sweep.submit_crossing(ctx, (b + 1) % 2, mooring=MOOR), sweep.params)
        h, params = cur
        out = sweep.wait_crossing(ctx, h)
        good = (out["flags"][:, 0] & 1).astype(bool) & (out["moor_flags"] == 0)   # converged, and every line solved
        flagged += int(np.count_nonzero(out["moor_flags"]))
        pitch = np.where(good, out["std"][:, 0, 4], np.inf)
        t3 = out["T_mean"] + 3.0 * out["T_std"][:, 0, :]                   # mean + 3 sigma of both ends of every segment
        i = int(np.argmin(pitch))
        if pitch[i] < best[0]:
            j = int(np.argmax(t3[i]))
            best = (float(pitch[i]), params[i].copy(), float(t3[i, j]), "%s of %s" % (ends[j], row_names[j % len(rows)]))
        cur = nxt
    dt = time.perf_counter() - t0
    print("%d batches x %d candidates on chain - rope - chain lines (%d rows) in %.1f ms: %.2f ms per batch; %d candidates flagged"
          % (n_batches, n, len(rows), 1e3 * dt, 1e3 * dt / n_batches, flagged))
    print("smallest pitch std %.3f deg for (ccD, ocD, T, ocR, pH) = %s; worst segment-end tension mean + 3 sigma %.3g N at %s"
          % (best[0], np.round(best[1], 2), best[2], best[3]))


if __name__ == "__main__":
    main()
