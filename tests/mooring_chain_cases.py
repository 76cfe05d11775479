"""The composite-line cases of tests/test_mooring_chains.py (fp64 model, CPU) and tests/test_hip_mooring_chains.py (kernels,
GPU): rows [nDesign,nRow,16] and poses at the numbers of real decks -- the VolturnUS-S lines of
tests/golden/refgold_mooring.npz in 200 m of water, and chain - rope - chain lines in 600 m (studless chain of 6 kN/m and
EA 3.27e9 N as the deck's; a polyester rope of 300 N/m and EA 5e8 N).  ``reference()`` evaluates
tests/mooring_chain_reference.py on the accuracy cases once per process.
"""
import functools

import numpy as np

from . import mooring_cases as mc
from . import mooring_chain_reference as cr

POSES = mc.POSES
DEEP = 600.0
CHAIN = (3.27e9, 6000.0)       # EA [N], w [N/m]
ROPE = (5.0e8, 300.0)
# The VolturnUS-S lines rest on the seabed over 437 .. 531 m of their 850 m at POSES, and only the anchor-side row may rest:
# the cuts leave it 70 % of the length.  ("Equal properties": every row has the line's EA and w.)
SPLITS = {2: (0.7, 0.3), 3: (0.7, 0.15, 0.15)}


def head(anchor, fairlead, L, EA, w):
    return mc.record(anchor, fairlead, L, EA, w)


def cont(L, EA, w, Wj=0.0):
    r = np.zeros(16)
    r[6], r[7], r[8], r[cr.ML_WJOINT], r[cr.ML_CONT] = L, EA, w, Wj, 1.0
    return r


def split(rec, fractions):
    """A single-line record cut into rows of its own EA and w with weightless joints."""
    L, EA, w = rec[6], rec[7], rec[8]
    rows = [head(rec[0:3], rec[3:6], fractions[0] * L, EA, w)] + [cont(f * L, EA, w) for f in fractions[1:]]
    return np.array(rows)


def _ends(heading_deg, z_anchor=-DEEP, radius=1600.0):
    c, s = np.cos(np.deg2rad(heading_deg)), np.sin(np.deg2rad(heading_deg))
    return [radius * c, radius * s, z_anchor], [58.0 * c, 58.0 * s, -14.0]


def crc(heading_deg=180.0, L=(600.0, 1000.0, 100.0), W1=0.0, W2=0.0, z_anchor=-DEEP, radius=1600.0):
    """Chain - rope - chain from an anchor at `radius` to the column at 58 m; W1 / W2: the lower / upper joint's weight."""
    a, f = _ends(heading_deg, z_anchor, radius)
    return np.array([head(a, f, L[0], *CHAIN), cont(L[1], *ROPE, W1), cont(L[2], *CHAIN, W2)])


def single(heading_deg):
    a, f = _ends(heading_deg)
    return head(a, f, 1720.0, 1.2e9, 1500.0)[None]


def chain_rope(heading_deg):
    a, f = _ends(heading_deg)
    return np.array([head(a, f, 700.0, *CHAIN), cont(1000.0, *ROPE, 5.0e4)])


def _surge(xs):
    p = np.zeros((len(xs), 6))
    p[:, 0] = xs
    return p


def split_batches():
    """(name, rows, pose, depth, single-line records): the split identity."""
    g = mc.golden()["VolturnUS-S"]
    out = []
    for k, fr in SPLITS.items():
        rows = np.concatenate([split(rec, fr) for rec in g["lines"]])
        out.append(("split-%d" % k, np.broadcast_to(rows, (len(POSES),) + rows.shape).copy(), POSES.copy(), g["depth"], g["lines"]))
    return out


def batches():
    """List of (name, rows [nD,nRow,16], pose [nD,6], depth): the accuracy cases.  Every one must solve with flag 0."""
    out = [b[:4] for b in split_batches()]
    # chain - rope - chain, the anchor-side chain partly resting; surged away from the anchor until it lifts off
    xs = [0.0, 40.0, 60.0, 70.0, 80.0, 120.0]
    out.append(("chain-rope-chain", np.broadcast_to(crc(), (len(xs), 3, 16)).copy(), _surge(xs), DEEP))
    out.append(("chain-rope-chain/poses", np.broadcast_to(crc(150.0), (len(POSES), 3, 16)).copy(), POSES.copy(), DEEP))
    out.append(("clump", np.broadcast_to(crc(W1=3.0e5), (2, 3, 16)).copy(), _surge([0.0, 60.0]), DEEP))
    # a buoy at the upper joint that lifts more than hangs below it: the top chain leaves it downwards (V_bottom < 0)
    out.append(("clump+buoy", np.broadcast_to(crc(L=(600.0, 1000.0, 150.0), W1=2.0e5, W2=-1.2e6), (2, 3, 16)).copy(), _surge([0.0, -60.0]), DEEP))
    out.append(("anchor-off-the-bed", np.broadcast_to(crc(L=(500.0, 1000.0, 100.0), z_anchor=-400.0, radius=1500.0), (len(POSES), 3, 16)).copy(),
                POSES.copy(), DEEP))
    # row order
    mixed = np.concatenate([single(180.0), crc(60.0, W1=1.0e5), single(-60.0)])
    out.append(("single+chain3+single", np.broadcast_to(mixed, (len(POSES),) + mixed.shape).copy(), POSES.copy(), DEEP))
    pairs = np.concatenate([chain_rope(h) for h in (180.0, 60.0, -60.0)])
    out.append(("3xchain2", np.broadcast_to(pairs, (len(POSES),) + pairs.shape).copy(), POSES.copy(), DEEP))
    return out


def flag_cases():
    """List of (name, rows [3,3,16] -- the flagged design between two healthy ones --, depth, the middle design's flag)."""
    good_a, good_b = crc(), crc(W1=3.0e5)
    bad_w = crc()
    bad_w[1, 8] = 0.0
    cases = [("grounded: the anchor-side chain rests wholly", crc(L=(200.0, 1500.0, 100.0)), cr.FLAG_GROUNDED),
             ("grounded: the sag below the seabed", crc(L=(500.0, 1000.0, 100.0), z_anchor=-550.0, radius=1500.0), cr.FLAG_GROUNDED),
             ("bad line: w = 0 in a continuation row", bad_w, cr.FLAG_BAD_LINE),
             ("slack on the total length", crc(L=(600.0, 1500.0, 100.0)), cr.FLAG_SLACK)]
    return [(name, np.array([good_a, rows, good_b]), DEEP, flag) for name, rows, flag in cases]


@functools.lru_cache(maxsize=None)
def reference():
    """name -> the longdouble reference of every accuracy batch (computed once, never modified)."""
    return {name: cr.evaluate(lines, pose, depth) for name, lines, pose, depth in batches()}


@functools.lru_cache(maxsize=None)
def split_reference():
    """name -> the single-line reference (tests/mooring_reference.py) of the uncut lines at the same poses."""
    return {name: mc.mr.evaluate(np.broadcast_to(recs, (len(pose),) + recs.shape).copy(), pose, depth)
            for name, _, pose, depth, recs in split_batches()}


def worst_multiples(res, ref):
    return {k: float(np.max(cr.gate_multiples(res[k], ref[k], ref["E" + k]))) for k in ("C", "F", "T", "J")}
