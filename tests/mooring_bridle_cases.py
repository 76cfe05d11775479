"""The fixed case list of the bridle tests (tests/test_mooring_bridles.py on the CPU, tests/test_hip_mooring_bridles.py on the
device): rows [nRow,16] in the format of include/raftx_mooring.h, a depth, and the poses every case is evaluated at -- zero,
and an offset with about 10 degrees of yaw, at which one leg of a bridle is much slacker than the other.
"""
import numpy as np

ML_N, ML_WJOINT, ML_LEG, ML_CONT = 16, 10, 14, 15
CHAIN = (7.5e8, 1500.0)          # EA [N], w [N/m]
ROPE = (2.0e8, 120.0)
POSES = (np.zeros(6), np.array([9.0, -6.0, 0.8, 0.02, -0.03, 0.17]))


def single(anchor, fairlead, L, EA, w):
    r = np.zeros((1, ML_N))
    r[0, 0:3], r[0, 3:6], r[0, 6:9] = anchor, fairlead, (L, EA, w)
    return r


def chain(anchor, fairlead, segs):
    """segs: (L, EA, w, weight of the point at the lower end), anchor side first."""
    r = np.zeros((len(segs), ML_N))
    r[0, 0:3], r[0, 3:6] = anchor, fairlead
    for i, (L, EA, w, Wj) in enumerate(segs):
        r[i, 6:9] = (L, EA, w)
        if i:
            r[i, ML_WJOINT], r[i, ML_CONT] = Wj, 1.0
    return r


def bridle(anchor, stem, legs, Wj=0.0):
    """stem: segments as in ``chain``; legs: (fairlead, L, EA, w); Wj: the junction's net submerged weight."""
    r = np.zeros((len(stem) + len(legs), ML_N))
    r[:len(stem)] = chain(anchor, (0.0, 0.0, 0.0), stem)
    for i, (f, L, EA, w) in enumerate(legs):
        k = len(stem) + i
        r[k, 3:6], r[k, 6:9], r[k, ML_LEG] = f, (L, EA, w), 1.0
    r[len(stem), ML_WJOINT] = Wj
    return r


def turned(rows, deg):
    """The rows with anchors and fairleads turned about the z axis."""
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    out = np.array(rows, dtype=float)
    for r in out:
        r[0:3], r[3:6] = R @ r[0:3], R @ r[3:6]
    return out


A200 = (-850.0, 0.0, -200.0)
FL, FR = (-40.0, 30.0, -14.0), (-40.0, -30.0, -14.0)
A600 = (-1600.0, 0.0, -600.0)

# name -> (rows, depth, number of stem rows of the bridle at row 0)
ACCURACY = {
    "symmetric_200": (bridle(A200, [(745.0,) + CHAIN + (0.0,)], [(FL, 110.0) + CHAIN, (FR, 110.0) + CHAIN]), 200.0),
    "unequal_legs": (bridle(A200, [(745.0,) + CHAIN + (0.0,)], [(FL, 125.0) + CHAIN, (FR, 105.0, 3.0e8, 900.0)]), 200.0),
    "clump": (bridle(A200, [(745.0,) + CHAIN + (0.0,)], [(FL, 110.0) + CHAIN, (FR, 110.0) + CHAIN], Wj=2.0e5), 200.0),
    "buoy": (bridle(A200, [(745.0,) + CHAIN + (0.0,)], [(FL, 110.0) + CHAIN, (FR, 110.0) + CHAIN], Wj=-1.5e5), 200.0),
    "chain_rope_600": (bridle(A600, [(500.0,) + CHAIN + (0.0,), (1080.0,) + ROPE + (0.0,)],
                              [(FL, 150.0) + ROPE, (FR, 150.0) + ROPE]), 600.0),
    "three_legs": (bridle(A200, [(745.0,) + CHAIN + (0.0,)],
                          [(FL, 112.0) + CHAIN, ((-45.0, 0.0, -16.0), 108.0) + CHAIN, (FR, 112.0) + CHAIN]), 200.0),
    "stem_on_seabed": (bridle((-900.0, 0.0, -200.0), [(800.0,) + CHAIN + (0.0,)], [(FL, 100.0) + CHAIN, (FR, 100.0) + CHAIN]), 200.0),
}


def accuracy_batch():
    """(lines [nD,nRow,16] per depth group, poses) -- every accuracy case at both poses, grouped by (depth, rows)."""
    groups = {}
    for name, (rows, depth) in ACCURACY.items():
        for ip, pose in enumerate(POSES):
            groups.setdefault((depth, len(rows)), []).append((name, ip, rows, pose))
    return groups


def mixed_design():
    """Bridle + chain + single line in one design of 6 rows (depth 200): the three kinds of line in one batch."""
    b = ACCURACY["symmetric_200"][0]
    c = turned(chain(A200, (-40.0, 0.0, -14.0), [(500.0,) + CHAIN + (0.0,), (340.0,) + ROPE + (3.0e4,)]), 120.0)
    s = turned(single(A200, (-40.0, 0.0, -14.0), 850.0, *CHAIN), 240.0)
    return np.vstack([b, c, s]), 200.0


def bridle_two_singles():
    """A bridle and two single lines at 120 and 240 degrees (depth 200), 5 rows: a moored unit."""
    b = ACCURACY["symmetric_200"][0]
    s1 = turned(single(A200, (-40.0, 0.0, -14.0), 850.0, *CHAIN), 120.0)
    s2 = turned(single(A200, (-40.0, 0.0, -14.0), 850.0, *CHAIN), 240.0)
    return np.vstack([b, s1, s2]), 200.0


def deck_bridles(lines, stem=760.0, leg=95.0, spread=20.0):
    """The single lines [nLine,16] of a deck, each turned into a bridle of 3 rows: a stem of the line's EA and w, and two legs
    of the same to fairleads turned +-spread degrees about the z axis from the line's own."""
    out = []
    for r in np.asarray(lines, dtype=float):
        legs = []
        for sg in (+1.0, -1.0):
            c, s = np.cos(np.radians(sg * spread)), np.sin(np.radians(sg * spread))
            legs.append(((c * r[3] - s * r[4], s * r[3] + c * r[4], r[5]), leg, r[7], r[8]))
        out.append(bridle(r[0:3], [(stem, r[7], r[8], 0.0)], legs))
    return np.vstack(out)


def coincident_legs():
    """Identity 1: two legs to one fairlead, each EA/2 and w/2 -- and the composite line whose last segment has EA and w."""
    f = (-40.0, 12.0, -14.0)
    two = bridle(A200, [(745.0,) + CHAIN + (0.0,)], [(f, 110.0, CHAIN[0] / 2, CHAIN[1] / 2), (f, 110.0, CHAIN[0] / 2, CHAIN[1] / 2)], Wj=5.0e4)
    one = chain(A200, f, [(745.0,) + CHAIN + (0.0,), (110.0,) + CHAIN + (5.0e4,)])
    return two, one, 200.0


MIRROR_POSE = np.array([7.0, 0.0, -0.5, 0.0, 0.04, 0.0])      # in the x-z plane: surge, heave, pitch

# name -> (rows, depth, pose, flag): firm decisions, the same in fp64 and longdouble
_S = ACCURACY["symmetric_200"][0]


def _with(rows, r, k, v):
    out = np.array(rows)
    out[r, k] = v
    return out


FLAGS = {
    "nan_leg_length": (_with(_S, 2, 6, np.nan), 200.0, POSES[0], 1),
    "negative_leg_weight": (_with(_S, 1, 8, -10.0), 200.0, POSES[0], 1),
    "zero_stem_EA": (_with(_S, 0, 7, 0.0), 200.0, POSES[0], 1),
    "slack_every_leg": (bridle(A200, [(900.0,) + CHAIN + (0.0,)], [(FL, 110.0) + CHAIN, (FR, 110.0) + CHAIN]), 200.0, POSES[0], 4),
    # a suspended anchor in shallow water and a 4 MN clump: the junction hangs at z = -27, two metres below the seabed
    "grounded_junction": (bridle((-300.0, 0.0, -20.0), [(200.0,) + CHAIN + (0.0,)], [(FL, 64.0) + CHAIN, (FR, 64.0) + CHAIN], Wj=4.0e6),
                          25.0, POSES[0], 64),
}
