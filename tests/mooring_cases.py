"""The mooring cases of tests/test_mooring.py (fp64 model, CPU) and tests/test_hip_mooring.py (kernels, GPU): line
records and poses covering both catenary branches and their boundary, taut and sagging lines, soft and stiff lines, two
depths and rotated poses, besides the decks of tests/golden/refgold_mooring.npz.  ``reference()`` evaluates
tests/mooring_reference.py on them once per process.
"""
import functools
import json
import os

import numpy as np

from . import mooring_reference as mr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refgold_mooring.npz")
DECKS = ("VolturnUS-S", "VolturnUS-S-pointInertia", "OC3spar", "OC4semi-WAMIT_Coefs")
POSES = np.array([[0, 0, 0, 0, 0, 0],
                  [3.0, -2.0, -0.5, 0, 0, np.deg2rad(30.0)],
                  [-4.0, 1.5, 0.3, np.deg2rad(5.0), np.deg2rad(-5.0), 0],
                  [2.0, 2.0, -0.2, np.deg2rad(-5.0), np.deg2rad(5.0), np.deg2rad(30.0)]], dtype=float)


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    out = {}
    for deck in DECKS:
        out[deck] = dict(design=json.loads(str(z[deck + "/design"])), lines=z[deck + "/lines"], depth=float(z[deck + "/depth"]),
                         rho=float(z[deck + "/rho"]), g=float(z[deck + "/g"]), poses=z[deck + "/poses"], Tmoor_avg=z[deck + "/Tmoor_avg"])
    return out


def record(anchor, fairlead, L, EA, w):
    r = np.zeros(16)
    r[0:3], r[3:6], r[6], r[7], r[8] = anchor, fairlead, L, EA, w
    return r


def _boundary_line(delta, depth=50.0):
    """A line whose solution has VF = w L (1 + delta): the span is computed from the catenary equations in longdouble
    for HF = 1e6 N, w = 1000 N/m, L = 200 m, EA = 1e9 N, so that both branches are met within 1e-9 of their boundary."""
    T = np.longdouble
    H, w, L, EA = T(1e6), T(1000.0), T(200.0), T(1e9)
    V = w * L * (1 + T(delta))
    X, Z = mr.catenary(H, V, L, EA, w, True)[:2]
    return record([-float(X), 0.0, -depth], [0.0, 0.0, float(Z) - depth], float(L), float(EA), float(w))


def single_lines():
    """name -> (record, depth): one line each."""
    c = {}
    c["no_contact"] = (record([-700.0, 0, -200.0], [-40.0, 0, -14.0], 700.0, 3.27e9, 6000.0), 200.0)
    c["contact"] = (record([-837.0, 0, -200.0], [-58.0, 0, -14.0], 850.0, 3.27e9, 6000.0), 200.0)
    c["boundary_above"] = (_boundary_line(+1e-9), 50.0)
    c["boundary_below"] = (_boundary_line(-1e-9), 50.0)
    chord = float(np.hypot(600.0, 186.0))
    c["nearly_taut"] = (record([-640.0, 0, -200.0], [-40.0, 0, -14.0], 1.0001 * chord, 3.27e9, 6000.0), 200.0)
    c["anchor_off_seabed"] = (record([-320.0, 0, -100.0], [-20.0, 0, -90.0], 305.0, 5.0e8, 1500.0), 200.0)
    c["EA_1e6"] = (record([-300.0, 50.0, -50.0], [-10.0, 5.0, -8.0], 280.0, 1.0e6, 300.0), 50.0)
    c["EA_1e10"] = (record([-837.0, 0, -200.0], [-58.0, 0, -14.0], 850.0, 1.0e10, 6000.0), 200.0)
    c["depth_50"] = (record([200.0, -150.0, -50.0], [10.0, -8.0, -6.0], 245.0, 8.0e8, 1200.0), 50.0)
    c["depth_320"] = (record([853.87, 0, -320.0], [5.2, 0, -70.0], 902.2, 384.243e6, 698.094), 320.0)
    return c


def batches():
    """List of (name, lines [nD,nL,16], pose [nD,6], depth): every single line at every pose of POSES (the boundary
    lines at the zero pose only: a displaced fairlead moves them off the boundary), every line of the decks on its own,
    and the three-line decks at their recorded poses and at POSES."""
    out = []
    for name, (rec, depth) in single_lines().items():
        poses = POSES[:1] if name.startswith("boundary") else POSES
        out.append((name, np.broadcast_to(rec, (len(poses), 1, 16)).copy(), poses.copy(), depth))
    for deck, g in golden().items():
        poses = np.concatenate([g["poses"], POSES])
        out.append((deck, np.broadcast_to(g["lines"], (len(poses),) + g["lines"].shape).copy(), poses, g["depth"]))
        out.append((deck + "/one-line", g["lines"][:, None, :].copy(), np.broadcast_to(POSES[1], (len(g["lines"]), 6)).copy(), g["depth"]))
    return out


@functools.lru_cache(maxsize=None)
def reference():
    """name -> the longdouble reference of every batch (computed once, never modified)."""
    return {name: mr.evaluate(lines, pose, depth) for name, lines, pose, depth in batches()}


def worst_multiples(res, ref):
    """Worst gate multiple per quantity of a result dict against a reference dict."""
    return {k: float(np.max(mr.gate_multiples(res[k], ref[k], ref["E" + k]))) for k in ("C", "F", "T", "J")}
