"""The cases of tests/test_array_mooring.py (fp64 model, CPU) and tests/test_hip_array_mooring.py (kernels, GPU): arrays of
VolturnUS-S units -- K_hs, F0 and the three chains of ``mean_pose_cases.decks()``, 200 m of water -- joined by shared lines.
``reference(name)`` solves a case once per process with tests/array_mooring_reference.py (plain Newton: every case passes it
unflagged, except ``pair_grounded``, which is there for its flag).

    pair              two units at (0, 0) and (1600, 0), unit 1's records turned by 180 degrees; one shared row from (58, 0, -14) on
                      unit 0 to (-58, 0, -14) on unit 1, L = 1490 m, EA = 2e8 N, w = 300 N/m.  ZF is exactly 0 at the first iterate.
    pair_grounded     the same pair with L = 1500 m and the chains' own EA and w: the sag passes the seabed mid-iteration
    pair_thrust       pair under the thrust-like load of mean_pose_cases on unit 0 only
    pair_yaw_pitch    pair from a start pose with yaw and pitch on both units
    pair_shared_first pair with the shared row first in row order (pair itself has it last)
    row3              three units in a row, two shared rows
    square4           four units on a square, four shared rows (24 DOFs)
    ring6             six units on a hexagon, six shared rows (36 DOFs)
    rows66            ring6 with ten anchored lines per unit: 66 rows, more rows than lanes
    single_unit       nUnit = 1 with the deck's lines
"""
import functools

import numpy as np

from raft_amd import mooring

from . import array_mooring_reference as ar
from . import mean_pose_cases as mpc

DEPTH = 200.0
SPACING = 1600.0
R_FAIR, Z_FAIR = 58.0, -14.0
SHARED = dict(L=1490.0, EA=2.0e8, w=300.0)
NAMES = ("pair", "pair_thrust", "pair_yaw_pitch", "pair_shared_first", "row3", "square4", "ring6", "rows66", "single_unit")


def _deck():
    return mpc.decks()["VolturnUS-S"]


def _shared(ua, ub, loc, **kw):
    """A shared row between the fairlead radius of unit ua and of unit ub, each attachment on the side of the other unit."""
    d = np.asarray(loc[ub], dtype=float) - np.asarray(loc[ua], dtype=float)
    d = d / np.hypot(*d)
    d = np.where(np.abs(d) < 1e-15, 0.0, d)
    p = dict(SHARED, **kw)
    return dict(unitA=ua, rA=(R_FAIR * d[0], R_FAIR * d[1], Z_FAIR), unitB=ub, rB=(-R_FAIR * d[0], -R_FAIR * d[1], Z_FAIR), **p)


def _turned(lines, deg):
    return mooring.array_lines([lines], [(0.0, 0.0)], [deg])[:, :11].copy()


def _ten_lines():
    """Ten anchored lines of one unit: the deck's three turned by 0, 30 and 60 degrees, and its first one turned by 15."""
    d = _deck()["lines"]
    out = [d, _turned(d, 30.0), _turned(d, 60.0), _turned(d[:1], 15.0)]
    return np.concatenate([np.pad(a, ((0, 0), (0, 16 - a.shape[1]))) for a in out])


def _case(unit_lines, loc, headings, shared, F_env=None, x_ref=None, shared_first=False):
    d = _deck()
    nU = len(loc)
    lines = mooring.array_lines(unit_lines, loc, headings, shared)
    if shared_first:
        k = len(shared)
        lines = np.ascontiguousarray(np.concatenate([lines[-k:], lines[:-k]]))
    xr = np.zeros((nU, 6))
    xr[:, :2] = loc
    if x_ref is not None:
        xr = xr + np.asarray(x_ref, dtype=float)
    return dict(lines=lines, depth=DEPTH, K_hs=np.ascontiguousarray(np.broadcast_to(d["K_hs"], (nU, 6, 6))),
                F0=np.ascontiguousarray(np.broadcast_to(d["F0"], (nU, 6))),
                F_env=np.zeros((nU, 6)) if F_env is None else np.ascontiguousarray(F_env, dtype=float), x_ref=np.ascontiguousarray(xr))


def _ring(n):
    """Locations of n units on a regular polygon of side SPACING, and headings that turn each unit's records with its place."""
    rad = SPACING / (2.0 * np.sin(np.pi / n))
    ang = 2.0 * np.pi * np.arange(n) / n
    loc = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    return np.round(loc, 6), list(np.degrees(ang))


@functools.lru_cache(maxsize=None)
def cases():
    d = _deck()["lines"]
    pair_loc = [(0.0, 0.0), (SPACING, 0.0)]
    sh = [_shared(0, 1, pair_loc)]
    out = {}
    out["pair"] = _case([d, d], pair_loc, [0.0, 180.0], sh)
    out["pair_grounded"] = _case([d, d], pair_loc, [0.0, 180.0], [_shared(0, 1, pair_loc, L=1500.0, EA=float(d[0, 7]), w=float(d[0, 8]))])
    thrust = np.zeros((2, 6))
    thrust[0] = mpc.thrust_load()
    out["pair_thrust"] = _case([d, d], pair_loc, [0.0, 180.0], sh, F_env=thrust)
    out["pair_yaw_pitch"] = _case([d, d], pair_loc, [0.0, 180.0], sh, x_ref=[[0, 0, 0, 0, 0.02, 0.05], [0, 0, 0, 0, -0.015, -0.04]])
    out["pair_shared_first"] = _case([d, d], pair_loc, [0.0, 180.0], sh, shared_first=True)
    loc3 = [(0.0, 0.0), (SPACING, 0.0), (2 * SPACING, 0.0)]
    out["row3"] = _case([d, d, d], loc3, [0.0, 90.0, 180.0], [_shared(0, 1, loc3), _shared(1, 2, loc3)])
    loc4, head4 = _ring(4)
    out["square4"] = _case([d] * 4, loc4, head4, [_shared(i, (i + 1) % 4, loc4) for i in range(4)])
    loc6, head6 = _ring(6)
    sh6 = [_shared(i, (i + 1) % 6, loc6) for i in range(6)]
    out["ring6"] = _case([d] * 6, loc6, head6, sh6)
    out["rows66"] = _case([_ten_lines()] * 6, loc6, head6, sh6)
    out["single_unit"] = _case([d], [(0.0, 0.0)], [0.0], [])
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The longdouble solution of a case (computed once, never modified)."""
    c = cases()[name]
    return ar.solve(c["lines"], c["depth"], c["K_hs"], c["F0"], c["F_env"], c["x_ref"])


def batch(names):
    """The cases ``names`` stacked as one batch (equal unit and row counts)."""
    cs = [cases()[n] for n in names]
    assert len({c["lines"].shape for c in cs}) == 1 and len({c["K_hs"].shape for c in cs}) == 1
    out = {k: np.ascontiguousarray([c[k] for c in cs]) for k in ("lines", "K_hs", "F0", "F_env", "x_ref")}
    out["depth"] = DEPTH
    return out
