"""The cases of tests/test_mean_pose.py (fp64 model, CPU) and tests/test_hip_mean_pose.py (kernel, GPU): the four
single-unit quasi-static decks -- hydrostatics of tests/golden/refgold_statics.npz, lines of refgold_mooring.npz, the
recorded current load of refgold_current.npz -- unloaded, under the scaled current load and under a thrust-like load;
single lines of tests/mooring_cases.py under a synthetic diagonally dominant K_hs; a non-zero x_ref (all six components) with the
anchors shifted by its horizontal part; and a four-line layout.  ``reference(name)`` solves a case once per process with tests/mean_pose_reference.py.
"""
import functools
import os

import numpy as np

from raft_amd import snapshot as standin

from . import mean_pose_reference as mpr
from . import mooring_cases as mc
from . import mooring_reference as mr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refgold_mean_pose.npz")
SINGLE = ("contact", "anchor_off_seabed", "nearly_taut")
THRUST = 1.0e6            # N, at 30 deg, applied 100 m above the reference point (a rotor's thrust)
THRUST_ARM = 100.0


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def decks():
    """deck -> dict(lines, depth, K_hs, F0, D_current, records): the order of the statics / current fixtures is golden()['decks']."""
    g = golden()
    stat = standin.load_fixture("refgold_statics.npz")["cases"]
    cur = standin.load_fixture("refgold_current.npz")["pickle"]
    moor = mc.golden()
    scale = (float(g["current_speed"]) / float(g["pickle_speed"])) ** 2
    out = {}
    for i, deck in enumerate(str(d) for d in g["decks"]):
        s = stat[i]
        out[deck] = dict(lines=moor[deck]["lines"], depth=moor[deck]["depth"],
                         K_hs=np.asarray(s["true_C_struc"]) + np.asarray(s["true_C_hydro"]),
                         F0=np.asarray(s["true_W_struc"]) + np.asarray(s["true_W_hydro"]),
                         D_current=scale * np.asarray(cur[i]["D"]),
                         records={"wave": g[deck + "/wave"], "current": g[deck + "/current"]})
    return out


def thrust_load():
    c, s = np.cos(np.deg2rad(30.0)), np.sin(np.deg2rad(30.0))
    return np.array([THRUST * c, THRUST * s, 0.0, -THRUST_ARM * THRUST * s, THRUST_ARM * THRUST * c, 0.0])


def _case(lines, depth, K_hs, F0, F_env=None, x_ref=None):
    return dict(lines=np.ascontiguousarray(lines, dtype=float), depth=float(depth), K_hs=np.ascontiguousarray(K_hs, dtype=float),
                F0=np.ascontiguousarray(F0, dtype=float), F_env=np.zeros(6) if F_env is None else np.ascontiguousarray(F_env, dtype=float),
                x_ref=np.zeros(6) if x_ref is None else np.ascontiguousarray(x_ref, dtype=float))


def synthetic_K():
    """Diagonally dominant, not symmetric."""
    K = np.diag([2.0e5, 2.5e5, 4.0e5, 3.0e8, 3.5e8, 2.0e8])
    K[0, 4], K[4, 0], K[1, 3], K[3, 1], K[2, 4] = -4.0e5, -3.0e5, 5.0e5, 4.0e5, 1.0e5
    return K


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case (one design each): dict lines [nL,16], depth, K_hs, F0, F_env, x_ref."""
    out = {}
    for deck, d in decks().items():
        out[deck + "/unloaded"] = _case(d["lines"], d["depth"], d["K_hs"], d["F0"])
        out[deck + "/current"] = _case(d["lines"], d["depth"], d["K_hs"], d["F0"], d["D_current"])
        out[deck + "/thrust"] = _case(d["lines"], d["depth"], d["K_hs"], d["F0"], thrust_load())
    single = mc.single_lines()
    for name in SINGLE:
        rec, depth = single[name]
        # F0 takes 90 % of the line's load at the zero pose: the unit settles a short way towards the anchor
        F_at_0 = mr.evaluate(rec[None, None], None, depth)["F"][0].astype(np.float64)
        out["single/" + name] = _case(rec[None], depth, synthetic_K(), -0.9 * F_at_0)
    d = decks()["VolturnUS-S"]
    x_ref = np.array([40.0, -25.0, -0.3, 0.005, -0.01, 0.02])
    lines = d["lines"].copy()
    lines[:, 0:2] += x_ref[:2]                                  # (horizontally: the anchors stay on the seabed)
    out["x_ref"] = _case(lines, d["depth"], d["K_hs"], d["F0"], thrust_load(), x_ref)
    # four lines: the deck's three and its first one once more, turned by 90 degrees about the vertical
    turn = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    extra = d["lines"][0].copy()
    extra[0:3], extra[3:6] = turn @ extra[0:3], turn @ extra[3:6]
    out["four_lines"] = _case(np.concatenate([d["lines"], extra[None]]), d["depth"], d["K_hs"], d["F0"], thrust_load())
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The longdouble solution of a case (computed once, never modified)."""
    c = cases()[name]
    return mpr.solve(c["lines"], c["depth"], c["K_hs"], c["F0"], c["F_env"], c["x_ref"])


def batch(names):
    """The cases ``names`` stacked as one batch (equal line counts): dict lines [nD,nL,16], K_hs, F0, F_env, x_ref, depth."""
    cs = [cases()[n] for n in names]
    assert len({c["depth"] for c in cs}) == 1 and len({len(c["lines"]) for c in cs}) == 1
    out = {k: np.ascontiguousarray([c[k] for c in cs]) for k in ("lines", "K_hs", "F0", "F_env", "x_ref")}
    out["depth"] = cs[0]["depth"]
    return out
