"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/refgold_mean_pose.npz from the reference's test DATA (no reference code
is imported or run: tests/test_model.py is parsed, and only two literal tables of it are evaluated).  Run in the build
container only:

    python scripts/make_mean_pose_golden.py

Never imported by the tests; they read the committed .npz, which holds numbers only:

  decks                      the four single-unit quasi-static decks, in the order of refgold_statics.npz / refgold_current.npz
  <deck>/wave, <deck>/current  the recorded mean pose desired_X0 [6] of Model.solveStatics (tests/test_model.py:82-123)
  current_speed, current_heading   of the 'current' case (m/s, deg); the 'wave' case has no mean load
  pickle_speed               the speed of the recorded current loads of refgold_current.npz ("pickle"): the load of the
                             'current' case is that record times (current_speed / pickle_speed)^2
  tol                        the reference's stopping tolerances (raft_model.py:664): 0.05 m, 0.005 rad
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle.stage_reference import REFERENCE_ROOT        # noqa: E402  (RAFT_REFERENCE_ROOT; only the path is used)

SOURCE = os.path.join(REFERENCE_ROOT, "tests", "test_model.py")
OUT = os.path.join(ROOT, "tests", "golden", "refgold_mean_pose.npz")
DECKS = ("OC3spar", "VolturnUS-S", "VolturnUS-S-pointInertia", "OC4semi-WAMIT_Coefs")
CASES = ("wave", "current")


def literal(tree, name):
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in node.targets):
            return eval(compile(ast.Expression(node.value), SOURCE, "eval"), {"np": np, "__builtins__": {}})
    raise KeyError(name)


def main():
    with open(SOURCE) as f:
        tree = ast.parse(f.read())
    files = [os.path.splitext(n)[0] for n in literal(tree, "list_files")]
    X0, cases = literal(tree, "desired_X0"), literal(tree, "cases4solveStatics")
    assert cases["wave"]["current_speed"] == 0 and cases["wave"]["wind_speed"] == 0 and cases["current"]["wind_speed"] == 0
    out = {"decks": np.array(DECKS), "current_speed": float(cases["current"]["current_speed"]),
           "current_heading": float(cases["current"]["current_heading"]), "pickle_speed": 2.0, "tol": np.array([0.05, 0.005])}
    for deck in DECKS:
        for case in CASES:
            x = np.asarray(X0[case][files.index(deck)], dtype=float)
            assert x.shape == (6,)
            out["%s/%s" % (deck, case)] = x
            print("%-26s %-8s %s" % (deck, case, np.array2string(x, precision=6)))
    np.savez(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
