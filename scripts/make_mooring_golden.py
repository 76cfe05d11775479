"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/refgold_mooring.npz from the reference's test DATA (no reference code
is imported or run).  Run in the build container only:

    python scripts/make_mooring_golden.py

Never imported by the tests; they read the committed .npz, which holds, per deck of DECKS:

  <deck>/design     the deck YAML's ``mooring`` and ``site`` sections as a JSON string (settings only),
  <deck>/lines      the line records raft_amd.mooring.lines_from_design makes of them, <deck>/depth, /rho, /g,
  <deck>/poses      [nCase,6] the recorded mean motions of every case of <deck>_true_analyzeCases.pkl (surge, sway,
                    heave in m; roll, pitch, yaw converted from the stored degrees to radians),
  <deck>/Tmoor_avg  [nCase,2 nLine] the recorded mean tensions (ends A, then ends B).

The farm decks (shared lines, MoorDyn files) are left out.  The script prints the worst relative difference between
tests/mooring_reference.py at the recorded poses and the recorded Tmoor_avg per deck: the figure recorded beside the
tolerance of tests/test_mooring.py.
"""
import json
import os
import pickle
import sys

import numpy as np
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle.stage_reference import REFERENCE_ROOT        # noqa: E402  (RAFT_REFERENCE_ROOT; only the path is used)
from raft_amd.mooring import lines_from_design          # noqa: E402
from tests import mooring_reference as mr                # noqa: E402

REFERENCE_DATA = os.path.join(REFERENCE_ROOT, "tests", "test_data")
OUT = os.path.join(ROOT, "tests", "golden", "refgold_mooring.npz")
DECKS = ("VolturnUS-S", "VolturnUS-S-pointInertia", "OC3spar", "OC4semi-WAMIT_Coefs")
DOF = ("surge", "sway", "heave", "roll", "pitch", "yaw")


def main():
    arrays = {}
    for deck in DECKS:
        with open(os.path.join(REFERENCE_DATA, deck + ".yaml")) as f:
            full = yaml.load(f, Loader=yaml.FullLoader)
        design = {"mooring": full["mooring"], "site": full["site"]}
        rho, g = float(full["site"].get("rho_water", 1025.0)), float(full["site"].get("g", 9.81))
        lines, depth = lines_from_design(design, rho=rho, g=g)
        with open(os.path.join(REFERENCE_DATA, deck + "_true_analyzeCases.pkl"), "rb") as f:
            cm = pickle.load(f)["case_metrics"]
        poses, tm = [], []
        for ic in sorted(cm):
            m = cm[ic][0]
            x = np.array([float(m[k + "_avg"]) for k in DOF])
            x[3:] = np.deg2rad(x[3:])
            poses.append(x)
            tm.append(np.asarray(m["Tmoor_avg"], dtype=float))
        poses, tm = np.array(poses), np.array(tm)
        ref = mr.evaluate(np.broadcast_to(lines, (len(poses),) + lines.shape), poses, depth)
        assert not ref["flags"].any()
        worst = float(np.max(np.abs(ref["T"].astype(float) - tm) / np.abs(tm)))
        print("%-28s %d lines, %d cases, depth %.0f: worst |T - Tmoor_avg| / Tmoor_avg = %.2e" % (deck, len(lines), len(poses), depth, worst))
        arrays[deck + "/design"] = np.array(json.dumps(design, sort_keys=True))
        arrays[deck + "/lines"] = lines
        arrays[deck + "/depth"] = np.array(depth)
        arrays[deck + "/rho"] = np.array(rho)
        arrays[deck + "/g"] = np.array(g)
        arrays[deck + "/poses"] = poses
        arrays[deck + "/Tmoor_avg"] = tm
    np.savez_compressed(OUT, **arrays)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
