"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/refgold_current.npz from the LIVE reference (imported unmodified
through oracle/ref_harness.py, read-only).  Run in the build container only:

    python scripts/make_current_golden.py

Never imported by the tests; they read the committed .npz, which holds data only:

  * "pickle": the reference's own goldens tests/test_data/<deck>_true_calcCurrentLoads.pkl (speed 2.0, heading 15 deg,
    tests/test_fowt.py:178-182) of the four rigid decks, bit-equal;
  * "units": live FOWT.calcCurrentLoads (raft_fowt.py:1961-1985) of those decks, of the offset-pose model of
    pose_volturnus_mcf.npz and of the 64 C3 sweep variants of c3_variants.npz, for the currents CURRENTS (speed 0, the
    headings -70 / 15 / 90 / 400 deg at two speeds), with the depth, exponent and Zref the reference used;
  * "zref": Member.calcCurrentLoads(..., Zref=-25, shearExp_water=0.2) of every member of one deck summed by hand about
    the PRP -- Zref and the exponent pinned without a rotor.

Every unit is built exactly as the fixture whose stand-in the tests rebuild it from (oracle/make_golden.py:
fixture_ref_goldens, fixture_pose, fixture_c3), and the script checks that the packed strip table of the live unit is
the stand-in's (the decks, the pose model) or the committed one (the C3 variants), bit for bit.
"""
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle import ref_harness as rh          # noqa: E402
from oracle import make_golden as mg          # noqa: E402
from raft_amd import snapshot as standin      # noqa: E402
from raft_amd.strips import pack_fowt         # noqa: E402

OUT = os.path.join(standin.GOLDEN_DIR, "refgold_current.npz")
DECKS = ("OC3spar", "VolturnUS-S", "VolturnUS-S-pointInertia", "OC4semi-WAMIT_Coefs")
SPEEDS = (2.0, 0.6)
HEADINGS = (-70.0, 15.0, 90.0, 400.0)
CURRENTS = [(0.0, 15.0)] + [(s, h) for s in SPEEDS for h in HEADINGS]          # (speed m/s, heading deg)


def live_loads(fowt):
    return np.array([np.array(fowt.calcCurrentLoads({"current_speed": s, "current_heading": h}), dtype=float)
                     for s, h in CURRENTS])


def record(name, fowt, source):
    Zref = 0.0
    for rot in fowt.rotorList:                       # raft_fowt.py:1971-1974
        if rot.r3[2] < 0:
            Zref = float(rot.r3[2])
    u = {"name": name, "source": source, "depth": float(fowt.depth), "shearExp": float(fowt.shearExp_water),
         "rho": float(fowt.rho_water), "Zref": Zref, "nDOF": int(fowt.nDOF), "D": live_loads(fowt)}
    print("%-28s depth %.1f exp %.3f Zref %.1f  |D| max %.4g" % (name, u["depth"], u["shearExp"], Zref, np.abs(u["D"]).max()))
    return u


def same_table(fowt, strips, what):
    mine = pack_fowt(fowt).strips
    assert mine.shape == np.asarray(strips).shape and np.array_equal(mine, strips), what + ": the live unit is not the committed one"


def deck_fowt(raft, name):
    """The unit of oracle/make_golden.py fixture_ref_goldens (= tests/test_fowt.py create_fowt + the hydro constants)."""
    d = rh.prepare_design(rh.load_design(os.path.join(rh.REFERENCE_ROOT, "tests/test_data", name + ".yaml")))
    if name == "OC4semi-WAMIT_Coefs":
        d["platform"]["potFirstOrder"] = 0
        d["platform"]["potSecOrder"] = 0
    fowt = raft.Model(d).fowtList[0]
    fowt.setPosition(np.zeros(fowt.nDOF))
    fowt.calcStatics()
    fowt.calcHydroConstants()
    return fowt


def main():
    raft = rh.import_raft()
    units, pickles = [], []
    zref = None
    for name in DECKS:
        fowt = deck_fowt(raft, name)
        fx, model = standin.load_model_fixture("refgold_%s.npz" % name)
        same_table(fowt, pack_fowt(model.fowtList[0]).strips, name)
        with open(os.path.join(rh.REFERENCE_ROOT, "tests/test_data", name + "_true_calcCurrentLoads.pkl"), "rb") as f:
            pickles.append({"name": name, "speed": 2.0, "heading": 15.0, "D": np.array(pickle.load(f), dtype=float)})
        units.append(record(name, fowt, "refgold_%s.npz" % name))
        if name == "VolturnUS-S":
            D = np.zeros((len(CURRENTS), 6))
            for i, (s, h) in enumerate(CURRENTS):
                for mem in fowt.memberList:         # rigid members: one node each, all about the PRP (raft_fowt.py:1976-1983)
                    D[i] += fowt.T.T[:, mem.nodeList[0].id * 6:mem.nodeList[0].id * 6 + 6] @ mem.calcCurrentLoads(
                        fowt.depth, speed=s, heading=h, Zref=-25.0, shearExp_water=0.2, rho=fowt.rho_water, g=fowt.g)
            zref = {"name": name, "source": "refgold_%s.npz" % name, "depth": float(fowt.depth), "Zref": -25.0,
                    "shearExp": 0.2, "D": D}
    # the offset-pose model of oracle/make_golden.py fixture_pose
    d = rh.prepare_design(rh.load_design(os.path.join(rh.REFERENCE_ROOT, "tests/test_data/VolturnUS-S.yaml")),
                          settings=dict(XiStart=0.1, nIter=15))
    d["platform"]["potSecOrder"] = 0
    fowt = rh.build_model(d, r6=[[3.0, -2.0, -0.5, 0.02, -0.03, 0.1]]).fowtList[0]
    fx, model = standin.load_model_fixture("pose_volturnus_mcf.npz")
    same_table(fowt, pack_fowt(model.fowtList[0]).strips, "pose model")
    units.append(record("VolturnUS-S-offset-pose", fowt, "pose_volturnus_mcf.npz"))
    # the C3 variants of oracle/make_golden.py fixture_c3
    C3 = standin.load_fixture("c3_variants.npz")
    base = rh.prepare_design(rh.load_design(os.path.join(rh.REFERENCE_ROOT, "examples/VolturnUS-S_example.yaml")))
    scales, off = np.asarray(C3["scales"])[:64], np.asarray(C3["strip_offsets"])
    for i in range(len(scales)):
        fowt = rh.build_model(mg.volturnus_variant(base, scales[i])).fowtList[0]
        same_table(fowt, np.asarray(C3["strips"])[off[i]:off[i + 1]], "C3 variant %d" % i)
        units.append(record("C3-variant-%d" % i, fowt, "c3_variants.npz"))
    fx = {"config": "reference FOWT.calcCurrentLoads per unit and current; the reference's own pickles; one deck with Zref / exponent",
          "currents": np.array(CURRENTS), "pickle": pickles, "units": units, "zref": zref}
    standin.save_fixture(OUT, fx)
    print("wrote %s (%d units, %d bytes)" % (OUT, len(units), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
