"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/refgold_qtf_tables.npz from the LIVE reference (imported unmodified
through oracle/ref_harness.py, read-only).  Run in the build container only:

    python scripts/make_qtf_tables_golden.py

The device tests read the committed .npz, which holds data only (tests/test_qtf_tables.py borrows live_units / record from
here where the reference tree is present, to hold the committed records to the live reference):

  * "units": for every unit of tests/golden/geom_units.npz, rebuilt exactly as that fixture's generator builds it
    (oracle/make_golden.py fixture_geom) at its pose: the records raft_amd.qtf.pack_qtf makes of the live FOWT (strips
    [n,24], members [n,16]), its kay_geom (per MacCamy-Fuchs member rA, rB, r, ds, dls, p1, p2) and
    raft_amd.qtf.kay_items of it at the headings HEADINGS;
  * "empty": a design made of ONE member wholly above water (the tower of OC3spar, member `member` of that unit's
    descriptors): no strips, no member records (raft_member.py:1493-1494);
  * "deck": the VolturnUS-S test deck of refgold_qtf_VolturnUS-S.npz (oracle/make_golden.py fixture_qtf), whose model
    snapshot does not carry the design dictionary: its member descriptors (raft_amd.geometry.describe_unit) and the
    records of the live unit, which the script checks against pack_qtf of the committed snapshot, bit for bit.

The script checks that the first-order strip table of every live unit is the committed one of geom_units.npz, bit for
bit, reports how many waterline-crossing members, rectangular members and strips with the waterline scaling of
raft_member.py:1562-1568 the set contains, and fails if one of the counts is zero.
"""
import copy
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle import ref_harness as rh          # noqa: E402
from oracle import make_golden as mg          # noqa: E402
from raft_amd import geometry as G            # noqa: E402
from raft_amd import snapshot as standin      # noqa: E402
from raft_amd.qtf import pack_qtf, kay_items  # noqa: E402
from raft_amd.strips import pack_fowt         # noqa: E402

OUT = os.path.join(standin.GOLDEN_DIR, "refgold_qtf_tables.npz")
HEADINGS = (0.0, 0.4)
REF = rh.REFERENCE_ROOT


def same_table(fowt, strips, what):
    mine = pack_fowt(fowt).strips
    assert mine.shape == np.asarray(strips).shape and np.array_equal(mine, strips), what + ": the live unit is not the committed one"


def live_units(FX):
    """(name, live FOWT) of every unit of geom_units.npz, built as oracle/make_golden.py fixture_geom builds them."""
    committed = {u["name"]: u for u in FX["units"]}

    def one(design, r6=None):
        return rh.build_model(copy.deepcopy(design), r6=None if r6 is None else [r6]).fowtList[0]

    d = rh.prepare_design(rh.load_design(os.path.join(REF, "designs/OC3spar.yaml")))
    yield "OC3spar", one(d)
    d = rh.prepare_design(rh.load_design(os.path.join(REF, "tests/test_data/VolturnUS-S.yaml")))
    yield "VolturnUS-S-test@pose", one(d, [3.0, -2.0, -0.5, 0.02, -0.03, 0.1])
    d = rh.prepare_design(rh.load_design(os.path.join(REF, "examples/OC4semi-RAFT_QTF.yaml")))
    d["platform"].pop("outFolderQTF", None)
    yield "OC4semi", one(d)
    yield "OC4semi@heel", one(d, [-1.0, 4.0, 0.3, -0.05, 0.04, -0.2])
    base = rh.prepare_design(rh.load_design(os.path.join(REF, "examples/VolturnUS-S_example.yaml")))
    scales = np.asarray(FX["c3_scales"])
    for i in range(3):
        yield "C3-variant-%d" % i, one(mg.volturnus_variant(base, scales[i]))
    # the synthetic platform: the member list is data of the committed fixture (taken before the reference touched it)
    t = copy.deepcopy(rh.prepare_design(rh.load_design(os.path.join(REF, "designs/OC3spar.yaml"))))
    t["platform"]["members"] = json.loads(committed["synthetic"]["design_json"])["platform"]["members"]
    yield "synthetic@heel", one(t, [2.0, -1.0, 0.4, 0.06, -0.04, 0.3])
    yield "synthetic", one(t)
    d = rh.prepare_design(rh.load_design(os.path.join(REF, "designs/VolturnUS-S_farm.yaml")),
                          settings=dict(min_freq=0.002, max_freq=0.2))
    d["array"]["data"] = [[1, 1, 0, 0, 0, 180], [1, 1, 0, 1600, 0, 0],
                          [1, 1, 0, 0, 1600, 90], [1, 1, 0, 1600, 1600, 270]]
    m = rh.build_model(copy.deepcopy(d))
    for i, f in enumerate(m.fowtList):
        yield "farm-unit-%d" % i, f


def record(tab):
    return {"strips": tab.strips, "members": tab.members,
            "kay_geom": [{k: np.array(v, dtype=float) for k, v in gm.items()} for gm in tab.kay_geom],
            "kay_items": [kay_items(tab.kay_geom, b) for b in HEADINGS]}


def main():
    raft = rh.import_raft()
    FX = standin.load_fixture("geom_units.npz")
    committed = {u["name"]: u for u in FX["units"]}
    units, seen = [], []
    n_cross = n_rect = n_scaled = n_mcf = 0
    empty = None
    for name, fowt in live_units(FX):
        u = committed[name]
        same_table(fowt, u["strips"], name)
        assert np.array_equal(np.array(fowt.rReducedDOF, dtype=float), u["pose"]), name
        tab = pack_qtf(fowt)
        r = record(tab)
        r["name"] = name
        units.append(r)
        seen.append(name)
        n_cross += int(np.sum(tab.members[:, 0] != 0))
        n_mcf += len(tab.kay_geom)
        for mem in fowt.memberList:
            rA, rB = np.asarray(mem.rA, float), np.asarray(mem.rB, float)
            if rA[2] > 0 and rB[2] > 0:
                continue
            n_rect += mem.shape != "circular"
            rr, dls = np.asarray(mem.r, float), np.asarray(mem.dls, float)
            n_scaled += int(np.sum((rr[:, 2] < 0) & (rr[:, 2] + 0.5 * dls > 0)))
        print("%-24s strips %3d members %2d MCF %d items %s" % (name, len(tab.strips), len(tab.members), len(tab.kay_geom),
                                                                  [len(k) for k in r["kay_items"]]))
        if name == "OC3spar":
            tower = fowt.memberList[1]
            assert tower.rA[2] > 0 and tower.rB[2] > 0
            te = pack_qtf(fowt, memberList=[tower])
            assert te.strips.shape == (0, 24) and te.members.shape == (0, 16) and not te.kay_geom
            empty = {"unit": name, "member": 1, "strips": te.strips, "members": te.members}
    assert seen == [u["name"] for u in FX["units"]], "units of geom_units.npz: %s" % seen
    print("waterline-crossing members %d, rectangular members %d, strips with the waterline scaling %d, MCF members %d"
          % (n_cross, n_rect, n_scaled, n_mcf))
    assert n_cross > 0 and n_rect > 0 and n_scaled > 0 and n_mcf > 0
    # the deck of refgold_qtf_VolturnUS-S.npz, built as oracle/make_golden.py fixture_qtf builds it
    d = rh.prepare_design(rh.load_design(os.path.join(REF, "tests/test_data/VolturnUS-S.yaml")))
    dj = mg._design_subset(d)
    fowt = raft.Model(d).fowtList[0]
    fowt.setPosition(np.zeros(fowt.nDOF))
    fowt.calcStatics()
    fowt.calcHydroConstants()
    live = pack_qtf(fowt)
    snap = pack_qtf(standin.build_model(standin.load_fixture("refgold_qtf_VolturnUS-S.npz")["model"]).fowtList[0])
    assert np.array_equal(live.strips, snap.strips) and np.array_equal(live.members, snap.members), "deck: not the committed snapshot"
    t = G.describe_unit(json.loads(dj))
    deck = record(live)
    deck.update({"name": "VolturnUS-S", "source": "refgold_qtf_VolturnUS-S.npz", "gm": t.members, "station_off": t.station_off,
                 "gs": t.stations, "cap_off": t.cap_off, "caps": t.caps})
    fx = {"config": "pack_qtf records, kay_geom and kay_items of the live reference for the units of geom_units.npz",
          "headings": np.array(HEADINGS), "units": units, "empty": empty, "deck": deck}
    standin.save_fixture(OUT, fx)
    print("wrote %s (%d units, %d bytes)" % (OUT, len(units), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
