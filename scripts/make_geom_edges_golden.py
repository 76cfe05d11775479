"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/refgold_geom_edges.npz from the LIVE reference (imported unmodified
through oracle/ref_harness.py, read-only).  Run in the build container only:

    python scripts/make_geom_edges_golden.py

Never imported by the tests except to regenerate and compare where the reference tree is present; they read the
committed .npz, which holds recorded results only.

Every one-member unit of tests/geom_cases.py that a platform can hold (all but the nacelle member) and its two small
multi-member units become the platform of the OC3spar deck (massless rotor-nacelle assembly, no additional effects, the
deck's dry tower kept, potModMaster 0 so that a member's own potMod counts) at the unit's pose.  Recorded per unit, as the
reference's own methods leave them: the strip table packed from the live Member objects (positions, triads, constants:
setPosition, calcHydroConstants, the drag areas), A_hydro_morison, C_hydro, W_hydro, V, AWP, rCB (getHydrostatics through
calcStatics), M_struc, C_struc, W_struc, m, rCG (getInertia / getWeight through calcStatics) and, for the two ballasted
trim cases, Model.adjustBallastDensity under the vertical mooring force of the case list.  A unit the reference fails on
is recorded with its error.
"""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle import ref_harness as rh          # noqa: E402
from oracle import make_golden as mg          # noqa: E402
from raft_amd import snapshot as standin      # noqa: E402
from tests import geom_cases as gc            # noqa: E402

OUT = os.path.join(standin.GOLDEN_DIR, "refgold_geom_edges.npz")
KEEP = ("design_json", "pose", "rho", "g", "strips", "A_hydro_morison", "C_hydro", "W_hydro", "V", "AWP", "rCB")


def template():
    d = mg._bare(rh.prepare_design(rh.load_design(os.path.join(rh.REFERENCE_ROOT, "designs/OC3spar.yaml"))))
    d["platform"]["potModMaster"] = 0
    return d


def units_recorded():
    return [u for u in gc.ONE if u.part_of == "platform"] + gc.MULTI


def record(u, base):
    d = copy.deepcopy(base)
    d["platform"]["members"] = copy.deepcopy(u.deck)
    for i, mi in enumerate(d["platform"]["members"]):        # the deck reader wants unique names and an explicit potMod
        mi["name"] = "m%d" % i
        mi.setdefault("potMod", False)
    out = {"name": u.name}
    try:
        dj = mg._design_subset(d)
        m = rh.build_model(copy.deepcopy(d), r6=[list(u.pose)])
        full = mg._geom_unit(m.fowtList[0], dj)
        out.update({k: full[k] for k in KEEP})
        out.update(mg._bare_statics(m.fowtList[0]))
        if any(u is t for t in gc.TRIM):
            i = [t.name for t in gc.TRIM].index(u.name)
            out.update(mg._trimmed_statics(d, list(u.pose), Fz=float(gc.TRIM_FZ[i])))
    except Exception as e:                                    # recorded, not hidden
        out["error"] = "%s: %s" % (type(e).__name__, e)
    print("%-40s %s" % (u.name, out["error"] if "error" in out else "%d strips" % len(out["strips"])))
    return out


def build():
    rh.import_raft()
    base = template()
    return {"config": "geometry edge cases of tests/geom_cases.py through the live reference (OC3spar deck, bare RNA, tower kept)",
            "units": [record(u, base) for u in units_recorded()]}


def main():
    fx = build()
    standin.save_fixture(OUT, fx)
    print("wrote %s (%d units, %d bytes)" % (OUT, len(fx["units"]), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
