"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/modal_reference.npz from the LIVE reference (imported unmodified
through oracle/ref_harness.py, read-only).  Run in the build container only:

    python scripts/make_modal_golden.py

Never imported by the tests; they read the committed .npz.  Per unit it records the attributes FOWT.solveEigen /
Model.solveEigen read (raft_fowt.py:1627-1729, raft_model.py:436-547) and the reference's fns / modes of both calls:
OC3spar (yaw_stiffness, degenerate surge/sway and roll/pitch pairs), VolturnUS-S, VolturnUS-S-pointInertia,
OC4semi-WAMIT_Coefs (A_BEM[:,:,0] from the deck's WAMIT coefficients) and the 64 C3 sweep variants that
tests/test_geometry.py::c3_generated rebuilds from descriptors, all with the injected C_moor of build_model.
"""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle import ref_harness as rh          # noqa: E402
from oracle import make_golden as mg          # noqa: E402
from raft_amd import snapshot as standin      # noqa: E402

OUT = os.path.join(standin.GOLDEN_DIR, "modal_reference.npz")
KEYS = ("M_struc", "A_hydro_morison", "C_struc", "C_hydro", "C_moor", "C_elast")


def record(name, model):
    """A unit the reference refuses (RuntimeError of a small diagonal or a non-positive eigenvalue) keeps the message
    as "error" and NaN results."""
    fowt = model.fowtList[0]
    err = ""
    try:
        fns_f, modes_f = fowt.solveEigen()
        fns_m, modes_m = model.solveEigen()
    except RuntimeError as e:
        err = str(e)
        fns_f = fns_m = np.full(6, np.nan)
        modes_f = modes_m = np.full((6, 6), np.nan)
    u = {"name": name, "error": err, "nDOF": int(fowt.nDOF), "yawstiff": float(fowt.yawstiff),
         "A_BEM0": np.array(fowt.A_BEM[:, :, 0], dtype=float),
         "fowt_fns": np.array(fns_f, dtype=float), "fowt_modes": np.array(modes_f, dtype=float),
         "model_fns": np.array(fns_m, dtype=float), "model_modes": np.array(modes_m, dtype=float)}
    for k in KEYS:
        u[k] = np.array(getattr(fowt, k), dtype=float)
    print("%-28s fns %s  yawstiff %.3g  |A_BEM0| %.3g %s" % (name, np.array2string(np.asarray(fns_f), precision=5),
                                                                u["yawstiff"], np.abs(u["A_BEM0"]).max(), err[:60]))
    return u


def wamit_stand_in(deck_dir, hydro_path, tmp):
    """The deck's WAMIT .1 file (added mass: A_BEM) next to a zero-excitation .3 file on the same periods -- the
    reference tree ships the .1 only, and readHydro reads both; the excitation plays no part in the eigen problem."""
    from raft_amd import bem
    src = os.path.normpath(os.path.join(deck_dir, hydro_path))
    stem = os.path.join(tmp, os.path.basename(src))
    shutil.copy(src + ".1", stem + ".1")
    _, _, per = bem.read_wamit1(stem + ".1")
    w = 2 * np.pi / per[per > 0]
    bem.write_wamit3(stem + ".3", w, [0.0, 180.0], np.zeros((2, 6, len(w)), dtype=complex))
    return stem


def deck_unit(name, rel):
    path = os.path.join(rh.REFERENCE_ROOT, rel)
    d = rh.prepare_design(rh.load_design(path))
    hp = d["platform"].get("hydroPath")
    if d["platform"].get("potFirstOrder") and hp and not os.path.exists(os.path.join(os.path.dirname(path), hp) + ".3"):
        tmp = tempfile.mkdtemp()
        d["platform"]["hydroPath"] = wamit_stand_in(os.path.dirname(path), hp, tmp)
        d["platform"]["potSecOrder"] = 0
    cwd = os.getcwd()
    os.chdir(os.path.dirname(path))                  # hydroPath of the WAMIT deck is relative to the deck
    try:
        return record(name, rh.build_model(d))
    finally:
        os.chdir(cwd)


def main():
    units = [deck_unit("OC3spar", "designs/OC3spar.yaml"),
             deck_unit("VolturnUS-S", "tests/test_data/VolturnUS-S.yaml"),
             deck_unit("VolturnUS-S-pointInertia", "tests/test_data/VolturnUS-S-pointInertia.yaml"),
             deck_unit("OC4semi-WAMIT_Coefs", "tests/test_data/OC4semi-WAMIT_Coefs.yaml")]
    # the C3 variants of tests/test_geometry.py::c3_generated (geom_units.npz's base deck, c3_variants.npz's scales)
    FX = standin.load_fixture("geom_units.npz")
    C3 = standin.load_fixture("c3_variants.npz")
    base = rh.prepare_design(rh.load_design(os.path.join(rh.REFERENCE_ROOT, "examples/VolturnUS-S_example.yaml")))
    assert mg._design_subset(base) == FX["c3_base_json"], "the C3 base deck has changed"
    scales = np.asarray(C3["scales"])[:64]
    for i in range(len(scales)):
        units.append(record("C3-variant-%d" % i, rh.build_model(mg.volturnus_variant(base, scales[i]))))
    fx = {"config": "reference FOWT.solveEigen / Model.solveEigen per unit (build_model, injected C_moor)",
          "units": units}
    standin.save_fixture(OUT, fx)
    print("wrote %s (%d units, %d bytes)" % (OUT, len(units), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
