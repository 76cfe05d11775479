"""Eigen analysis (include/raftx_modal.h), what needs no GPU: the entry points are exported by the device library and
kept out of raftx.h's contract, the oracle refuses them cleanly, the committed reference fixture is pinned by a fresh
numpy restatement of the reference procedure, the new kernel has no private segment, and dropin.install() patches
exactly what it patched before unless eigen=True is asked for."""
import os
import re

import numpy as np
import pytest

from raft_amd import snapshot as standin
from raft_amd._abi import EXPORTS, MODAL_EXPORTS, RaftxError, RaftxLib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "raftx_modal.h")
HIP_LIB = os.path.join(ROOT, "raft_amd", "csrc", "libraftx_hip.so")

FX = standin.load_fixture("modal_reference.npz")
UNITS = FX["units"]


def reference_eigen(M, C):
    """raft_fowt.py:1676-1703 restated: eig(solve(M, C)), the DOF claim of rows 5 .. 0, fn in Hz."""
    lam, vec = np.linalg.eig(np.linalg.solve(M, C))
    claimed = []
    for i in range(5, -1, -1):
        v = np.abs(vec[i, :]).copy()
        for _ in range(6):
            j = int(np.argmax(v))
            if j in claimed:
                v[j] = 0.0
            else:
                claimed.append(j)
                break
    claimed.reverse()
    return np.sqrt(lam[claimed]) / 2.0 / np.pi, vec[:, claimed]


def unit_matrices(u, model_order=True):
    """M_tot, C_tot of a fixture unit as Model.solveEigen (model_order) or FOWT.solveEigen sums them."""
    M = np.zeros((6, 6))
    M += u["M_struc"] + u["A_hydro_morison"] + u["A_BEM0"]
    C = np.zeros((6, 6))
    if model_order:
        C += u["C_struc"] + u["C_hydro"] + u["C_moor"] + u["C_elast"]
        C[5, 5] += u["yawstiff"]
    else:
        C += u["C_moor"]
        C[5, 5] += u["yawstiff"]
        C += u["C_struc"] + u["C_hydro"] + u["C_elast"]
    return M, C


def header_prototypes():
    return set(re.findall(r"^int\s+(raftx_\w+)\s*\(", open(HEADER).read(), re.M))


def test_modal_header_is_separate_from_the_oracle_contract():
    protos = header_prototypes()
    assert protos == set(MODAL_EXPORTS)
    assert not protos & set(EXPORTS)
    base = set(re.findall(r"\b(raftx_\w+)\s*\(", open(os.path.join(ROOT, "include", "raftx.h")).read()))
    assert not protos & base


@pytest.mark.skipif(not os.path.exists(HIP_LIB), reason="needs the built device library")
def test_device_library_exports_the_modal_entries():
    import ctypes
    lib = ctypes.CDLL(HIP_LIB)
    for name in header_prototypes():
        assert hasattr(lib, name), name
    assert RaftxLib(HIP_LIB).has_modal


def test_oracle_binds_and_refuses_modal(oracle_ctx):
    assert not oracle_ctx.rlib.has_modal
    with pytest.raises(RaftxError, match="raftx_modal.h"):
        oracle_ctx.modal_batch(np.eye(6)[None] * 1e6, np.eye(6)[None] * 1e5)
    with pytest.raises(RaftxError):
        oracle_ctx.modal_resident()


def test_fixture_is_the_reference_procedure():
    """Every recorded fns (both reference entry points) reproduced by the restatement to 1e-12; the units the reference
    refused carry its message and NaN results."""
    n_ok = 0
    for u in UNITS:
        assert u["nDOF"] == 6
        if u["error"]:
            assert "small or negative diagonals" in u["error"] or "negative system eigenvalues" in u["error"]
            assert np.all(np.isnan(u["model_fns"]))
            continue
        n_ok += 1
        for model_order, key in ((True, "model_fns"), (False, "fowt_fns")):
            fn, modes = reference_eigen(*unit_matrices(u, model_order))
            assert np.max(np.abs(fn - u[key]) / np.abs(u[key])) < 1e-12, (u["name"], key)
            mref = u[key.replace("fns", "modes")]
            assert np.allclose(np.abs(np.sum(modes * mref, axis=0)), 1.0, atol=1e-9), u["name"]
    assert n_ok >= 60
    names = [u["name"] for u in UNITS]
    assert {"OC3spar", "VolturnUS-S", "VolturnUS-S-pointInertia", "OC4semi-WAMIT_Coefs"} <= set(names)
    assert sum(n.startswith("C3-variant-") for n in names) == 64
    spar = UNITS[names.index("OC3spar")]
    assert spar["yawstiff"] > 0
    assert np.abs(UNITS[names.index("OC4semi-WAMIT_Coefs")]["A_BEM0"]).max() > 0


@pytest.mark.skipif(not os.path.exists(HIP_LIB), reason="needs the built device library")
def test_modal_kernel_has_no_private_segment():
    from tests import test_code_object as tco
    if not os.path.exists(os.path.join(tco.LLVM, "clang-offload-bundler")):
        pytest.skip("needs the ROCm LLVM tools")
    import tempfile

    class _F:
        def mktemp(self, name):
            import pathlib
            return pathlib.Path(tempfile.mkdtemp(prefix=name))
    notes = tco.kernel_notes(tco.code_object.__wrapped__(_F()))
    mine = {n: k for n, k in notes.items() if "k_modal" in n}
    assert mine, sorted(notes)[:5]
    for n, k in mine.items():
        assert int(k["private_segment_fixed_size"]) == 0, n
        assert k["uses_dynamic_stack"] == "false", n


def test_install_without_eigen_patches_what_it_did():
    from oracle import ref_harness as rh
    if not rh.reference_available():
        pytest.skip("reference package not present")
    rh.import_raft()
    from raft import raft_model, raft_fowt
    from raft_amd import dropin
    orig = (raft_model.Model.solveEigen, raft_fowt.FOWT.solveEigen)
    saved = dropin.install()
    try:
        assert set(saved) == {"solveDynamics", "calcHydroExcitation", "calcHydroLinearization", "calcDragExcitation",
                              "calcQTF_slenderBody", "calcHydroForce_2ndOrd"}
        assert (raft_model.Model.solveEigen, raft_fowt.FOWT.solveEigen) == orig
    finally:
        dropin.uninstall(saved)
    saved = dropin.install(eigen=True)
    try:
        assert raft_model.Model.solveEigen is dropin.solveEigen and raft_fowt.FOWT.solveEigen is dropin.fowt_solveEigen
    finally:
        dropin.uninstall(saved)
    assert (raft_model.Model.solveEigen, raft_fowt.FOWT.solveEigen) == orig
