"""Mean current loads (include/raftx_current.h), what needs no GPU: the entry points are exported by the device library
and kept out of raftx.h's contract, the oracle refuses them cleanly, the committed reference fixture
(tests/golden/refgold_current.npz: the reference's own pickles and live FOWT.calcCurrentLoads values) is reproduced by the
extended-precision and the fp64 restatement of tests/current_reference.py within the gate of DESIGN.md section 4, the new
kernel has no private segment, and dropin.install() patches exactly what it patched before unless current=True is asked
for."""
import os
import re

import numpy as np
import pytest

from raft_amd import snapshot as standin
from raft_amd._abi import CURRENT_EXPORTS, EXPORTS, MODAL_EXPORTS, RaftxError, RaftxLib
from raft_amd.strips import pack_fowt
from tests import current_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "raftx_current.h")
HIP_LIB = os.path.join(ROOT, "raft_amd", "csrc", "libraftx_hip.so")

FX = standin.load_fixture("refgold_current.npz")
CURRENTS = np.asarray(FX["currents"])                         # [nCur, (speed, heading)]
UNITS = FX["units"]
DECKS = ("OC3spar", "VolturnUS-S", "VolturnUS-S-pointInertia", "OC4semi-WAMIT_Coefs")
_C3 = standin.load_fixture("c3_variants.npz")
_cache = {}


def unit_model(u):
    """The stand-in model of a fixture unit that is a deck or the pose model (rebuilt from the fixture it was snapshot
    into), with the attributes FOWT.calcCurrentLoads reads besides the members."""
    fx, model = standin.load_model_fixture(u["source"])
    fowt = model.fowtList[0]
    fowt.shearExp_water = float(u["shearExp"])
    assert float(fowt.depth) == float(u["depth"]) and float(fowt.rho_water) == float(u["rho"])
    return model, fowt


def unit_table(u):
    """Packed strips [n,32] of a fixture unit: the committed reference-packed table of a C3 variant, the packed stand-in
    of a deck (scripts/make_current_golden.py checked both against the live unit, bit for bit)."""
    if u["name"] not in _cache:
        if u["source"] == "c3_variants.npz":
            i, off = int(u["name"].rsplit("-", 1)[1]), np.asarray(_C3["strip_offsets"])
            _cache[u["name"]] = np.asarray(_C3["strips"])[off[i]:off[i + 1]]
        else:
            _cache[u["name"]] = pack_fowt(unit_model(u)[1]).strips
    return _cache[u["name"]]


def unit_reference(u, dtype=np.longdouble, Zref=None, shearExp=None):
    """(D, E) [nCur,6] of a fixture unit for the fixture's currents (cached for the extended-precision default)."""
    key = (u["name"], dtype, Zref, shearExp)
    if key not in _cache:
        s = unit_table(u)
        D, E = cr.current_loads(s, [0, len(s)], CURRENTS[:, 0], CURRENTS[:, 1], u["depth"],
                                u["Zref"] if Zref is None else Zref, u["shearExp"] if shearExp is None else shearExp, dtype=dtype)
        _cache[key] = (D[0], E[0])
    return _cache[key]


def header_prototypes():
    return set(re.findall(r"^int\s+(raftx_\w+)\s*\(", open(HEADER).read(), re.M))


def test_current_header_is_separate_from_the_oracle_contract():
    protos = header_prototypes()
    assert protos == set(CURRENT_EXPORTS)
    assert not protos & set(EXPORTS) and not protos & set(MODAL_EXPORTS)
    base = set(re.findall(r"\b(raftx_\w+)\s*\(", open(os.path.join(ROOT, "include", "raftx.h")).read()))
    assert not protos & base


@pytest.mark.skipif(not os.path.exists(HIP_LIB), reason="needs the built device library")
def test_device_library_exports_the_current_entries():
    import ctypes
    lib = ctypes.CDLL(HIP_LIB)
    for name in header_prototypes():
        assert hasattr(lib, name), name
    assert RaftxLib(HIP_LIB).has_current


def test_oracle_binds_and_refuses_current(oracle_ctx):
    assert not oracle_ctx.rlib.has_current
    with pytest.raises(RaftxError, match="raftx_current.h"):
        oracle_ctx.current_loads([1.0], [0.0], 200.0)
    with pytest.raises(RaftxError, match="raftx_current.h"):
        oracle_ctx.sweep_current({"slot": 0, "out": {"niter": np.zeros((1, 1))}}, [1.0], [0.0])


def test_fixture_holds_what_the_issue_lists():
    names = [u["name"] for u in UNITS]
    assert set(DECKS) <= set(names) and "VolturnUS-S-offset-pose" in names
    assert sum(n.startswith("C3-variant-") for n in names) == 64
    assert all(u["nDOF"] == 6 and u["D"].shape == (len(CURRENTS), 6) for u in UNITS)
    assert np.any(CURRENTS[:, 0] == 0) and {-70.0, 15.0, 90.0, 400.0} <= set(CURRENTS[:, 1]) and len(set(CURRENTS[:, 0]) - {0.0}) == 2
    assert [p["name"] for p in FX["pickle"]] == list(DECKS)
    assert FX["zref"]["Zref"] == -25.0 and FX["zref"]["shearExp"] == 0.2
    assert all(np.all(np.isfinite(u["D"])) for u in UNITS)          # only the dedicated below-seabed case may hold NaN


def test_pickles_are_the_live_values_and_inside_the_gate():
    """The reference's own goldens (speed 2.0, heading 15 deg) are, bit for bit, what the live reference gave for that
    current, and both restatements reproduce them within the gate."""
    ic = [i for i, (s, h) in enumerate(CURRENTS) if s == 2.0 and h == 15.0][0]
    for p in FX["pickle"]:
        u = UNITS[[x["name"] for x in UNITS].index(p["name"])]
        assert (p["speed"], p["heading"]) == (2.0, 15.0)
        assert np.array_equal(np.asarray(p["D"]).view(np.uint8), np.asarray(u["D"][ic]).view(np.uint8)), p["name"]
        D, E = unit_reference(u)
        m = cr.gate_multiples(p["D"], D[ic], E[ic]).max()
        m64 = cr.gate_multiples(unit_reference(u, np.float64)[0][ic], D[ic], E[ic]).max()
        print("%-28s pickle %.2f eps E, fp64 restatement %.2f eps E" % (p["name"], m, m64))
        assert m <= cr.GATE_C and m64 <= cr.GATE_C / 4


def test_gate_constant_is_what_the_cpu_measures():
    """C = 16 x the worst multiple of eps E over the whole fixture -- the reference's recorded values and the fp64 mode of
    the restatement, against the extended-precision evaluation -- rounded up to a power of two; the fp64 host mode stays
    inside C / 4.  Every entry of every unit is compared."""
    worst_ref = worst_64 = 0.0
    n = 0
    for u in UNITS:
        D, E = unit_reference(u)
        m_ref = cr.gate_multiples(u["D"], D, E)
        m_64 = cr.gate_multiples(unit_reference(u, np.float64)[0], D, E)
        assert m_ref.shape == m_64.shape == (len(CURRENTS), 6)
        n += m_ref.size
        worst_ref, worst_64 = max(worst_ref, m_ref.max()), max(worst_64, m_64.max())
    z = FX["zref"]
    u = UNITS[[x["name"] for x in UNITS].index(z["name"])]
    D, E = unit_reference(u, Zref=float(z["Zref"]), shearExp=float(z["shearExp"]))
    worst_ref = max(worst_ref, cr.gate_multiples(z["D"], D, E).max())
    worst_64 = max(worst_64, cr.gate_multiples(unit_reference(u, np.float64, float(z["Zref"]), float(z["shearExp"]))[0], D, E).max())
    assert not np.allclose(D, unit_reference(u)[0], rtol=1e-3)            # Zref and the exponent do enter
    print("worst multiple of eps E: recorded reference values %.2f, fp64 restatement %.2f (%d entries)" % (worst_ref, worst_64, n))
    assert n == len(UNITS) * len(CURRENTS) * 6
    worst = max(worst_ref, worst_64)
    assert cr.GATE_C == 2 ** int(np.ceil(np.log2(16 * worst)))
    assert worst_64 <= cr.GATE_C / 4


def test_reference_module_edge_cases():
    """No wet strip: zeros with a zero envelope; a strip below the seabed: NaN in that design only; speed 0: exact zeros."""
    s = np.array(unit_table(UNITS[0]))[:3].copy()
    dry = s.copy()
    dry[:, 2] = 1.0
    deep = s.copy()
    deep[1, 2] = -400.0
    strips = np.concatenate([s, dry, deep])
    D, E = cr.current_loads(strips, [0, 3, 6, 9], [1.5, 0.0], [20.0, 20.0], 320.0)
    assert np.all(D[1] == 0) and np.all(E[1] == 0)
    assert np.all(np.isnan(D[2])) and np.all(np.isfinite(D[0])) and np.any(D[0, 0] != 0)
    assert np.all(D[0, 1] == 0) and np.all(E[0, 1] == 0)
    m = cr.gate_multiples(np.where(np.isnan(D), np.nan, D), D, E)
    assert m.max() == 0
    assert np.isinf(cr.gate_multiples(np.zeros_like(D), D, E)[2]).all()      # a finite value where the reference has NaN fails


@pytest.mark.skipif(not os.path.exists(HIP_LIB), reason="needs the built device library")
def test_current_kernel_has_no_private_segment():
    from tests import test_code_object as tco
    if not os.path.exists(os.path.join(tco.LLVM, "clang-offload-bundler")):
        pytest.skip("needs the ROCm LLVM tools")
    import tempfile

    class _F:
        def mktemp(self, name):
            import pathlib
            return pathlib.Path(tempfile.mkdtemp(prefix=name))
    notes = tco.kernel_notes(tco.code_object.__wrapped__(_F()))
    mine = {n: k for n, k in notes.items() if "k_current_loads" in n}
    assert mine, sorted(notes)[:5]
    for n, k in mine.items():
        assert int(k["private_segment_fixed_size"]) == 0, n
        assert k["uses_dynamic_stack"] == "false", n
        assert int(k["group_segment_fixed_size"]) == 0, n


def test_install_without_current_patches_what_it_did():
    from oracle import ref_harness as rh
    if not rh.reference_available():
        pytest.skip("reference package not present")
    rh.import_raft()
    from raft import raft_fowt
    from raft_amd import dropin
    orig = raft_fowt.FOWT.calcCurrentLoads
    saved = dropin.install()
    try:
        assert set(saved) == {"solveDynamics", "calcHydroExcitation", "calcHydroLinearization", "calcDragExcitation",
                              "calcQTF_slenderBody", "calcHydroForce_2ndOrd"}
        assert raft_fowt.FOWT.calcCurrentLoads is orig
    finally:
        dropin.uninstall(saved)
    saved = dropin.install(current=True)
    try:
        assert raft_fowt.FOWT.calcCurrentLoads is dropin.calcCurrentLoads
        assert set(saved) == {"solveDynamics", "calcHydroExcitation", "calcHydroLinearization", "calcDragExcitation",
                              "calcQTF_slenderBody", "calcHydroForce_2ndOrd", "calcCurrentLoads"}
    finally:
        dropin.uninstall(saved)
    assert raft_fowt.FOWT.calcCurrentLoads is orig


def test_dropin_refuses_units_with_more_than_six_dofs():
    from types import SimpleNamespace
    from raft_amd import dropin
    from raft_amd.strips import UnsupportedFOWT
    with pytest.raises(UnsupportedFOWT, match="reduced DOFs"):
        dropin.Engine(ctx=object()).calcCurrentLoads(SimpleNamespace(nDOF=12), {"current_speed": 1.0})
