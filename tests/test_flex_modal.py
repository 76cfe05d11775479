"""Eigen analysis of units with flexible members (include/raftx_flex_modal.h), what needs no GPU.

* tests/csrc/flex_modal_driver.cpp, a stand-alone host program built by g++ -ffp-contract=off, runs (a) the serial core
  modal_core_n<N> of raft_amd/csrc/raftx_modal.h for N = 6, 12, 36, (b) the same method for n at run time as serial code
  (tests/csrc/flex_modal_serial.h) and (c) the lane schedule flex_modal_lanes of raft_amd/csrc/raftx_flex_modal.h -- what
  k_flex_modal runs -- with its lane loops run one lane after the other.  (b) and (c) return identical bits at every size; at
  6, 12 and 36 DOFs they equal (a) put in ascending order.  Every case of tests/golden/flex_modal_reference.npz (mpmath at 50
  digits, scripts/make_flex_modal_golden.py) meets the gates of tests/flex_modal_cases.py.  The flag seeds, the nModes rule.  The
  same program passes under -fsanitize=address,undefined (nothing is preloaded).
* The header holds exactly FLEX_MODAL_EXPORTS, the device library exports them, the oracle refuses the call by name.
* The drop-in on stand-ins through a stub context; FlexSweep.natural_modes through a stub context.
"""
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from raft_amd._abi import EXPORTS, FLEX_MODAL_EXPORTS, FLEX_MODAL_MAX_N, MODAL_COMPLEX, MODAL_NONPOSITIVE, RaftxError, RaftxLib
from raft_amd.strips import UnsupportedFOWT
from tests import array_modal_cases as amc
from tests import flex_modal_cases as fmc
from tests.test_modal import UNITS, unit_matrices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "raftx_flex_modal.h")
HIP_LIB = os.path.join(ROOT, "raft_amd", "csrc", "libraftx_hip.so")
DRIVER = os.path.join(ROOT, "tests", "csrc", "flex_modal_driver.cpp")
SIZES = (6, 7, 12, 36, 37, 64, 65, 129, 150, 240, 256)


# ------------------------------------------------------------------ the three variants on the host
def build_driver(tmp, name, flags):
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", exe, DRIVER], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("flex_modal")
    return tmp, build_driver(tmp, "flex_modal_driver", ["-O2"])


def run_driver(tmp, exe, M, C, n_modes=None, env=None):
    """(serial, lanes, core or None): dict(fn [nS,n], modes [nS,n,m], flags [nS], raw: the words of the variant); stderr."""
    M, C = np.ascontiguousarray(M, dtype=np.float64), np.ascontiguousarray(C, dtype=np.float64)
    nS, n = M.shape[:2]
    m = n if n_modes is None else n_modes
    fin, fout = str(tmp / "in.bin"), str(tmp / "out.bin")
    with open(fin, "wb") as f:
        np.array([nS, n, m], dtype=np.int32).tofile(f)
        M.tofile(f)
        C.tofile(f)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("OK "), (r.stdout[-500:], r.stderr[-3000:])
    raw = np.fromfile(fout)
    rec = n + n * m + 1

    def unpack(w, cols):
        return dict(fn=w[:, :n], modes=w[:, n:n + n * cols].reshape(nS, n, cols), flags=w[:, -1].astype(np.int32), raw=w.view(np.uint64))
    two = raw[:2 * nS * rec].reshape(2, nS, rec)
    rest = raw[2 * nS * rec:]
    core = unpack(rest.reshape(nS, n + n * n + 1), n) if rest.size else None
    return unpack(two[0], m), unpack(two[1], m), core, r.stderr


def system_of(n):
    """A system of n DOFs: the decks at 150 and 240, a seeded synthetic one elsewhere."""
    if n == 150:
        return fmc.deck_matrices("flex_volturnus.npz")
    if n == 240:
        return fmc.deck_matrices("flex_mcf.npz")
    return fmc.synthetic(n, 4200 + n)


@pytest.mark.parametrize("n", SIZES)
def test_lane_schedule_returns_the_serial_bits(driver, n):
    tmp, exe = driver
    M, C = system_of(n)
    serial, lanes, core, _ = run_driver(tmp, exe, M[None], C[None])
    assert serial["flags"][0] == 0
    assert np.array_equal(serial["raw"], lanes["raw"])
    assert (core is not None) == (n in (6, 12, 36))


def test_both_equal_the_template_core_in_ascending_order(driver):
    tmp, exe = driver
    gold = amc.golden()["cases"]
    units = [u for u in UNITS if not u["error"]][:8]
    batches = {6: [unit_matrices(u) for u in units], 12: [(gold["synthetic2"]["M"], gold["synthetic2"]["C"])],
               36: [(gold["synthetic6"]["M"], gold["synthetic6"]["C"])]}
    for n, systems in batches.items():
        M, C = np.array([s[0] for s in systems], dtype=float), np.array([s[1] for s in systems], dtype=float)
        serial, lanes, core, _ = run_driver(tmp, exe, M, C)
        assert np.array_equal(serial["raw"], lanes["raw"]), n
        for k in range(len(systems)):
            assert core["flags"][k] == 0 and lanes["flags"][k] == 0, (n, k)
            assert len(np.unique(core["fn"][k])) == n, (n, k, "tied frequencies")
            fn, modes = fmc.ascending(core["fn"][k], core["modes"][k])
            assert np.array_equal(fn.view(np.uint64), lanes["fn"][k].view(np.uint64)), (n, k)
            assert np.array_equal(modes.view(np.uint64), lanes["modes"][k].view(np.uint64)), (n, k)


@pytest.mark.parametrize("name", fmc.CASES)
def test_host_driver_meets_the_gates_on_every_golden_case(driver, name):
    tmp, exe = driver
    gold = fmc.golden()
    assert gold["digits"] >= 30 and gold["G"] == 4.0 * max(1.0, gold["g"])
    M, C = fmc.matrices(name)
    serial, lanes, _, _ = run_driver(tmp, exe, M[None], C[None])
    assert lanes["flags"][0] == 0 and np.array_equal(serial["raw"], lanes["raw"])
    fmc.check_system(name, lanes["fn"][0], lanes["modes"][0], label="host")


def seeded_batch(n):
    """Clean, the four flag seeds, a NaN system, clean: (M, C, the seeds' names)."""
    M, C = system_of(n)
    seeds = amc.flag_seeds(M, C, 0)
    Mn = M.copy()
    Mn[3, 2] = np.nan
    Ms = np.array([M] + [s[0] for s in seeds.values()] + [Mn, M])
    Cs = np.array([C] + [s[1] for s in seeds.values()] + [C, C])
    return Ms, Cs, list(seeds)


@pytest.mark.parametrize("n", (37, 150))
def test_flags_and_the_nan_rule_on_seeded_systems(driver, n):
    tmp, exe = driver
    Ms, Cs, names = seeded_batch(n)
    if n == 150:                                         # (the NaN system runs into the 30 n cap: kept to the small size)
        keep = [k for k in range(len(Ms)) if k != len(names) + 1]
        Ms, Cs = Ms[keep], Cs[keep]
    serial, lanes, _, _ = run_driver(tmp, exe, Ms, Cs, n_modes=5)
    assert np.array_equal(serial["raw"], lanes["raw"])
    k = len(names)
    assert lanes["flags"][0] == 0 and lanes["flags"][-1] == 0
    assert np.array_equal(lanes["raw"][0], lanes["raw"][-1])
    amc.check_flag_seeds(lanes["flags"][1:k + 1], lanes["fn"][1:k + 1], lanes["modes"][1:k + 1], names)
    if n == 37:
        assert lanes["flags"][k + 1] & ~1 and np.all(np.isnan(lanes["fn"][k + 1])) and np.all(np.isnan(lanes["modes"][k + 1]))


def test_results_do_not_depend_on_nmodes(driver):
    tmp, exe = driver
    M, C = system_of(37)
    full = run_driver(tmp, exe, M[None], C[None])[1]
    for m in (0, 3):
        serial, lanes, _, _ = run_driver(tmp, exe, M[None], C[None], n_modes=m)
        assert np.array_equal(serial["raw"], lanes["raw"]), m
        assert np.array_equal(lanes["fn"].view(np.uint64), full["fn"].view(np.uint64)), m
        assert np.array_equal(lanes["modes"].view(np.uint64), full["modes"][:, :, :m].view(np.uint64)), m


def test_driver_is_clean_under_address_and_undefined_behaviour_sanitizers(driver):
    tmp, _ = driver
    san = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++"] + san + ["-o", str(tmp / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("sanitizer runtimes not installed: " + r.stderr[-300:])
    exe = build_driver(tmp, "flex_modal_driver_san", san)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for n, m in ((6, 6), (7, 0), (12, 3), (37, 37), (65, 12)):
        Ms, Cs, _ = seeded_batch(n)
        if n > 12:                                       # (the NaN system's 30 n steps are slow under the sanitizers)
            Ms, Cs = Ms[:5], Cs[:5]
        serial, lanes, _, err = run_driver(tmp, exe, Ms, Cs, n_modes=m, env=env)
        assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err and "LeakSanitizer" not in err, err[-3000:]
        assert np.array_equal(serial["raw"], lanes["raw"]), n


# ------------------------------------------------------------------ header, exports, oracle
def header_prototypes():
    return set(re.findall(r"^int\s+(raftx_\w+)\s*\(", open(HEADER).read(), re.M))


def test_flex_modal_header_is_separate_from_the_oracle_contract():
    protos = header_prototypes()
    assert protos == set(FLEX_MODAL_EXPORTS)
    assert not protos & set(EXPORTS)
    base = set(re.findall(r"\b(raftx_\w+)\s*\(", open(os.path.join(ROOT, "include", "raftx.h")).read()))
    assert not protos & base
    text = open(HEADER).read()
    assert '#include "raftx_modal.h"' in text
    assert int(re.search(r"#define RAFTX_FLEX_MODAL_MAX_N (\d+)", text).group(1)) == FLEX_MODAL_MAX_N


@pytest.mark.skipif(not os.path.exists(HIP_LIB), reason="needs the built device library")
def test_device_library_exports_the_flex_modal_entry():
    import ctypes
    lib = ctypes.CDLL(HIP_LIB)
    for name in header_prototypes():
        assert hasattr(lib, name), name
    assert RaftxLib(HIP_LIB).has_flex_modal


def test_oracle_binds_and_refuses_flex_modal(oracle_ctx):
    assert not oracle_ctx.rlib.has_flex_modal
    with pytest.raises(RaftxError, match="raftx_flex_modal.h"):
        oracle_ctx.flex_modal_batch(np.eye(7)[None] * 1e6, np.eye(7)[None] * 1e5)


# ------------------------------------------------------------------ the Python layers through a stub context
class StubCtx:
    """Stands in for the context: records the matrices of each call and answers with numpy's ascending spectrum (or a flag)."""

    def __init__(self, flags=0):
        self.flags, self.calls = flags, []

    def flex_modal_batch(self, M, C, n_modes=None):
        self.calls.append((np.array(M), np.array(C), n_modes))
        nS, n = M.shape[:2]
        m = n if n_modes is None else n_modes
        if self.flags & ~1:
            return dict(fn=np.full((nS, n), np.nan), modes=np.full((nS, n, m), np.nan), flags=np.full(nS, self.flags, dtype=np.int32))
        fn, modes = np.zeros((nS, n)), np.zeros((nS, n, m))
        for k in range(nS):
            lam, vec = np.linalg.eig(np.linalg.solve(M[k], C[k]))
            o = np.argsort(lam.real, kind="stable")
            fn[k], modes[k] = np.sqrt(lam.real[o]) / 2 / np.pi, vec.real[:, o[:m]]
        return dict(fn=fn, modes=modes, flags=np.full(nS, self.flags, dtype=np.int32))

    def modal_batch(self, M, C):
        raise AssertionError("a unit with flexible members goes through flex_modal_batch")

    array_modal_batch = modal_batch


def deck_standin(yawstiff=0.0):
    u = fmc.deck_unit("flex_volturnus.npz")
    n = int(u["nDOF"])
    A_BEM = np.zeros((n, n, 3))
    A_BEM[:6, :6, 0] = np.diag([1e6, 1e6, 2e6, 3e8, 3e8, 1e8])
    fowt = SimpleNamespace(nDOF=n, M_struc=u["M_struc"], A_hydro_morison=u["A_hydro_morison"], A_BEM=A_BEM, C_struc=u["C_struc"],
                           C_hydro=u["C_hydro"], C_moor=u["C_moor"], C_elast=u["C_elast"], yawstiff=yawstiff, body=None)
    return fowt, SimpleNamespace(fowtList=[fowt], ms=None, moorMod=0, results={})


def test_dropin_flexible_units_on_standins():
    from raft_amd import dropin
    fowt, model = deck_standin(yawstiff=4e7)
    n = fowt.nDOF
    stub = StubCtx()
    eng = dropin.Engine(stub)
    with pytest.raises(UnsupportedFOWT, match="150 reduced DOFs are not covered"):      # the default keeps today's refusal
        eng.solveEigen(model)
    with pytest.raises(UnsupportedFOWT, match="150 reduced DOFs are not covered"):
        eng.fowt_solveEigen(fowt)
    with pytest.raises(UnsupportedFOWT, match="150 reduced DOFs are not covered"):
        eng.solveEigen(model, arrays=True)
    assert not stub.calls
    Mw = fowt.M_struc + fowt.A_hydro_morison + fowt.A_BEM[:, :, 0]
    Cm = fowt.C_struc + fowt.C_hydro + fowt.C_moor + fowt.C_elast                       # raft_model.py:460-464
    Cm[5, 5] += fowt.yawstiff
    Cf = np.zeros((n, n)) + fowt.C_moor                                                # raft_fowt.py:1627-1644 (getStiffness)
    Cf[5, 5] += fowt.yawstiff
    Cf += fowt.C_struc + fowt.C_hydro + fowt.C_elast
    for call, Cw in ((lambda: eng.solveEigen(model, flexible=True), Cm), (lambda: eng.fowt_solveEigen(fowt, flexible=True), Cf)):
        stub.calls.clear()
        fns, modes = call()
        (M, C, n_modes), = stub.calls
        assert n_modes is None and M.shape == (1, n, n)
        assert np.array_equal(M[0], Mw) and np.array_equal(C[0], Cw)
        assert fns.shape == (n,) and modes.shape == (n, n) and np.all(np.diff(fns) >= 0)
    assert model.results["eigen"]["frequencies"].shape == (n,) and model.results["eigen"]["modes"].shape == (n, n)
    # the reference's errors, the flags
    bad, bad_model = deck_standin()
    bad.C_struc = np.array(bad.C_struc)
    bad.C_struc[8, 8] = -1e15
    with pytest.raises(RuntimeError, match="small or negative diagonals: Diagonal entry 8 of system stiffness matrix"):
        dropin.Engine(StubCtx()).solveEigen(bad_model, flexible=True)
    with pytest.raises(RuntimeError, match="zero or negative system eigenvalues"):
        dropin.Engine(StubCtx(flags=MODAL_NONPOSITIVE)).solveEigen(deck_standin()[1], flexible=True)
    with pytest.raises(UnsupportedFOWT, match="complex eigenvalue pair"):
        dropin.Engine(StubCtx(flags=MODAL_COMPLEX)).fowt_solveEigen(deck_standin()[0], flexible=True)
    # what stays refused: arrays of units with flexible members, with or without the array keyword
    pair = deck_standin()[1]
    pair.fowtList = pair.fowtList * 2
    for kw in (dict(flexible=True), dict(flexible=True, arrays=True)):
        with pytest.raises(UnsupportedFOWT):
            dropin.Engine(StubCtx()).solveEigen(pair, **kw)
    moored = deck_standin()[1]
    moored.ms = SimpleNamespace(getCoupledStiffnessA=lambda lines_only=False: np.zeros((150, 150)))
    for kw in (dict(flexible=True), dict(flexible=True, arrays=True)):
        with pytest.raises(UnsupportedFOWT):
            dropin.Engine(StubCtx()).solveEigen(moored, **kw)
    # a rigid unit under flexible=True is still the rigid path
    rigid = SimpleNamespace(nDOF=6)
    assert dropin.Engine._eigen_unit(rigid, "x", flexible=True) is False


def test_flexsweep_natural_modes_shapes_and_sums():
    from raft_amd.flex import FlexSweep, FlexUnit
    n = 13
    units = []
    for k in range(3):
        M, C = fmc.synthetic(n, 900 + k)
        units.append(FlexUnit([], np.zeros((0, 6, n)), M, np.zeros((n, n)), C))
    sweep = FlexSweep(units, np.linspace(0.1, 1, 4), np.linspace(0.01, 0.1, 4), 200.0, np.ones((1, 1, 4)), np.zeros((1, 1)), 5, 0.1)
    stub = StubCtx()
    out = sweep.natural_modes(stub)
    assert stub.calls[-1][2] == 12                                                    # (the library refuses more modes than DOFs)
    out = sweep.natural_modes(stub, n_modes=4)
    assert out["fn"].shape == (3, n) and out["modes"].shape == (3, n, 4) and out["flags"].shape == (3,)
    M, C, _ = stub.calls[-1]
    assert np.array_equal(M, np.array([u.M for u in units])) and np.array_equal(C, np.array([u.C for u in units]))
    dM = np.zeros((n, n))
    dM[:6, :6] = np.diag([1e6] * 6)
    dC = np.arange(3 * n * n, dtype=float).reshape(3, n, n)
    sweep.natural_modes(stub, n_modes=None, dM=dM, dC=dC)
    M, C, m = stub.calls[-1]
    assert m is None
    assert np.array_equal(M, np.array([u.M + dM for u in units])) and np.array_equal(C, np.array([u.C + dC[k] for k, u in enumerate(units)]))
    assert np.array_equal(units[0].M, fmc.synthetic(n, 900)[0])                       # the units themselves are untouched
    with pytest.raises(ValueError, match="dM has shape"):
        sweep.natural_modes(stub, dM=np.zeros((2, n, n)))
