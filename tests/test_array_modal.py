"""Eigen analysis of moored arrays (include/raftx_array_modal.h), what needs no GPU.

* tests/csrc/array_modal_driver.cpp, a stand-alone host program built by g++ -ffp-contract=off, runs the serial core
  modal_core_n<N> of raft_amd/csrc/raftx_modal.h for N = 6 .. 36 and the wavefront schedule modal_wave<N> of
  raft_amd/csrc/raftx_array_modal.h with its lane loops run one lane after the other.  Every case of
  tests/golden/array_modal_reference.npz (mpmath at 50 digits, scripts/make_array_modal_golden.py) is held to the gate of
  tests/array_modal_cases.py: |lambda - lambda_ref| <= G n eps ||A_b||_F / s_j with G = 4 max(1, g) = 4 (g = 0.516 is LAPACK's
  own worst multiple over the committed cases), fn to half the relative gate plus 2 eps, modes to 1 - |<v, v_ref>| <= 1e-9
  (relative gap >= 1e-6) or a principal angle <= 1e-7 (clusters), and the DOF claim of the firm cases to the golden's.  The
  wave schedule returns the serial core's bits.  N = 6 on the units of modal_reference.npz reproduces the reference's
  recorded model_fns to 1e-9.  The same program passes under -fsanitize=address,undefined (nothing is preloaded).
* The header holds exactly ARRAY_MODAL_EXPORTS, the device library exports them, the oracle refuses them.
* Every k_array_modal instantiation of the gfx950 code object has 0 B scratch and no dynamic stack.
* The drop-in on stand-ins through a stub context: the refusal without arrays=True, the assembly of raft_model.py:450-476,
  the reference's errors.
"""
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from raft_amd._abi import ARRAY_MODAL_EXPORTS, EXPORTS, MODAL_COMPLEX, MODAL_NONPOSITIVE, RaftxError, RaftxLib
from raft_amd.strips import UnsupportedFOWT
from tests import array_modal_cases as amc
from tests.test_modal import UNITS, unit_matrices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "raftx_array_modal.h")
HIP_LIB = os.path.join(ROOT, "raft_amd", "csrc", "libraftx_hip.so")
DRIVER = os.path.join(ROOT, "tests", "csrc", "array_modal_driver.cpp")


# ------------------------------------------------------------------ the serial core and the wave schedule on the host
def _build(tmp, name, flags):
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", exe, DRIVER], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("array_modal")
    return tmp, _build(tmp, "array_modal_driver", ["-O2"])


def run_driver(tmp, exe, M, C, env=None):
    """(serial core, wave schedule), each dict(fn [nS,N], modes [nS,N,N], flags [nS]) and the raw words of both."""
    M, C = np.ascontiguousarray(M, dtype=np.float64), np.ascontiguousarray(C, dtype=np.float64)
    nS, N = M.shape[:2]
    fin, fout = str(tmp / "in.bin"), str(tmp / "out.bin")
    with open(fin, "wb") as f:
        np.array([nS, N], dtype=np.int32).tofile(f)
        M.tofile(f)
        C.tofile(f)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK "), (r.stdout[-500:], r.stderr[-3000:])
    raw = np.fromfile(fout).reshape(2, nS, N + N * N + 1)
    out = [dict(fn=w[:, :N], modes=w[:, N:N + N * N].reshape(nS, N, N), flags=w[:, -1].astype(np.int32)) for w in raw]
    return out[0], out[1], raw, r.stderr


def test_serial_core_and_wave_schedule_meet_the_gate_on_every_golden_case(driver):
    tmp, exe = driver
    gold = amc.golden()
    assert gold["G"] == 4.0 * max(1.0, gold["g"])
    assert set(amc.FIRM + amc.LOOSE) <= set(gold["cases"])
    sizes = set()
    for name, rec in gold["cases"].items():
        core, wave, raw, _ = run_driver(tmp, exe, rec["M"][None], rec["C"][None])
        sizes.add(len(rec["M"]))
        assert core["flags"][0] == 0 and wave["flags"][0] == 0, name
        amc.check_system(name, core["fn"][0], core["modes"][0], rec, gold["G"], firm=name in amc.FIRM)
        assert np.array_equal(raw[0].view(np.uint64), raw[1].view(np.uint64)), name     # the wave schedule: the core's bits
    assert sizes == {6, 12, 18, 24, 30, 36}


def test_flags_and_bits_of_both_schedules_on_seeded_systems(driver):
    tmp, exe = driver
    gold = amc.golden()["cases"]
    for name, unit in (("synthetic2", 1), ("synthetic6", 4)):
        M, C = np.asarray(gold[name]["M"]), np.asarray(gold[name]["C"])
        seeds = amc.flag_seeds(M, C, unit)
        Mn = M.copy()
        Mn[3, 2] = np.nan
        Ms = np.array([M] + [s[0] for s in seeds.values()] + [Mn, M[::-1, ::-1]])         # (the last one pivots in the LU of M)
        Cs = np.array([C] + [s[1] for s in seeds.values()] + [C, C[::-1, ::-1]])
        core, wave, raw, _ = run_driver(tmp, exe, Ms, Cs)
        assert np.array_equal(raw[0].view(np.uint64), raw[1].view(np.uint64)), name
        assert core["flags"][0] == 0 and core["flags"][-1] == 0
        k = len(seeds)
        amc.check_flag_seeds(core["flags"][1:k + 1], core["fn"][1:k + 1], core["modes"][1:k + 1], list(seeds))
        assert core["flags"][-2] & ~1 and np.all(np.isnan(core["fn"][-2]))


def test_serial_core_at_six_dofs_reproduces_the_recorded_reference_frequencies(driver):
    tmp, exe = driver
    units = [u for u in UNITS if not u["error"]]
    assert len(units) >= 60
    Ms, Cs = zip(*[unit_matrices(u) for u in units])
    core, wave, raw, _ = run_driver(tmp, exe, np.array(Ms), np.array(Cs))
    assert np.array_equal(raw[0].view(np.uint64), raw[1].view(np.uint64))
    for i, u in enumerate(units):
        assert core["flags"][i] == 0, u["name"]
        assert np.max(np.abs(core["fn"][i] - u["model_fns"]) / u["model_fns"]) <= 1e-9, u["name"]


def test_driver_is_clean_under_address_and_undefined_behaviour_sanitizers(driver):
    tmp, _ = driver
    san = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++"] + san + ["-o", str(tmp / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("sanitizer runtimes not installed: " + r.stderr[-300:])
    exe = _build(tmp, "array_modal_driver_san", san)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    gold = amc.golden()["cases"]
    for name in ("single_unit", "pair", "ring6"):
        rec = gold[name]
        M, C = np.asarray(rec["M"]), np.asarray(rec["C"])
        seeds = amc.flag_seeds(M, C, len(M) // 6 - 1).values()
        _, _, raw, err = run_driver(tmp, exe, np.array([M] + [s[0] for s in seeds]), np.array([C] + [s[1] for s in seeds]), env=env)
        assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err and "LeakSanitizer" not in err, err[-3000:]
        assert np.array_equal(raw[0].view(np.uint64), raw[1].view(np.uint64)), name


# ------------------------------------------------------------------ header, exports, oracle
def header_prototypes():
    return set(re.findall(r"^int\s+(raftx_\w+)\s*\(", open(HEADER).read(), re.M))


def test_array_modal_header_is_separate_from_the_oracle_contract():
    protos = header_prototypes()
    assert protos == set(ARRAY_MODAL_EXPORTS)
    assert not protos & set(EXPORTS)
    base = set(re.findall(r"\b(raftx_\w+)\s*\(", open(os.path.join(ROOT, "include", "raftx.h")).read()))
    assert not protos & base
    text = open(HEADER).read()
    assert '#include "raftx_modal.h"' in text and '#include "raftx_array_mooring.h"' in text


@pytest.mark.skipif(not os.path.exists(HIP_LIB), reason="needs the built device library")
def test_device_library_exports_the_array_modal_entries():
    import ctypes
    lib = ctypes.CDLL(HIP_LIB)
    for name in header_prototypes():
        assert hasattr(lib, name), name
    assert RaftxLib(HIP_LIB).has_array_modal


def test_oracle_binds_and_refuses_array_modal(oracle_ctx):
    assert not oracle_ctx.rlib.has_array_modal
    with pytest.raises(RaftxError, match="raftx_array_modal.h"):
        oracle_ctx.array_modal_batch(np.eye(12)[None] * 1e6, np.eye(12)[None] * 1e5)
    with pytest.raises(RaftxError, match="raftx_array_modal.h"):
        oracle_ctx.array_modal_moored(np.eye(6)[None, None] * 1e6, np.eye(6)[None, None] * 1e5, np.zeros((1, 1, 16)),
                                      np.zeros((1, 1, 6)), 200.0)


# ------------------------------------------------------------------ the drop-in on stand-ins, through a stub context
class StubCtx:
    """Stands in for the context: records the matrices of the one array call and answers with the golden's own numbers in
    the claimed order (or with a flag)."""

    def __init__(self, rec=None, flags=0):
        self.rec, self.flags, self.calls = rec, flags, []

    def array_modal_batch(self, M, C):
        self.calls.append((np.array(M), np.array(C)))
        n = M.shape[1]
        if self.flags & ~1:
            return dict(fn=np.full((1, n), np.nan), modes=np.full((1, n, n), np.nan), flags=np.array([self.flags], dtype=np.int32))
        cols, _ = amc.claim(np.asarray(self.rec["vec"]))
        return dict(fn=amc.fn_ref(self.rec)[cols][None], modes=np.asarray(self.rec["vec"])[:, cols][None],
                    flags=np.array([self.flags], dtype=np.int32))

    def modal_batch(self, M, C):
        raise AssertionError("an array goes through array_modal_batch")


def _unit_standin(u, nDOF=6):
    return SimpleNamespace(nDOF=nDOF, M_struc=u["M_struc"], A_hydro_morison=u["A_hydro_morison"],
                           A_BEM=np.asarray(u["A_BEM0"])[:, :, None] * np.ones(3), C_struc=u["C_struc"], C_hydro=u["C_hydro"],
                           C_moor=u["C_moor"], C_elast=u["C_elast"], yawstiff=u["yawstiff"], body=None)


def _array_standin(C_ms, moorMod=0, nDOF=6):
    ua, ub = [u for u in UNITS if u["name"] == "VolturnUS-S"][0], [u for u in UNITS if u["name"] == "OC3spar"][0]
    ms = SimpleNamespace(calls=[])

    def getCoupledStiffnessA(lines_only=False):
        ms.calls.append(lines_only)
        return C_ms
    ms.getCoupledStiffnessA = getCoupledStiffnessA
    model = SimpleNamespace(fowtList=[_unit_standin(ua), _unit_standin(ub, nDOF)], ms=ms, moorMod=moorMod, results={})
    return model, (ua, ub)


def test_dropin_arrays_on_standins():
    from raft_amd import dropin
    rec = amc.golden()["cases"]["pair"]
    rng = np.random.default_rng(3)
    C_ms = rng.uniform(-1e4, 1e4, size=(12, 12))
    model, (ua, ub) = _array_standin(C_ms)
    stub = StubCtx(rec)
    eng = dropin.Engine(stub)
    with pytest.raises(UnsupportedFOWT, match="arrays .* are not covered"):          # the default keeps today's refusal
        eng.solveEigen(model)
    assert not stub.calls and not model.ms.calls
    fns, modes = eng.solveEigen(model, arrays=True)
    assert model.ms.calls == [True]                                                  # lines_only=True
    (M, C), = stub.calls
    Mw, Cw = np.zeros((12, 12)), np.zeros((12, 12))
    for i, u in enumerate((ua, ub)):
        Mu, Cu = unit_matrices(u)
        Mw[6 * i:6 * i + 6, 6 * i:6 * i + 6] = Mu
        Cw[6 * i:6 * i + 6, 6 * i:6 * i + 6] = Cu
    assert M.shape == (1, 12, 12) and np.array_equal(M[0], Mw) and np.array_equal(C[0], Cw + C_ms)
    assert fns.shape == (12,) and modes.shape == (12, 12)
    assert model.results["eigen"]["frequencies"] is fns and model.results["eigen"]["modes"] is modes
    # the reference's errors
    bad = C_ms.copy()
    bad[8, 8] = -1e12
    with pytest.raises(RuntimeError, match="small or negative diagonals: Diagonal entry 8 of system stiffness matrix"):
        dropin.Engine(StubCtx(rec)).solveEigen(_array_standin(bad)[0], arrays=True)
    with pytest.raises(RuntimeError, match="zero or negative system eigenvalues"):
        dropin.Engine(StubCtx(rec, flags=MODAL_NONPOSITIVE)).solveEigen(_array_standin(C_ms)[0], arrays=True)
    with pytest.raises(UnsupportedFOWT, match="complex eigenvalue pair"):
        dropin.Engine(StubCtx(rec, flags=MODAL_COMPLEX)).solveEigen(_array_standin(C_ms)[0], arrays=True)
    # what stays refused
    with pytest.raises(UnsupportedFOWT, match="moorMod 2"):
        dropin.Engine(StubCtx(rec)).solveEigen(_array_standin(C_ms, moorMod=2)[0], arrays=True)
    with pytest.raises(UnsupportedFOWT, match="reduced DOFs"):
        dropin.Engine(StubCtx(rec)).solveEigen(_array_standin(C_ms, nDOF=12)[0], arrays=True)
    many, _ = _array_standin(C_ms)
    many.fowtList = many.fowtList * 4
    with pytest.raises(UnsupportedFOWT, match="1 to 6 units"):
        dropin.Engine(StubCtx(rec)).solveEigen(many, arrays=True)
