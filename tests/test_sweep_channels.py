"""Output channels of a sweep crossing (include/raftx_channels.h), what needs no GPU: the entry point is exported by the
device library and kept out of raftx.h's contract, the oracle refuses it cleanly, the argument errors of the sweep
classes, the new kernel has no private segment, and the committed reference fixture
(tests/golden/refgold_sweep_outputs.npz: the reference's own saveTurbineOutputs standard deviations of four VolturnUS-S
variants x two load cases, scripts/make_sweep_outputs_golden.py) is reproduced by the oracle's resident path through the
rows of raft_amd.dropin.sweep_output_rows within 1e-8 x the key's largest value + 1e-12 -- the gate
tests/test_dropin_live_reference.py uses for these keys."""
import os
import re

import numpy as np
import pytest

from raft_amd import snapshot as standin
from raft_amd._abi import CHANNEL_EXPORTS, CURRENT_EXPORTS, EXPORTS, MODAL_EXPORTS, RaftxError, RaftxLib
from raft_amd.geometry import DesignTables
from raft_amd.sweep import GeometrySweep, VariantSweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "raftx_channels.h")
HIP_LIB = os.path.join(ROOT, "raft_amd", "csrc", "libraftx_hip.so")

FX = standin.load_fixture("refgold_sweep_outputs.npz")
KEYS = list(FX["keys"])
DEG = 57.29577951308232


def header_prototypes(path=HEADER):
    return set(re.findall(r"^int\s+(raftx_\w+)\s*\(", open(path).read(), re.M))


def fixture_sweep():
    """The GeometrySweep of the fixture's four variants and two load cases."""
    s = FX["sweep"]
    tabs = DesignTables(*(np.asarray(s[k]) for k in ("member_off", "members", "station_off", "stations", "cap_off", "caps")))
    return GeometrySweep(tabs, s["M_extra"], s["B0"], s["C_extra"], s["w"], s["k"], float(s["depth"]), s["zeta"], s["beta"],
                         int(s["nIter"]), float(s["XiStart"]), tol=float(s["tol"]), add_mask=int(s["add_mask"]),
                         rho=float(s["rho"]), g=float(s["g"]))


def fixture_rows():
    """(L, Gw) of the fixture: the rows of sweep_output_rows of the base unit."""
    r = FX["rows"]
    return np.asarray(r["L"]), (None if r["Gw"] is None else np.asarray(r["Gw"]))


def motion_rows():
    L = np.zeros((6, 3, 6))
    for j in range(6):
        L[j, 0, j] = 1.0 if j < 3 else DEG
    return L


def check_against_reference(std_by_key, what):
    """std_by_key[key] [variant, case(, rotor)] against the recorded reference values, key by key and pair by pair."""
    worst = 0.0
    for key in KEYS:
        ref = np.asarray(FX["ref"][key])
        got = np.asarray(std_by_key[key]).reshape(ref.shape)
        for d in range(ref.shape[0]):
            for c in range(ref.shape[1]):
                gate = 1e-8 * np.max(np.abs(ref[d, c])) + 1e-12
                err = np.max(np.abs(got[d, c] - ref[d, c]))
                worst = max(worst, err / gate)
                assert err <= gate, (what, key, d, c, float(err / gate))
    print("%s: worst %.3g of the gate 1e-8 max + 1e-12" % (what, worst))


def test_channels_header_is_separate_from_the_other_contracts():
    protos = header_prototypes()
    assert protos == set(CHANNEL_EXPORTS)
    assert not protos & set(EXPORTS) and not protos & set(MODAL_EXPORTS) and not protos & set(CURRENT_EXPORTS)
    for other in ("raftx.h", "raftx_modal.h", "raftx_current.h"):
        names = set(re.findall(r"\b(raftx_\w+)\s*\(", open(os.path.join(ROOT, "include", other)).read()))
        assert not protos & names, other
    text = open(HEADER).read()
    for cite in ("raft_fowt.py:2422-2444", "2500-2537", "2356-2373", "omdao_raft.py:870-876"):
        assert cite in text, cite
    assert re.search(r"#define\s+RAFTX_SWEEP_CHAN_MAX\s+64\b", text)


@pytest.mark.skipif(not os.path.exists(HIP_LIB), reason="needs the built device library")
def test_device_library_exports_the_channels_entry():
    import ctypes
    lib = ctypes.CDLL(HIP_LIB)
    for name in header_prototypes():
        assert hasattr(lib, name), name
    assert RaftxLib(HIP_LIB).has_channels


def test_oracle_binds_and_refuses_channels(oracle_ctx):
    assert not oracle_ctx.rlib.has_channels
    with pytest.raises(RaftxError, match="raftx_channels.h"):
        oracle_ctx.sweep_channels({"slot": 0, "out": {"niter": np.zeros((1, 1))}}, np.zeros((1, 3, 6)))


class _Recorder:
    """A context that records what _with_channels asks of it."""

    def __init__(self):
        self.cancelled, self.asked = [], []

    def sweep_cancel(self, handle):
        self.cancelled.append(handle)

    def sweep_channels(self, handle, L, Gw=None):
        self.asked.append((handle, L, Gw))
        return handle


@pytest.mark.parametrize("cls", [GeometrySweep, VariantSweep])
def test_with_channels_argument_errors(cls):
    L = np.zeros((2, 3, 6))
    ctx, h = _Recorder(), {"slot": 1}
    assert cls._with_channels(ctx, h, None) is h and not ctx.asked and not ctx.cancelled
    assert cls._with_channels(ctx, h, dict(L=L)) is h and ctx.asked[-1][1] is L and ctx.asked[-1][2] is None
    G = np.zeros((2, 6, 4), dtype=complex)
    cls._with_channels(ctx, h, dict(L=L, Gw=G))
    assert ctx.asked[-1][2] is G and not ctx.cancelled
    for bad in (dict(Gw=G), dict(L=None), dict(L=L, pow=[0, 1]), dict(L=L, psd=True), {}):
        n = len(ctx.cancelled)
        with pytest.raises(ValueError, match=r"channels=dict\(L="):
            cls._with_channels(ctx, h, bad)
        assert len(ctx.cancelled) == n + 1 and ctx.cancelled[-1] is h      # the prepared crossing is cancelled
    assert len(ctx.asked) == 2

    class _Refusing(_Recorder):
        def sweep_channels(self, handle, L, Gw=None):
            raise RaftxError("refused")
    ctx = _Refusing()
    with pytest.raises(RaftxError, match="refused"):
        cls._with_channels(ctx, h, dict(L=L))
    assert ctx.cancelled == [h]


@pytest.mark.skipif(not os.path.exists(HIP_LIB), reason="needs the built device library")
def test_channel_kernel_has_no_private_segment():
    from tests import test_code_object as tco
    if not os.path.exists(os.path.join(tco.LLVM, "clang-offload-bundler")):
        pytest.skip("needs the ROCm LLVM tools")
    import tempfile

    class _F:
        def mktemp(self, name):
            import pathlib
            return pathlib.Path(tempfile.mkdtemp(prefix=name))
    notes = tco.kernel_notes(tco.code_object.__wrapped__(_F()))
    mine = {n: k for n, k in notes.items() if "k_sweep_channels" in n}
    assert len(mine) == 2, sorted(mine)                                  # with and without Gw
    for n, k in mine.items():
        assert int(k["private_segment_fixed_size"]) == 0, n
        assert k["uses_dynamic_stack"] == "false", n
        assert int(k["group_segment_fixed_size"]) == 256, n              # one slot per (wave, channel of the tile)


def test_fixture_holds_what_it_should():
    assert np.asarray(FX["scales"]).shape == (4, 5)
    assert KEYS == [m + "_std" for m in ("surge", "sway", "heave", "roll", "pitch", "yaw")] + ["AxRNA_std", "AyRNA_std", "AzRNA_std", "Mbase_std"]
    sw = fixture_sweep()
    assert (sw.n_design, sw.n_case, sw.n_head, sw.nw) == (4, 2, 2, 30)
    assert np.all(sw.zeta[0, 1] == 0) and sw.zeta[1, 1].max() > 0.1 and np.all(sw.zeta[:, 0].max(axis=-1) > 0.1)   # one train | two trains
    L, Gw = fixture_rows()
    assert list(FX["rows"]["names"]) == ["AxRNA[0]", "AyRNA[0]", "AzRNA[0]", "Mbase[0]"] and L.shape == (4, 3, 6)
    assert Gw is None or Gw.shape == (4, 6, 30)
    for key in KEYS:
        ref = np.asarray(FX["ref"][key])
        assert ref.shape[:2] == (4, 2) and np.all(np.isfinite(ref)) and np.all(ref >= 0), key
    assert np.all(np.asarray(FX["ref"]["Mbase_std"]) > 1e6) and np.all(np.asarray(FX["ref"]["AxRNA_std"]) > 0)


def test_oracle_resident_path_reproduces_the_recorded_reference(oracle_ctx):
    """sweep.upload + run_channels on the fixture: the six motions and the rows of sweep_output_rows."""
    sw = fixture_sweep()
    L, Gw = fixture_rows()
    Lf = np.concatenate([motion_rows(), L])
    Gf = None if Gw is None else np.concatenate([np.zeros((6,) + Gw.shape[1:], dtype=complex), Gw])
    sw.upload(oracle_ctx)
    got = sw.run_channels(oracle_ctx, Lf, Gw=Gf)
    assert np.all(got["flags"] & 1) and not np.any(got["flags"] & 2)
    check_against_reference({key: got["std"][:, :, i] for i, key in enumerate(KEYS)}, "oracle, resident")
