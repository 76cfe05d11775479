"""The mean-pose request of a sweep crossing (raftx_sweep_mean_pose, include/raftx_statics.h), what needs no GPU: the
prototype is in the header, the built device library exports the symbol and raft_amd/_abi.py binds it, the sweep classes
validate the request's dict before anything reaches a library, and ``take`` shards a standing request with the designs."""
import ctypes
import os
import re

import numpy as np
import pytest

from raft_amd._abi import EXPORTS, STATICS_EXPORTS, RaftxLib
from raft_amd.sweep import GeometrySweep, VariantSweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "raftx_statics.h")
HIP_LIB = os.path.join(ROOT, "raft_amd", "csrc", "libraftx_hip.so")
ORACLE = os.path.join(ROOT, "oracle", "libraftx_oracle.so")


def test_prototype_is_in_the_statics_header():
    text = open(HEADER).read()
    protos = set(re.findall(r"^int\s+(raftx_\w+)\s*\(", text, re.M))
    assert protos == set(STATICS_EXPORTS) == {"raftx_mean_pose", "raftx_sweep_mean_pose"}
    assert "raftx_sweep_mean_pose" not in EXPORTS                      # the device library only: not raftx.h's contract
    m = re.search(r"^int\s+raftx_sweep_mean_pose\s*\(([^;]*)\);", text, re.M | re.S)
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert len(args) == 14 and args[0].startswith("raftx_ctx") and args[1] == "int slot"
    assert [a.split()[-1].lstrip("*").split("[")[0] for a in args[2:]] == [
        "nLine", "lines", "nX", "C_extra", "F_extra", "F_env", "tol", "max_iter", "pose", "F_res", "iterations", "flags"]
    assert "feeding the pose into a sweep crossing" not in text       # the "not covered" list is up to date


def test_symbol_is_exported_and_bound(oracle_lib):
    lib = RaftxLib(HIP_LIB)                                            # loads without a GPU
    assert lib.has_statics
    fn = lib.lib.raftx_sweep_mean_pose
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 14
    assert fn.argtypes[1] is ctypes.c_int and fn.argtypes[2] is ctypes.c_int and fn.argtypes[4] is ctypes.c_int
    assert fn.argtypes[9] is ctypes.c_int
    assert not oracle_lib.has_statics                                  # the oracle has no solver: the request is refused there


class FakeCtx:
    """Stands in for a context: records what would reach the library."""

    def __init__(self):
        self.calls, self.cancelled = [], 0
        self._mprog_owner = None

    def sweep_mean_pose(self, handle, **kw):
        self.calls.append(("mean_pose", kw))
        return handle

    def sweep_mooring(self, handle, **kw):
        self.calls.append(("mooring", kw))
        return handle

    def sweep_cancel(self, handle):
        self.cancelled += 1

    def mooring_program(self, prog):
        self._mprog_owner = prog


def plain_sweep(n=5):
    z = np.zeros((n, 6, 6))
    s = GeometrySweep.__new__(GeometrySweep)
    s.M0 = s.B0 = s.C0 = z
    return s


def test_dict_validation():
    s, ctx, lines = plain_sweep(), FakeCtx(), np.zeros((5, 3, 16))
    for bad in (dict(lines=lines, thrust=1.0), dict(), dict(lines=lines, program=object()), dict(C_extra=np.eye(6))):
        with pytest.raises(ValueError, match=r"mean_pose=dict\(lines= \| program="):
            s._with_mean_pose(ctx, "h", bad)
    assert ctx.cancelled == 4 and not ctx.calls                        # the prepared crossing is retired, nothing was asked
    assert s._with_mean_pose(ctx, "h", None) == "h" and not ctx.calls  # no request: nothing
    prog = object()
    s._with_mean_pose(ctx, "h", dict(program=prog, F_env=np.ones((5, 6)), tol=(1e-6, 1e-7), max_iter=7))
    assert ctx._mprog_owner is prog
    kind, kw = ctx.calls[-1]
    assert kind == "mean_pose" and kw["lines"] is None and kw["max_iter"] == 7 and kw["tol"] == (1e-6, 1e-7)
    assert kw["C_extra"] is None and kw["F_extra"] is None and kw["F_env"].shape == (5, 6)
    # the standing request is used when the argument is None, and the pose request goes ahead of the mooring request
    s.mean_pose = dict(lines=lines)
    s.mooring = dict(lines=lines)
    ctx.calls.clear()
    s._with_mooring(ctx, s._with_mean_pose(ctx, "h", None), None)
    assert [c[0] for c in ctx.calls] == ["mean_pose", "mooring"]
    for cls in (GeometrySweep, VariantSweep):
        import inspect
        for name in ("prepare_crossing", "submit_crossing", "run_crossing"):
            assert "mean_pose" in inspect.signature(getattr(cls, name)).parameters, (cls.__name__, name)
        src = inspect.getsource(cls.prepare_crossing)
        assert src.index("_with_mooring(") < src.index("_with_mean_pose(")         # nested: the inner call runs first


def test_take_slices_a_standing_request():
    from tests.test_abi_and_sharding import _variant_sweep
    s, _ = _variant_sweep(6)
    n = s.n_design
    lines = np.arange(n * 3 * 16, dtype=float).reshape(n, 3, 16)
    F_env = np.arange(n * 6, dtype=float).reshape(n, 6)
    Cx, Fx = np.arange(36.0).reshape(6, 6), np.arange(6.0)
    s.mean_pose = dict(lines=lines, F_env=F_env, C_extra=Cx, F_extra=Fx, max_iter=9)
    sub = s.take(2, 5)
    assert sub.n_design == 3 and sub.mean_pose is not s.mean_pose
    assert np.array_equal(sub.mean_pose["lines"], lines[2:5]) and np.array_equal(sub.mean_pose["F_env"], F_env[2:5])
    assert sub.mean_pose["C_extra"] is Cx and sub.mean_pose["F_extra"] is Fx and sub.mean_pose["max_iter"] == 9   # shared: as they are
    s.mean_pose = dict(program="P", C_extra=np.repeat(Cx[None], n, 0), F_extra=np.repeat(Fx[None], n, 0) * np.arange(n)[:, None])
    sub = s.take(1, 3)
    assert sub.mean_pose["program"] == "P" and sub.mean_pose["C_extra"].shape == (2, 6, 6)
    assert np.array_equal(sub.mean_pose["F_extra"], s.mean_pose["F_extra"][1:3])
    s.mean_pose = dict(lines=lines, thrust=3.0)
    with pytest.raises(ValueError, match="mean_pose=dict"):
        s.take(0, 2)
    s.mean_pose = None
    assert s.take(0, 2).mean_pose is None
