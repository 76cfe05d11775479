"""The resource owners of the device library (raft_amd/csrc/raftx_owned.h: DevPool, Bag, Staging, DevBuf, Pinned, Event,
Stream) compiled by a plain host compiler with -fsanitize=address,undefined into a stand-alone program
(tests/csrc/owned_driver.cpp) whose HIP entry points are malloc-backed stand-ins that count live objects and fail on
demand: every owner leaves nothing behind, a failed growth leaves an empty buffer, bags return their blocks to the pool
and the pool frees each block once, moved-from owners release nothing, a borrowed stream is never destroyed; the arrays
of one call (Staging) are copied in declaration order with exact byte counts, results only by fetch, nothing for a null
or empty array, and a refused block sets the flag and leaves every other block to the pool.  No GPU and no HIP runtime
are involved."""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hip_include():
    roots = [os.environ.get("ROCM_PATH"), os.environ.get("HIP_PATH"), "/opt/rocm"] + sorted(glob.glob("/opt/rocm-*"), reverse=True)
    hipcc = shutil.which("hipcc")
    if hipcc:
        roots.append(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))))
    for r in roots:
        if r and os.path.exists(os.path.join(r, "include", "hip", "hip_runtime_api.h")):
            return os.path.join(r, "include")
    return None


@pytest.fixture(scope="module")
def owned_driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    inc = _hip_include()
    if inc is None:
        pytest.skip("no HIP headers")
    tmp = tmp_path_factory.mktemp("owned")
    san = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    # the sanitizer runtimes are probed with a trivial program: only their absence skips, and whatever the compiler then
    # says about the driver or the header is an error
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(san + ["-o", str(tmp / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("sanitizer runtimes not installed: " + r.stderr[-300:])
    exe = str(tmp / "owned_san")
    r = subprocess.run(san + ["-D__HIP_PLATFORM_AMD__", "-I" + inc, "-o", exe, os.path.join(ROOT, "tests", "csrc", "owned_driver.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_owners_release_everything_once_under_address_and_undefined_behaviour_sanitizers(owned_driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([owned_driver], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.startswith("OK ") and int(r.stdout.split()[1]) > 190
