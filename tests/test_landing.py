"""The layouts of the page-locked landing areas of a sweep crossing (raft_amd/csrc/raftx_landing.h: statistics and eigen
analysis of a block, mooring and mean pose of a crossing) compiled by a plain host compiler with
-fsanitize=address,undefined into a stand-alone program (tests/csrc/landing_driver.cpp): over n, P in {0, 1, 2, 3, 7, 64, 65}
and nLine in {1, 3} every area is allocated with exactly the doubles its layout asks for, every region is filled with a
pattern of its own through the layout and read back; the offsets equal the formulas written out in the driver, the regions
are in order, disjoint and aligned to their type, the last one ends within the need, and the need is not above the figure
the areas were reserved with before the layouts existed.  No GPU and no HIP header are involved."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def landing_driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("landing")
    san = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-Wall", "-Wextra", "-Werror"]
    # the sanitizer runtimes are probed with a trivial program: only their absence skips, and whatever the compiler then
    # says about the driver or the header is an error
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(san + ["-o", str(tmp / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("sanitizer runtimes not installed: " + r.stderr[-300:])
    exe = str(tmp / "landing_san")
    r = subprocess.run(san + ["-o", exe, os.path.join(ROOT, "tests", "csrc", "landing_driver.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_landing_layouts_hold_their_offsets_and_fit_their_need_under_address_and_undefined_behaviour_sanitizers(landing_driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([landing_driver], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.startswith("OK ") and int(r.stdout.split()[1]) > 1000
