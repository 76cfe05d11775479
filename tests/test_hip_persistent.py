"""The persistent form of the fused fixed point (raftx_kp_f<FLAGS>, raftx_kpg_f0) with workgroups that solve pair after pair.

The default grid holds a workgroup per pair for every batch the rest of the suite launches on the featured twins, so a
workgroup claims once, re-enters once, finds the list dry and leaves: solve_pair never runs on re-entered state.  Here the
battery of tests/persistent_battery.py -- (a) all twelve twins on 27 heterogeneous pairs with a NaN pair among them, (b) the
claim edges nl = 1, 2, 7, 8, 9, 17, (c) 131 consecutive launches through the 64 counter sets, (d) the generating form on
64 designs -- runs with RAFTX_KP_GRID = 1, 3, 8, 13, with the default grid and with RAFTX_PERSIST=0.  The variables are read
once per process: every setting is a child process of its own, one at a time, which asserts through
raftx_last_solve_launch / raftx_last_solve_kernel that it ran the form, the grid and the specialisation it was asked for.
Every checked launch of (a) and (b) follows one of the same batch with tripled wave amplitudes on the same context: a
pair that is never claimed shows those numbers.

Asserted: every setting against the oracle (niter and flags equal, group_rel_err(Xi) < TOL per design, B_drag and F_wave
to TOL; tests/test_persistent_reference.py shows that this comparison rejects a pair never claimed, a leaked XiLast, a
carried NaN flag, swapped sea states and a count off by one); the persistent settings among each other bit for bit (the
same machine code on another schedule); persistent against per-pair launches (separate template instantiations): niter and
flags equal and, measured on an MI355X on every batch of (a) and (b), every output bit for bit the same -- the largest
group_rel_err(Xi) between the two forms is 0 -- so bit equality is asserted there too.

If a child ends by a signal or at its time limit the remaining cases fail at once and start no further process."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import persistent_battery as pb

pytestmark = pytest.mark.gpu
ROOT = pb.ROOT
CHILD = "import sys; sys.path.insert(0, %r); from tests import persistent_battery as pb; pb.child_%%s(sys.argv[1])" % ROOT
# setting -> what the child's environment adds (the variables of the other settings are taken out)
SETTINGS = {
    "grid1": {"RAFTX_KP_GRID": "1"}, "grid3": {"RAFTX_KP_GRID": "3"}, "grid8": {"RAFTX_KP_GRID": "8"},
    "grid13": {"RAFTX_KP_GRID": "13"}, "default": {}, "per_pair": {"RAFTX_PERSIST": "0"},
}
PERSISTENT = [s for s in SETTINGS if s != "per_pair"]
_RUNS = {}            # (kind, setting, fused generation) -> arrays of the child
_FAILED = {}          # the same key -> the end of the output of a child that failed: it is not started again
_DEAD = []            # why no further child is started
DEVICE_FAULTS = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "hipErrorLaunchFailure", "unspecified launch failure")


def child(kind, setting, tmp_path_factory, fused_gen=None):
    key = (kind, setting, fused_gen)
    if key in _RUNS:
        return _RUNS[key]
    if key in _FAILED:
        pytest.fail("the child of %s failed before: %s" % (key, _FAILED[key]))
    if _DEAD:
        pytest.fail("no further child process: " + _DEAD[0])
    env = dict(os.environ)
    for name in ("RAFTX_KP_GRID", "RAFTX_PERSIST", "RAFTX_FUSED_GEN", "RAFTX_FORCE_ALL", "RAFTX_SHAPE"):
        env.pop(name, None)
    env.update(SETTINGS[setting])
    if fused_gen is not None:
        env["RAFTX_FUSED_GEN"] = fused_gen
    path = str(tmp_path_factory.mktemp("persistent") / ("%s_%s_%s.npz" % (kind, setting, fused_gen)))
    try:
        p = subprocess.run([sys.executable, "-c", CHILD % kind, path], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _DEAD.append("the child of %s ran into its time limit" % (key,))
        pytest.fail(_DEAD[0])
    if p.returncode < 0 or (p.returncode and any(w in p.stdout + p.stderr for w in DEVICE_FAULTS)):
        _DEAD.append("the child of %s ended by a signal or a device fault (exit status %d): %s" % (key, p.returncode, p.stderr[-1500:]))
        pytest.fail(_DEAD[0])
    if p.returncode:
        _FAILED[key] = (p.stdout + p.stderr)[-3000:]
        pytest.fail("%s: %s" % (key, _FAILED[key]))
    _RUNS[key] = dict(np.load(path))
    return _RUNS[key]


def results(run, b, prefix=None):
    return {key: run["%s_%s" % (prefix or b.name, key)] for key in b.keys}


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_every_twin_and_claim_edge_against_the_oracle(setting, tmp_path_factory):
    run = child("main", setting, tmp_path_factory)
    batches = pb.all_batches()
    diag = run["diag"]                                   # [flags, persistent, grid, pairs] per checked launch, as the child saw it
    checked = batches + [pb.reuse_batch()[0]] * 2         # (c): the first launch of either set of sea states
    assert len(diag) == len(checked)
    g = int(SETTINGS[setting].get("RAFTX_KP_GRID", 0))
    worst = 0.0
    for b, (flags, persistent, grid, pairs) in zip(checked, diag.tolist()):
        assert flags == b.flags and pairs == b.pairs and persistent == (0 if setting == "per_pair" else 1)
        assert grid == (min(g, pb.grid_for_pairs(pairs)) if g else pb.grid_for_pairs(pairs)), (b.name, grid)
    for b in batches:
        covered, w = pb.compare_with_oracle(results(run, b), pb.oracle_reference(b.name), "%s %s" % (setting, b.name))
        assert covered.all()
        worst = max(worst, w)
    print("%s: %d launches held to the oracle, largest error %.3g; grids %s" % (
        setting, len(batches), worst, sorted(set(diag[:, 2].tolist()))))
    # (c) 2 x 64 + 3 launches through the 64 counter sets, two sets of sea states in turn: each the bits of its set's first
    assert run["c_differ"].size == 0, "launches %s differ from the first of their sea-state set" % run["c_differ"].tolist()
    c0, c1 = results(run, pb.reuse_batch()[0], "c0"), results(run, pb.reuse_batch()[0], "c1")
    assert pb.differing_keys(c0, c1, ("Xi",)) and int(c0["niter"].min()) >= 1


def test_the_persistent_settings_agree_bit_for_bit(tmp_path_factory):
    """Grids of 1, 3, 8 and 13 workgroups and the default grid: the same machine code on another schedule.  A condition,
    not a measurement."""
    base = child("main", PERSISTENT[0], tmp_path_factory)
    for setting in PERSISTENT[1:]:
        run = child("main", setting, tmp_path_factory)
        for b in pb.all_batches():
            assert not pb.differing_keys(results(run, b), results(base, b), b.keys), (setting, b.name)
        for pre in ("c0", "c1"):
            b = pb.reuse_batch()[0]
            assert not pb.differing_keys(results(run, b, pre), results(base, b, pre), b.keys), (setting, pre)


def test_persistent_and_per_pair_launches_agree(tmp_path_factory):
    """raftx_kp_f<FLAGS> and k_solve_dynamics<2, FLAGS, 128, 2> are separate instantiations of solve_pair; whether their
    bits agree is not known from the code.  Measured on an MI355X with every batch of (a) and (b): they do -- Xi, niter,
    flags, B_drag and F_wave of all twelve twins and all six claim edges are bit for bit the same in both forms (largest
    group_rel_err(Xi) between the forms: 0).  Asserted as bit equality since."""
    a, b_ = child("main", "grid1", tmp_path_factory), child("main", "per_pair", tmp_path_factory)
    worst, differ = 0.0, []
    for b in pb.all_batches():
        ra, rb = results(a, b), results(b_, b)
        assert np.array_equal(ra["niter"], rb["niter"]) and np.array_equal(ra["flags"], rb["flags"]), b.name
        worst = max(worst, pb.largest_group_rel_err(ra, rb))
        if pb.differing_keys(ra, rb, b.keys):
            differ.append(b.name)
    print("persistent against per-pair launches: largest group_rel_err(Xi) %.3g; batches that differ in some bit: %s" % (worst, differ))
    assert not differ


@pytest.mark.parametrize("setting", ["grid1", "grid3"])
def test_the_generating_form_builds_design_after_design(setting, tmp_path_factory):
    """raftx_kpg_f0 (RAFTX_FUSED_GEN=1): one and three workgroups build and solve 7, 1 and 64 C3 variants, design after
    design; std, niter, flags, strip offsets (and the responses) bit for bit those of a process with the same grid that
    generates with the kernels of their own."""
    fused = child("gen", setting, tmp_path_factory, "1")          # (asserts itself that every block ran the fused form)
    plain = child("gen", setting, tmp_path_factory, "0")
    g = int(SETTINGS[setting]["RAFTX_KP_GRID"])
    for run in (fused, plain):
        assert run["diag"].tolist() == [[1, g, 64]]            # persistent, grid, pairs of the last block launched
    keys = [k for k in fused if k != "diag"]
    assert sorted(keys) == sorted(k for k in plain if k != "diag") and len(keys) == 15
    for k in keys:
        assert fused[k].shape == plain[k].shape and np.array_equal(fused[k].view(np.uint8), plain[k].view(np.uint8)), (setting, k)
