"""Quasi-static mooring lines on the device (include/raftx_mooring.h) through the C-ABI: raftx_mooring_lines on every
batch of tests/mooring_cases.py against the longdouble evaluation of tests/mooring_reference.py under the gate
|x - ref| <= C eps Ek of DESIGN.md section 4 (C = 16, from the fp64 model on the CPU, whose worst is 2.34; worst measured on the
MI355X 1.68; every batch prints its own), launch shapes, flags, the mooring program, and the errors raised before any launch."""
import json

import numpy as np
import pytest

from raft_amd import geometry as G
from raft_amd import snapshot as standin
from raft_amd._abi import RaftxError
from raft_amd.mooring import MooringProgram
from tests import mooring_cases as mc
from tests import mooring_reference as mr

pytestmark = pytest.mark.gpu
KEYS = ("C", "F", "T", "J", "line_out", "flags")
WORKGROUP = 256            # MOOR_THREADS of raft_amd/csrc/raftx_mooring.h


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def gate(res, ref, what):
    w = mc.worst_multiples(res, ref)
    print("%-36s kappa %.3g  worst multiples of eps Ek: %s" % (what, ref["kappa"].max(), {k: round(v, 2) for k, v in w.items()}))
    assert max(w.values()) <= mr.GATE_C, (what, w)
    return max(w.values())


def test_cases_against_the_reference(hip_ctx):
    worst = 0.0
    for name, lines, pose, depth in mc.batches():
        ref = mc.reference()[name]
        res = hip_ctx.mooring_lines(lines, depth, pose=pose)
        assert np.array_equal(res["flags"], ref["flags"]) and not res["flags"].any(), name
        lo, lr = res["line_out"], np.asarray(ref["line_out"], dtype=float)
        assert np.array_equal(lo[..., 6], lr[..., 6]), name                                    # the branch
        assert np.all(lo[..., 5] >= 1) and np.all(lo[..., 5] < 60) and np.all(lo[..., 7] == 0), name
        k1 = 1 + ref["kappa"][..., None]
        a, b = lo[..., :5].copy(), lr[..., :5].copy()
        a[..., 4] *= lines[..., 8]                                                             # L_B w: a force, as HF, VF, HA, VA
        b[..., 4] *= lines[..., 8]
        E = np.abs(lr[..., :2]).max(axis=-1) + lines[..., 8] * lines[..., 6]                   # max(HF, |VF|) + w L
        m = np.abs(a - b) / (mr.EPS * k1 * E[..., None])
        assert m.max() <= mr.GATE_C, (name, float(m.max()))
        worst = max(worst, gate(res, ref, name))
    print("worst multiple over all batches: %.3g (gate %d)" % (worst, mr.GATE_C))


def test_null_pose_is_the_zero_pose(hip_ctx):
    g = mc.golden()["OC3spar"]
    lines = np.broadcast_to(g["lines"], (5,) + g["lines"].shape).copy()
    a = hip_ctx.mooring_lines(lines, g["depth"], pose=None)
    b = hip_ctx.mooring_lines(lines, g["depth"], pose=np.zeros((5, 6)))
    assert all(same_bits(a[k], b[k]) for k in KEYS)
    assert not a["flags"].any()


def _mixed_lines(n_design, n_line):
    """n_design designs of n_line lines drawn from the single-line cases of depth 200 and the VolturnUS-S deck."""
    pool = [rec for name, (rec, depth) in mc.single_lines().items() if depth == 200.0 and not name.startswith("boundary")]
    pool += list(mc.golden()["VolturnUS-S"]["lines"])
    idx = (np.arange(n_design)[:, None] * 3 + np.arange(n_line)[None, :] * 5) % len(pool)
    return np.array(pool)[idx]


@pytest.mark.parametrize("n_line", [1, 2, 3])
def test_launch_shapes(hip_ctx, n_line):
    """(design x line) counts one below, at and one above the wave (64) and the workgroup (256), and design counts around
    them for the per-design kernel: every design's bits are those it has on its own."""
    counts = sorted({max(1, (c + d) // n_line) for c in (64, WORKGROUP) for d in (-1, 0, 1, n_line)} |
                    {c + d for c in (64, WORKGROUP) for d in (-1, 0, 1)})
    big = max(counts)
    lines = _mixed_lines(big, n_line)
    pose = np.tile(mc.POSES, (big // 4 + 1, 1))[:big]
    full = hip_ctx.mooring_lines(lines, 200.0, pose=pose)
    assert not full["flags"].any()
    ref = mr.evaluate(lines[:8], pose[:8], 200.0)
    gate({k: full[k][:8] for k in KEYS}, ref, "first designs of the largest launch, %d lines" % n_line)
    for n in counts:
        part = hip_ctx.mooring_lines(lines[:n], 200.0, pose=pose[:n])
        assert all(same_bits(part[k], full[k][:n]) for k in KEYS), (n, n_line)
    one = hip_ctx.mooring_lines(lines[big - 1:], 200.0, pose=pose[big - 1:])
    assert all(same_bits(one[k], full[k][big - 1:]) for k in KEYS)


def test_flags_poison_only_their_design(hip_ctx):
    n, mid = 9, 4
    lines = _mixed_lines(n, 3)
    pose = np.tile(mc.POSES, (3, 1))[:n]
    good = hip_ctx.mooring_lines(lines, 200.0, pose=pose)
    assert not good["flags"].any()

    def with_line(edit):
        bad = lines.copy()
        edit(bad[mid, 1])
        return bad

    def vertical(r):
        r[0:3], r[3:6], r[6] = [0.0, 0.0, -200.0], [0.0, 0.0, -14.0], 300.0

    def no_convergence(r):                       # a line 20 times heavier than it is stiff (w L = 7e5 N, EA = 577 N): the
        # damped iteration of the fp64 model breaks down on it (step factor below 2^-40) however many steps it is given
        r[0:3], r[3:6], r[6], r[7], r[8] = [-6.18136278, 0.0, -200.0], [0.0, 0.0, -141.946279], 58.4067875, 577.150747, 12060.5612

    cases = [(mr.FLAG_BAD_LINE, lambda r: r.__setitem__(7, np.nan)), (mr.FLAG_BAD_LINE, lambda r: r.__setitem__(6, 0.0)),
             (mr.FLAG_BAD_LINE, lambda r: r.__setitem__(8, -1.0)), (mr.FLAG_BAD_LINE, lambda r: r.__setitem__(2, -200.1)),
             (mr.FLAG_BAD_LINE, lambda r: r.__setitem__(5, -260.0)), (mr.FLAG_VERTICAL, vertical),
             (mr.FLAG_SLACK, lambda r: r.__setitem__(6, 5000.0)), (mr.FLAG_NO_CONVERGENCE, no_convergence)]
    for flag, edit in cases:
        res = hip_ctx.mooring_lines(with_line(edit), 200.0, pose=pose)
        want = np.zeros(n, dtype=np.int32)
        want[mid] = flag
        assert np.array_equal(res["flags"], want), (flag, res["flags"])
        keep = np.arange(n) != mid
        for k in ("C", "F", "T", "J", "line_out"):
            assert np.all(np.isnan(res[k][mid])), (flag, k)
            assert same_bits(res[k][keep], good[k][keep]), (flag, k)
    # a bad pose is a bad line of that design
    p = pose.copy()
    p[mid, 4] = np.inf
    res = hip_ctx.mooring_lines(lines, 200.0, pose=p)
    assert res["flags"][mid] == mr.FLAG_BAD_LINE and res["flags"].sum() == mr.FLAG_BAD_LINE
    assert same_bits(res["C"][np.arange(n) != mid], good["C"][np.arange(n) != mid])


def test_wild_records_converge_or_say_so(hip_ctx):
    """Records far outside the physical range (EA from 100 N, lines half as long as their chord): whatever the solver does
    on them -- converge or give up -- it must say so: finite outputs with flag 0, or NaN with its flag, and the
    neighbours' bits unchanged."""
    rng = np.random.default_rng(11)
    n = 64
    lines = _mixed_lines(n, 1)
    good = hip_ctx.mooring_lines(lines, 200.0)
    wild = lines.copy()
    odd = np.arange(1, n, 2)
    wild[odd, 0, 7] = 10.0 ** rng.uniform(2, 14, len(odd))                  # EA
    wild[odd, 0, 8] = 10.0 ** rng.uniform(-3, 5, len(odd))                  # w
    wild[odd, 0, 6] *= rng.uniform(0.5, 1.2, len(odd))                      # L, from far shorter than the chord
    res = hip_ctx.mooring_lines(wild, 200.0)
    assert np.all(np.isin(res["flags"], [0, mr.FLAG_SLACK, mr.FLAG_NO_CONVERGENCE]))
    ok = res["flags"] == 0
    assert np.all(np.isfinite(res["C"][ok])) and np.all(np.isnan(res["C"][~ok]))
    assert same_bits(res["C"][::2], good["C"][::2]) and same_bits(res["J"][::2], good["J"][::2])
    print("wild records: %d solved, %d slack, %d not converged; most steps %d" % (
        ok.sum(), (res["flags"] == mr.FLAG_SLACK).sum(), (res["flags"] == mr.FLAG_NO_CONVERGENCE).sum(), np.nanmax(res["line_out"][..., 5])))


def test_optional_outputs(hip_ctx):
    g = mc.golden()["VolturnUS-S"]
    lines = g["lines"][None]
    full = hip_ctx.mooring_lines(lines, g["depth"])
    for k in ("C", "F", "T", "J", "line_out"):
        part = hip_ctx.mooring_lines(lines, g["depth"], want=(k,))
        assert set(part) == {k, "flags"} and same_bits(part[k], full[k])
    only = hip_ctx.mooring_lines(lines, g["depth"], want=())
    assert set(only) == {"flags"} and only["flags"][0] == 0


def _programs():
    base = json.loads(standin.load_fixture("geom_units.npz")["c3_base_json"])
    moor = mc.golden()["VolturnUS-S"]["design"]
    return G.volturnus_program(base), G.volturnus_mooring_program(moor)


def test_mooring_expand_is_the_host_evaluation(hip_ctx):
    vp, mp = _programs()
    hip_ctx.variant_program(vp)
    hip_ctx.mooring_program(mp)
    for n in (1, 63, 257):
        params = G.volturnus_params(np.random.default_rng(n).uniform(0.75, 1.25, (n, 5)))
        assert same_bits(hip_ctx.mooring_expand(params), mp.expand(params))
    # a program with an unedited line and awkward coefficients
    rng = np.random.default_rng(2)
    q = MooringProgram(mp.lines, 5)
    q.ends(0, rng.normal(size=(3, 6)), rng.normal(size=(3, 6)))
    q.ends(2, rng.normal(size=(3, 6)) * 1e3, rng.normal(size=(3, 6)) * 1e-3)
    hip_ctx.mooring_program(q)
    params = rng.normal(size=(65, 5)) * 10
    got = hip_ctx.mooring_expand(params)
    assert same_bits(got, q.expand(params)) and same_bits(got[:, 1], np.broadcast_to(mp.lines[1], (65, 16)).copy())
    # the expanded records go straight into the stateless entry
    params = G.volturnus_params(np.random.default_rng(4).uniform(0.75, 1.25, (6, 5)))
    hip_ctx.mooring_program(mp)
    lines = hip_ctx.mooring_expand(params)
    res = hip_ctx.mooring_lines(lines, 200.0)
    gate(res, mr.evaluate(lines, None, 200.0), "six variants with the fairleads on the columns")
    hip_ctx.mooring_program(None)
    with pytest.raises(RaftxError, match="no program"):
        hip_ctx.mooring_expand(params)


def test_errors_before_any_launch(hip_ctx):
    g = mc.golden()["VolturnUS-S"]
    lines = g["lines"][None].copy()
    fr = lines.copy()
    fr[0, 1, 9] = 0.3
    with pytest.raises(RaftxError, match="CB = 0.3"):
        hip_ctx.mooring_lines(fr, g["depth"])
    with pytest.raises(RaftxError, match="depth"):
        hip_ctx.mooring_lines(lines, -1.0)
    with pytest.raises(RaftxError, match="depth"):
        hip_ctx.mooring_lines(lines, np.nan)
    with pytest.raises(RaftxError, match="nLine must be positive"):
        hip_ctx.mooring_lines(np.zeros((2, 0, 16)), 200.0)
    L = hip_ctx.rlib.lib
    flags = np.zeros(1, dtype=np.int32)
    ptr = lambda a: a.ctypes.data
    assert L.raftx_mooring_lines(hip_ctx._h, 1, 3, None, None, 200.0, None, None, None, None, None, ptr(flags)) != 0
    assert L.raftx_mooring_lines(hip_ctx._h, 1, 3, ptr(lines), None, 200.0, None, None, None, None, None, None) != 0
    assert b"required" in L.raftx_last_error(hip_ctx._h)
    assert hip_ctx.mooring_lines(np.zeros((0, 3, 16)), 200.0)["flags"].shape == (0,)
    # the program: needs the variant program, and its parameter count
    vp, mp = _programs()
    with pytest.raises(RaftxError, match="no variant program"):
        hip_ctx.mooring_program(mp)
    hip_ctx.variant_program(vp)
    with pytest.raises(RaftxError, match="nParam=4"):
        hip_ctx.mooring_program(MooringProgram(mp.lines, 4))
    bad = MooringProgram(mp.lines, 5)
    bad.lines[2, 9] = 1.0
    with pytest.raises(RaftxError, match="CB = 1"):
        hip_ctx.mooring_program(bad)
    with pytest.raises(RaftxError, match="no program"):
        hip_ctx.mooring_expand(np.zeros((1, 5)))
    hip_ctx.mooring_program(mp)
    assert L.raftx_mooring_expand(hip_ctx._h, 1, None, None) != 0
    with pytest.raises(ValueError):
        hip_ctx.mooring_expand(np.zeros((1, 4)))
    # raftx_sweep_mooring: an idle slot, a launched slot, NULL flags (the rest: tests/test_hip_sweep_mooring.py)
    from tests.test_hip_modal import _variant_sweep
    n_flags = np.zeros(4, dtype=np.int32)
    l4 = np.broadcast_to(g["lines"], (4, 3, 16)).copy()
    assert L.raftx_sweep_mooring(hip_ctx._h, 1, 3, ptr(l4), 1, None, None, None, None, ptr(n_flags)) != 0
    assert b"nothing prepared on slot 1" in L.raftx_last_error(hip_ctx._h)
    assert L.raftx_sweep_mooring(hip_ctx._h, 9, 3, ptr(l4), 1, None, None, None, None, ptr(n_flags)) != 0
    sw = _variant_sweep(4)
    h = sw.prepare_crossing(hip_ctx, 1)
    assert L.raftx_sweep_mooring(hip_ctx._h, 1, 3, ptr(l4), 1, None, None, None, None, None) != 0
    assert b"flags is required" in L.raftx_last_error(hip_ctx._h)
    sw.launch_crossing(hip_ctx, h)
    with pytest.raises(RaftxError, match="slot 1 has been launched"):
        hip_ctx.sweep_mooring(h, lines=l4)
    sw.wait_crossing(hip_ctx, h)
