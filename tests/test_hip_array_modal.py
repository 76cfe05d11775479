"""Eigen analysis of moored arrays on the device (include/raftx_array_modal.h): k_array_modal, one wavefront per system.

Against tests/golden/array_modal_reference.npz (mpmath at 50 digits) with the gate of tests/array_modal_cases.py:
|lambda - lambda_ref| <= G n eps ||A_b||_F / s_j, G = 4 max(1, g) = 4 with g = 0.516 LAPACK's own worst multiple over the
committed cases; fn to half the relative gate plus 2 eps; modes to 1 - |<v, v_ref>| <= 1e-9 where the relative gap is >= 1e-6,
clusters to a principal angle <= 1e-7; the DOF claim of the firm cases (lead >= 1e-3 in the golden) to the golden's claim.
Every kernel entry keeps the serial core's arithmetic, so nUnit = 1 returns the bits of raftx_modal_batch and a system's bits
do not depend on its place in the batch, the batch size or its neighbours.  Measured on the MI355X: every case uses at most
0.15 of its fn gate (lambda multiple <= 0.57 of G = 4), 1 - |<v, v_ref>| <= 3.4e-16 and cluster angles 0: the figures of the
serial core on the host, which the device reproduces bit for bit.
"""
import numpy as np
import pytest
from types import SimpleNamespace

from raft_amd import statics
from raft_amd._abi import MODAL_SMALL_DIAG
from tests import array_modal_cases as amc
from tests import array_mooring_cases as ac
from tests.test_modal import UNITS, unit_matrices

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64 if a.dtype == np.float64 else a.dtype),
                                                 b.view(np.uint64 if b.dtype == np.float64 else b.dtype))


def test_every_golden_case_meets_the_gate_at_several_positions(hip_ctx):
    gold = amc.golden()
    G = gold["G"]
    assert G == 4.0 * max(1.0, gold["g"])
    assert set(amc.FIRM + amc.LOOSE) <= set(gold["cases"])
    by_units = {}
    for name, rec in gold["cases"].items():
        by_units.setdefault(len(rec["M"]) // 6, []).append(name)
    assert sorted(by_units) == [1, 2, 3, 4, 5, 6]
    for nU, names in sorted(by_units.items()):
        order = names + names[::-1] + names[1:] + names[:1]            # every case at three places of the batch
        r = hip_ctx.array_modal_batch(np.array([gold["cases"][k]["M"] for k in order]), np.array([gold["cases"][k]["C"] for k in order]))
        assert not r["flags"].any(), (nU, r["flags"])
        first = {}
        for i, name in enumerate(order):
            if name not in first:
                first[name] = i
                amc.check_system(name, r["fn"][i], r["modes"][i], gold["cases"][name], G, firm=name in amc.FIRM)
            else:
                assert same_bits(r["fn"][i], r["fn"][first[name]]) and same_bits(r["modes"][i], r["modes"][first[name]]), (name, i)


def test_one_unit_returns_the_bits_of_raftx_modal_batch(hip_ctx):
    Ms, Cs = zip(*[unit_matrices(u) for u in UNITS])
    assert len(Ms) == 68
    Ms, Cs = np.array(Ms + (np.full((6, 6), np.nan),)), np.array(Cs + (Cs[0],))
    a, b = hip_ctx.array_modal_batch(Ms, Cs), hip_ctx.modal_batch(Ms, Cs)
    for k in ("fn", "modes", "flags"):
        assert same_bits(a[k], b[k]), k
    assert a["flags"][-1] & ~MODAL_SMALL_DIAG and np.all(np.isnan(a["fn"][-1]))


@pytest.mark.parametrize("nU", [2, 6])
def test_a_systems_bits_do_not_depend_on_its_place_or_its_neighbours(hip_ctx, nU):
    rec = amc.golden()["cases"]["synthetic%d" % nU]
    M0, C0 = np.asarray(rec["M"]), np.asarray(rec["C"])
    rng = np.random.default_rng(nU)
    pool_M = [M0 * (1 + 0.05 * k) for k in range(7)]
    pool_C = [C0 * (1 + 1e-3 * rng.uniform(-1, 1, size=C0.shape)) for _ in range(7)]
    alone = [hip_ctx.array_modal_batch(m[None], c[None]) for m, c in zip(pool_M, pool_C)]            # batches of 1
    assert not any(a["flags"][0] for a in alone)
    for n in (63, 64, 65, 130):
        idx = [(3 * i + 1) % 7 for i in range(n)]
        M, C = np.array([pool_M[k] for k in idx]), np.array([pool_C[k] for k in idx])
        M[n // 2] = np.nan                                                                               # a NaN system in the middle
        r = hip_ctx.array_modal_batch(M, C)
        for i in range(n):
            if i == n // 2:
                assert r["flags"][i] & ~MODAL_SMALL_DIAG and np.all(np.isnan(r["fn"][i])) and np.all(np.isnan(r["modes"][i]))
                continue
            for k in ("fn", "modes", "flags"):
                assert same_bits(r[k][i], alone[idx[i]][k][0]), (n, i, k)


@pytest.mark.parametrize("name, unit", [("synthetic2", 1), ("synthetic6", 4)])
def test_flags_at_12_and_36_dofs(hip_ctx, name, unit):
    gold = amc.golden()["cases"]
    M, C = np.asarray(gold[name]["M"]), np.asarray(gold[name]["C"])
    seeds = amc.flag_seeds(M, C, unit)
    Ms = np.array([M] + [s[0] for s in seeds.values()] + [M])
    Cs = np.array([C] + [s[1] for s in seeds.values()] + [C])
    r = hip_ctx.array_modal_batch(Ms, Cs)
    k = len(seeds)
    amc.check_flag_seeds(r["flags"][1:k + 1], r["fn"][1:k + 1], r["modes"][1:k + 1], list(seeds))
    clean = hip_ctx.array_modal_batch(M[None], C[None])
    for i in (0, -1):                                                    # the others are untouched
        assert r["flags"][i] == 0
        assert same_bits(r["fn"][i], clean["fn"][0]) and same_bits(r["modes"][i], clean["modes"][0])


def test_twins_and_uncoupled_pair_are_unflagged(hip_ctx):
    gold = amc.golden()
    for name in ("twins", "uncoupled_pair"):
        rec = gold["cases"][name]
        r = hip_ctx.array_modal_batch(rec["M"][None], rec["C"][None])
        assert r["flags"][0] == 0, name
        amc.check_system(name, r["fn"][0], r["modes"][0], rec, gold["G"], firm=name in amc.FIRM)


def test_errors_are_raised_before_any_launch(hip_ctx):
    from raft_amd._abi import RaftxError
    with pytest.raises(RaftxError, match="nUnit must be 1 to 6"):
        hip_ctx.array_modal_batch(np.eye(42)[None] * 1e6, np.eye(42)[None] * 1e5)
    c = ac.cases()["pair"]
    Mv = unit_matrices([u for u in UNITS if u["name"] == "VolturnUS-S"][0])[0]
    lines = c["lines"][None].copy()
    lines[0, 0, 11] = 5.0                                               # a unit index out of range: the array entry's line error
    with pytest.raises(RaftxError, match="unit B"):
        hip_ctx.array_modal_moored(np.broadcast_to(Mv, (1, 2, 6, 6)), c["K_hs"][None], lines, c["x_ref"][None], ac.DEPTH)


# ------------------------------------------------------------------ the moored entry
def _moored_inputs(name):
    c = ac.cases()[name]
    nU = len(c["K_hs"])
    Mv = unit_matrices([u for u in UNITS if u["name"] == "VolturnUS-S"][0])[0]
    pose = np.asarray(ac.reference(name)["x"], dtype=np.float64).reshape(nU, 6)
    return c, np.ascontiguousarray(np.broadcast_to(Mv, (nU, 6, 6))), pose


def _blockdiag(blocks):
    n = 6 * len(blocks)
    out = np.zeros((n, n))
    for u, b in enumerate(blocks):
        out[6 * u:6 * u + 6, 6 * u:6 * u + 6] = b
    return out


@pytest.mark.parametrize("name", ["pair", "row3", "ring6"])
def test_moored_entry_composes_the_line_kernels_and_the_eigen_kernel(hip_ctx, name):
    c, M_unit, pose = _moored_inputs(name)
    r = hip_ctx.array_modal_moored(M_unit[None], c["K_hs"][None], c["lines"][None], pose[None], ac.DEPTH)
    assert r["moor_flags"][0] == 0 and r["flags"][0] == 0
    moor = hip_ctx.array_mooring_lines(c["lines"][None], pose[None], ac.DEPTH, want=("C",))
    C_tot = _blockdiag(c["K_hs"]) + moor["C"][0]
    assert same_bits(r["C"][0], C_tot)
    b = hip_ctx.array_modal_batch(_blockdiag(M_unit)[None], C_tot[None])
    for k in ("fn", "modes", "flags"):
        assert same_bits(r[k], b[k]), k
    dC = np.zeros_like(C_tot)
    dC[5, 5] = 1e7
    r2 = hip_ctx.array_modal_moored(M_unit[None], c["K_hs"][None], c["lines"][None], pose[None], ac.DEPTH, dC=dC[None])
    assert same_bits(r2["C"][0], C_tot + dC)
    m = statics.array_modes(hip_ctx, M_unit[None], c["K_hs"][None], c["lines"][None], pose[None], ac.DEPTH)
    assert same_bits(m.fn, r["fn"]) and same_bits(m.modes, r["modes"]) and same_bits(m.C, r["C"])
    assert np.array_equal(m.periods, 1.0 / r["fn"]) and m.ok.all() and m.describe_flags(0) == []


def test_a_grounded_array_in_the_batch_flags_only_itself(hip_ctx):
    c, M_unit, pose = _moored_inputs("pair")
    g = ac.cases()["pair_grounded"]
    near = pose.copy()
    near[0, 0] += 40.0                                                  # 1500 m of chain over a 1404 m span: the sag passes the seabed
    near[1, 0] -= 40.0
    lines = np.array([c["lines"], g["lines"], c["lines"]])
    poses = np.array([pose, near, pose])
    Mu, Ku = np.array([M_unit] * 3), np.array([c["K_hs"], g["K_hs"], c["K_hs"]])
    r = hip_ctx.array_modal_moored(Mu, Ku, lines, poses, ac.DEPTH)
    moor = hip_ctx.array_mooring_lines(lines, poses, ac.DEPTH, want=("C",))
    assert np.array_equal(r["moor_flags"], moor["flags"]) and r["moor_flags"][1] & 64 and not r["moor_flags"][[0, 2]].any()
    assert r["flags"].tolist() == [0, 0, 0]
    assert np.all(np.isnan(r["fn"][1])) and np.all(np.isnan(r["modes"][1])) and np.all(np.isnan(r["C"][1]))
    alone = hip_ctx.array_modal_moored(Mu[:1], Ku[:1], lines[:1], poses[:1], ac.DEPTH)
    for i in (0, 2):
        for k in ("fn", "modes", "C"):
            assert same_bits(r[k][i], alone[k][0]), (i, k)
    m = statics.array_modes(hip_ctx, Mu, Ku, lines, poses, ac.DEPTH)
    assert m.ok.tolist() == [True, False, True] and "line on or below the seabed" in m.describe_flags(1)


# ------------------------------------------------------------------ the drop-in
def test_dropin_arrays_on_a_two_unit_standin(hip_ctx):
    from raft_amd import dropin
    gold = amc.golden()
    rec = gold["cases"]["pair"]
    u = [x for x in UNITS if x["name"] == "VolturnUS-S"][0]
    Mu, Cu = unit_matrices(u)
    C_ms = np.asarray(rec["C"]) - _blockdiag([Cu, Cu])                  # what the array mooring system must add to land on the golden's C

    def fowt():
        return SimpleNamespace(nDOF=6, M_struc=u["M_struc"], A_hydro_morison=u["A_hydro_morison"],
                               A_BEM=np.asarray(u["A_BEM0"])[:, :, None] * np.ones(3), C_struc=u["C_struc"], C_hydro=u["C_hydro"],
                               C_moor=u["C_moor"], C_elast=u["C_elast"], yawstiff=u["yawstiff"], body=None)
    ms = SimpleNamespace(getCoupledStiffnessA=lambda lines_only=False: C_ms)
    model = SimpleNamespace(fowtList=[fowt(), fowt()], ms=ms, moorMod=0, results={})
    fns, modes = dropin.Engine(hip_ctx).solveEigen(model, arrays=True)
    assert model.results["eigen"]["frequencies"] is fns and model.results["eigen"]["modes"] is modes
    # (C_tot = blockdiag + C_ms may round once more than the golden's C: a relative eps per entry, which the gate's backward
    # error n eps ||A_b||_F allows for)
    amc.check_system("pair (drop-in)", fns, modes, rec, gold["G"], firm=True)
    r = hip_ctx.array_modal_batch(np.asarray(rec["M"])[None], (_blockdiag([Cu, Cu]) + C_ms)[None])
    assert same_bits(fns, r["fn"][0]) and same_bits(modes, r["modes"][0])
