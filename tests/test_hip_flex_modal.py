"""Eigen analysis of units with flexible members on the device (include/raftx_flex_modal.h): k_flex_modal, one workgroup of
256 threads per system, n at run time, H | X | Z in a global workspace per workgroup.

Against tests/golden/flex_modal_reference.npz (mpmath at 50 digits) under the gates of tests/flex_modal_cases.py; bit for bit
against the host driver tests/csrc/flex_modal_driver.cpp (built at test time: the test that catches a missing barrier or a
mis-owned lane) and, at 6, 12 and 36 DOFs, against k_array_modal in ascending order.  A system's bits do not depend on its place
in the batch, the batch size, its neighbours or the grid (RAFTX_FLEX_MODAL_GRID).
"""
import shutil

import numpy as np
import pytest

from raft_amd._abi import MODAL_SMALL_DIAG, RaftxError
from tests import array_modal_cases as amc
from tests import flex_modal_cases as fmc
from tests.test_flex_modal import build_driver, deck_standin, run_driver, seeded_batch, system_of
from tests.test_modal import UNITS, unit_matrices

pytestmark = pytest.mark.gpu

DEFAULT_GRID = 2 * 256                   # FLEX_MODAL_WG_PER_CU workgroups on each of the 256 CUs of an MI355X


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64 if a.dtype == np.float64 else a.dtype),
                                                 b.view(np.uint64 if b.dtype == np.float64 else b.dtype))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("the bit comparison needs g++ for the host driver")
    tmp = tmp_path_factory.mktemp("hip_flex_modal")
    return tmp, build_driver(tmp, "flex_modal_driver", ["-O2"])


def test_small_golden_cases_meet_the_gates_at_three_places(hip_ctx):
    for name in fmc.SYNTH:
        M, C = fmc.matrices(name)
        other = M * 1.25
        r = hip_ctx.flex_modal_batch(np.array([M, other, M, other, M]), np.array([C] * 5))
        assert not r["flags"].any(), (name, r["flags"])
        fmc.check_system(name, r["fn"][0], r["modes"][0], label="device")
        for i in (2, 4):
            assert same_bits(r["fn"][i], r["fn"][0]) and same_bits(r["modes"][i], r["modes"][0]), (name, i)


@pytest.mark.parametrize("name", ["deck150", "deck150_moor"])
def test_deck150_meets_the_gates_batched_three_times(hip_ctx, name):
    M, C = fmc.matrices(name)
    r = hip_ctx.flex_modal_batch(np.array([M] * 3), np.array([C] * 3))
    assert not r["flags"].any()
    fmc.check_system(name, r["fn"][0], r["modes"][0], label="device")
    for i in (1, 2):
        assert same_bits(r["fn"][i], r["fn"][0]) and same_bits(r["modes"][i], r["modes"][0]), i


def test_deck240_meets_the_gates(hip_ctx):
    M, C = fmc.matrices("deck240")
    r = hip_ctx.flex_modal_batch(M[None], C[None])
    assert r["flags"][0] == 0
    fmc.check_system("deck240", r["fn"][0], r["modes"][0], label="device")


def test_256_dofs_where_every_lane_owns_a_row(hip_ctx, host):
    tmp, exe = host
    M, C = system_of(256)
    r = hip_ctx.flex_modal_batch(M[None], C[None], n_modes=12)
    _, lanes, _, _ = run_driver(tmp, exe, M[None], C[None], n_modes=12)
    assert r["flags"][0] == 0
    assert same_bits(r["fn"], lanes["fn"]) and same_bits(r["modes"], lanes["modes"])
    fmc.check_against_numpy("synthetic n = 256", M, C, r["fn"][0])


@pytest.mark.parametrize("n", [7, 37, 65, 129, 150])
def test_device_returns_the_bits_of_the_host_driver(hip_ctx, host, n):
    tmp, exe = host
    M, C = system_of(n)
    Ms, Cs = np.array([M, M[::-1, ::-1]]), np.array([C, C[::-1, ::-1]])              # (the second one pivots in the LU of M)
    r = hip_ctx.flex_modal_batch(Ms, Cs)
    _, lanes, _, _ = run_driver(tmp, exe, Ms, Cs)
    assert not r["flags"].any() and same_bits(r["flags"], lanes["flags"])
    assert same_bits(r["fn"], lanes["fn"]), n
    assert same_bits(r["modes"], lanes["modes"]), n


def test_device_returns_the_bits_of_the_array_kernel_in_ascending_order(hip_ctx):
    gold = amc.golden()["cases"]
    units = [u for u in UNITS if not u["error"]]
    batches = {6: [unit_matrices(u) for u in units], 12: [(gold["synthetic2"]["M"], gold["synthetic2"]["C"])],
               36: [(gold["synthetic6"]["M"], gold["synthetic6"]["C"])]}
    for n, systems in batches.items():
        M, C = np.array([s[0] for s in systems], dtype=float), np.array([s[1] for s in systems], dtype=float)
        a, f = hip_ctx.array_modal_batch(M, C), hip_ctx.flex_modal_batch(M, C)
        assert same_bits(a["flags"], f["flags"]), n
        compared = 0
        for k in range(len(systems)):
            if a["flags"][k] & ~MODAL_SMALL_DIAG or len(np.unique(a["fn"][k])) < n:   # (exactly tied frequencies: no order to compare)
                continue
            fn, modes = fmc.ascending(a["fn"][k], a["modes"][k])
            assert same_bits(fn, f["fn"][k]) and same_bits(modes, f["modes"][k]), (n, k)
            compared += 1
        assert compared >= (60 if n == 6 else 1), (n, compared)


@pytest.mark.parametrize("n", [12, 65])
@pytest.mark.parametrize("grid", [5, None])
def test_a_systems_bits_do_not_depend_on_its_place_the_batch_or_the_grid(hip_ctx, monkeypatch, n, grid):
    monkeypatch.delenv("RAFTX_FLEX_MODAL_GRID", raising=False)
    M0, C0 = system_of(n)
    rng = np.random.default_rng(n)
    pool_M = [M0 * (1 + 0.05 * k) for k in range(7)]
    pool_C = [C0 * (1 + 1e-3 * rng.uniform(-1, 1, size=C0.shape)) for _ in range(7)]
    alone = [hip_ctx.flex_modal_batch(m[None], c[None], n_modes=4) for m, c in zip(pool_M, pool_C)]       # batches of 1
    assert not any(a["flags"][0] for a in alone)
    G = DEFAULT_GRID
    if grid is not None:
        monkeypatch.setenv("RAFTX_FLEX_MODAL_GRID", str(grid))
        G = grid
    for nS in (G - 1, G, G + 1, 2 * G + 3):
        idx = [(3 * i + 1) % 7 for i in range(nS)]
        M, C = np.array([pool_M[k] for k in idx]), np.array([pool_C[k] for k in idx])
        M[nS // 2] = np.nan                                                                                  # a NaN system in the middle
        r = hip_ctx.flex_modal_batch(M, C, n_modes=4)
        bad = nS // 2
        assert r["flags"][bad] & ~MODAL_SMALL_DIAG and np.all(np.isnan(r["fn"][bad])) and np.all(np.isnan(r["modes"][bad]))
        keep = np.arange(nS) != bad
        want = {k: np.array([alone[j][k][0] for j in idx]) for k in ("fn", "modes", "flags")}
        for k in ("fn", "modes", "flags"):
            assert same_bits(r[k][keep], want[k][keep]), (nS, k)


@pytest.mark.parametrize("n", [37, 150])
def test_flags_with_clean_systems_on_both_sides_untouched(hip_ctx, n):
    Ms, Cs, names = seeded_batch(n)
    keep = [k for k in range(len(Ms)) if k != len(names) + 1]                        # (the NaN system: the test above)
    Ms, Cs = Ms[keep], Cs[keep]
    r = hip_ctx.flex_modal_batch(Ms, Cs, n_modes=5)
    k = len(names)
    amc.check_flag_seeds(r["flags"][1:k + 1], r["fn"][1:k + 1], r["modes"][1:k + 1], names)
    clean = hip_ctx.flex_modal_batch(Ms[:1], Cs[:1], n_modes=5)
    for i in (0, -1):
        assert r["flags"][i] == 0
        assert same_bits(r["fn"][i], clean["fn"][0]) and same_bits(r["modes"][i], clean["modes"][0])


def test_results_do_not_depend_on_nmodes(hip_ctx):
    M, C = system_of(37)
    full = hip_ctx.flex_modal_batch(M[None], C[None])
    assert full["modes"].shape == (1, 37, 37) and full["flags"][0] == 0
    for m in (0, 3):
        r = hip_ctx.flex_modal_batch(M[None], C[None], n_modes=m)
        assert r["modes"].shape == (1, 37, m)
        assert same_bits(r["fn"], full["fn"]) and same_bits(r["modes"], full["modes"][:, :, :m]) and r["flags"][0] == 0, m


def test_errors_are_raised_before_any_launch(hip_ctx):
    for n, m, what in ((5, None, "n must be 6 to 256"), (257, None, "n must be 6 to 256"), (7, 8, "nModes must be 0 to n")):
        with pytest.raises(RaftxError, match=what):
            hip_ctx.flex_modal_batch(np.eye(n)[None] * 1e6, np.eye(n)[None] * 1e5, n_modes=m)
    with pytest.raises(RaftxError, match="nModes must be 0 to n"):
        hip_ctx.flex_modal_batch(np.eye(7)[None] * 1e6, np.eye(7)[None] * 1e5, n_modes=-1)
    r = hip_ctx.flex_modal_batch(np.zeros((0, 7, 7)), np.zeros((0, 7, 7)))
    assert r["fn"].shape == (0, 7) and r["modes"].shape == (0, 7, 7)


def test_flexsweep_natural_modes_and_the_dropin_on_the_deck(hip_ctx):
    from raft_amd import dropin
    from raft_amd.flex import FlexSweep, FlexUnit
    M, C = fmc.deck_matrices("flex_volturnus.npz")
    n = len(M)
    units = [FlexUnit([], np.zeros((0, 6, n)), M, np.zeros((n, n)), C * s) for s in (0.8, 1.25)]
    sweep = FlexSweep(units, np.linspace(0.1, 1, 4), np.linspace(0.01, 0.1, 4), 200.0, np.ones((1, 1, 4)), np.zeros((1, 1)), 5, 0.1)
    dM = np.zeros((n, n))
    dM[:6, :6] = np.diag([1e6, 1e6, 2e6, 3e8, 3e8, 1e8])
    out = sweep.natural_modes(hip_ctx, dM=dM)
    assert out["fn"].shape == (2, n) and out["modes"].shape == (2, n, 12) and not out["flags"].any()
    for k, u in enumerate(units):
        fmc.check_against_numpy("FlexSweep variant %d" % k, u.M + dM, u.C, out["fn"][k])
    fowt, model = deck_standin(yawstiff=4e7)
    fns, modes = dropin.Engine(hip_ctx).solveEigen(model, flexible=True)
    Mw = fowt.M_struc + fowt.A_hydro_morison + fowt.A_BEM[:, :, 0]
    Cw = fowt.C_struc + fowt.C_hydro + fowt.C_moor + fowt.C_elast
    Cw[5, 5] += fowt.yawstiff
    fmc.check_against_numpy("dropin.solveEigen", Mw, Cw, fns)
    assert modes.shape == (n, n) and model.results["eigen"]["frequencies"] is fns
    assert np.allclose(np.linalg.norm(modes, axis=0), 1.0, rtol=0, atol=1e-12)
