"""Lifetime of what a context owns (raft_amd/csrc/raftx_owned.h): buffers that regrow between solves, the requests of a
crossing on a slot that is used again, cancelled, or left prepared when the context is closed, and contexts created and
destroyed in a row.  Every comparison is bit for bit against a fresh context or the first run: none of this may show in
the results.  (Leaks are the business of tests/test_owned.py: free device memory of a shared card is not ours to assert.)"""
import numpy as np
import pytest

from tests.test_hip_modal import _variant_sweep
from tests.test_hip_sweep_channels import same_bits, shared_rows
from tests.test_hip_sweep_mooring import program
from tests.util import random_matrices, random_strips, synthetic_cases

pytestmark = pytest.mark.gpu
N = 3
REQUEST_KEYS = ("std", "niter", "flags", "Xi", "fn", "modes", "modal_flags", "D_hydro", "chan_std", "C_moor", "F_moor", "T_mean", "T_std",
                "moor_flags")


def solve(ctx, nw):
    """Two designs, one case, nw bins: std, niter, flags, Xi of the resident solve."""
    rng = np.random.default_rng(500 + nw)
    tables = [random_strips(rng, S) for S in (30, 17)]
    M0, B0, C0, _ = random_matrices(rng, 2)
    w, k, zeta, beta = synthetic_cases(rng, 1, 1, nw)
    ctx.upload_designs(tables, M0, B0, C0, nw)
    ctx.upload_cases(w, k, 200.0, 1025.0, 9.81, zeta, beta)
    out = ctx.solve_dynamics(6, tol=0.01, XiStart=0.1, want_Xi=True)
    sd, _ = ctx.motion_stats(w[1] - w[0])
    return {"std": sd, "niter": out["niter"], "flags": out["flags"], "Xi": out["Xi"]}


def test_buffers_regrown_between_solves(hip_ctx, hip_lib):
    """nw = 130, 200, 130 on one context: both take the 2 x 128 shape, whose XiLast lives in the global slab that grows with
    nw (and stays grown); the results are those of a context that has seen that size only."""
    for nw in (130, 200, 130):
        got = solve(hip_ctx, nw)
        fresh = hip_lib.context(0)
        try:
            want = solve(fresh, nw)
        finally:
            fresh.close()
        assert np.all(np.isfinite(got["std"])) and got["Xi"].shape[-1] == nw
        for key in want:
            assert same_bits(got[key], want[key]), (nw, key)


def requests():
    return dict(modal=True, current=dict(speed=[0.8, 1.3], heading=[0.0, 40.0]), channels=shared_rows(True), mooring=dict(program=program()))


def test_requests_on_a_reused_slot(hip_ctx, hip_lib):
    """All four requests on one slot, twice; then a prepared crossing with requests cancelled, and one left in the slot when
    the context is closed: the close returns and the next context works."""
    ctx = hip_lib.context(0)
    try:
        sw = _variant_sweep(N)
        first = sw.wait_crossing(ctx, sw.submit_crossing(ctx, 1, want_Xi=True, **requests()))
        assert all(key in first for key in REQUEST_KEYS) and np.all(np.isfinite(first["std"])) and not first["moor_flags"].any()
        again = sw.wait_crossing(ctx, sw.submit_crossing(ctx, 1, want_Xi=True, **requests()))
        for key in REQUEST_KEYS:
            assert same_bits(again[key], first[key]), key
        ctx.sweep_cancel(sw.prepare_crossing(ctx, 1, want_Xi=True, **requests()))
        plain = sw.wait_crossing(ctx, sw.submit_crossing(ctx, 1, want_Xi=True))       # the cancelled requests are gone
        assert "chan_std" not in plain and "C_moor" not in plain and "D_hydro" not in plain and "fn" not in plain
        left = sw.prepare_crossing(ctx, 1, want_Xi=True, **requests())              # kept alive: the caller's arrays of a prepared crossing
    finally:
        ctx.close()
    del left
    after = _variant_sweep(N)
    out = after.wait_crossing(hip_ctx, after.submit_crossing(hip_ctx, 1, want_Xi=True, **requests()))
    for key in REQUEST_KEYS:
        assert same_bits(out[key], first[key]), key


def test_create_and_destroy_in_a_row(hip_ctx, hip_lib):
    first = None
    for cycle in range(5):
        ctx = hip_lib.context(0)
        try:
            std = _variant_sweep(N).run_crossing(ctx)["std"]
        finally:
            ctx.close()
        assert np.all(np.isfinite(std))
        first = std if first is None else first
        assert same_bits(std, first), cycle
