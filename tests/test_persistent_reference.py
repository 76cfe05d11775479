"""CPU half of the persistent-kernel tests (tests/test_hip_persistent.py runs the battery of tests/persistent_battery.py on the
device): the conditions on the inputs, checked with the oracle alone so that a later change of seed cannot hollow the
device tests out, and the comparison itself run on oracle outputs with one seeded fault each -- every fault a workgroup
that solves pair after pair can produce must fail it."""
import numpy as np
import pytest

from raft_amd._abi import FLAG_CONVERGED, FLAG_NAN
from tests import persistent_battery as pb


def test_the_gate_is_the_parity_suite_s():
    from tests import test_hip_parity
    assert pb.TOL == test_hip_parity.TOL


def test_every_persistent_twin_has_a_batch():
    """RAFTX_PERSIST128 as raftx_kernels.h lists it: twelve flag sets, one batch of (a) each."""
    assert sorted(pb.persist128_flags()) == sorted(pb.TWINS) and len(pb.TWINS) == 12


def test_launch_header_is_separate_from_the_other_contracts():
    """include/raftx_launch.h declares raftx_last_solve_launch and nothing else; raftx.h, the contract the oracle implements
    too, does not."""
    import os
    import re
    from raft_amd import _abi
    inc = os.path.join(pb.ROOT, "include")
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, name)).read(), flags=re.S)
    assert set(re.findall(r"\b(raftx_[a-z_0-9]+)\s*\(", strip("raftx_launch.h"))) == set(_abi.LAUNCH_EXPORTS) == {"raftx_last_solve_launch"}
    for other in sorted(os.listdir(inc)):
        if other != "raftx_launch.h":
            assert "raftx_last_solve_launch" not in re.findall(r"\b(raftx_\w+)\s*\(", strip(other)), other
    assert not set(_abi.LAUNCH_EXPORTS) & set(_abi.EXPORTS)


def test_device_library_exports_the_launch_diagnostic():
    import ctypes
    from raft_amd._abi import RaftxLib
    from tests.conftest import HIP_SO
    assert hasattr(ctypes.CDLL(HIP_SO), "raftx_last_solve_launch") and RaftxLib(HIP_SO).has_launch


def test_oracle_binds_and_refuses_the_launch_diagnostic(oracle_ctx):
    """The oracle has no launches: it binds without the entry, and the call is refused there by name."""
    from raft_amd._abi import RaftxError
    assert not oracle_ctx.rlib.has_launch
    pb.run(oracle_ctx, pb.edge_batch(2), False)
    with pytest.raises(RaftxError, match="raftx_launch.h"):
        oracle_ctx.last_solve_launch()


def test_the_claim_edges_are_the_ones_meant():
    """27 pairs: per = 4, slab 6 holds three positions, slab 7 none; (b): nl < 8, nl = 8, nl no multiple of 8, empty slabs."""
    b = pb.twin_batch(0)
    per = (b.pairs + 7) // 8
    assert b.pairs == 27 and per == 4 and b.pairs - 6 * per == 3 and b.pairs - 7 * per < 0
    assert pb.EDGE_NL == (1, 2, 7, 8, 9, 17) and all(pb.edge_batch(n).pairs == n for n in pb.EDGE_NL)
    assert pb.REUSE_LAUNCHES == 2 * 64 + 3 and pb.reuse_batch()[0].pairs == 9


@pytest.mark.parametrize("flags", list(pb.TWINS))
def test_neighbouring_pairs_of_a_twin_batch_differ(flags):
    b = pb.twin_batch(flags)
    r = pb.oracle_reference(b.name)
    S = [t.n for t in b.tables]
    assert S[pb.NAN_D] == 0 and 0 in S[:pb.NAN_D] + S[pb.NAN_D + 1:] and 1 in S and len(set(S)) >= 6      # 0 (twice) and 1 strips among them
    amp = np.sort(np.abs(b.zeta).max(axis=(1, 2)))
    assert b.nC == 3 and np.all(amp[1:] > 10.0 * amp[:-1])                  # more than an order of magnitude apart
    assert b.nH == pb.TWINS[flags][2]
    # the singular design, NaN-flagged in every sea state, between two ordinary ones
    nan = (r["flags"] & FLAG_NAN) != 0
    assert nan[pb.NAN_D].all() and not np.delete(nan, pb.NAN_D, axis=0).any()
    assert not np.isfinite(r["Xi"][pb.NAN_D]).any()
    assert S[pb.NAN_D - 1] > 1 and S[pb.NAN_D + 1] > 1 and np.isfinite(r["Xi"][pb.NAN_D - 1]).all() and np.isfinite(r["Xi"][pb.NAN_D + 1]).all()
    # iteration counts: at least three distinct values, at least one pair unconverged at the cap
    cap = b.nIter + 1
    assert len(set(r["niter"].ravel().tolist())) >= 3 and int(r["niter"].max()) == cap
    at_cap = (r["niter"] == cap) & ((r["flags"] & (FLAG_CONVERGED | FLAG_NAN)) == 0)
    assert at_cap.any() and ((r["flags"] & FLAG_CONVERGED) != 0).any()
    # neighbours in the pair list differ in iteration count somewhere
    assert (np.diff(r["niter"].ravel()) != 0).sum() >= 6


@pytest.mark.parametrize("name", [b.name for b in pb.all_batches()])
def test_iteration_counts_are_firm(name):
    """The oracle gives the same niter and flags with the solver's tolerance scaled by 1 +- 1e-6: no pair sits on the edge of
    one more iteration, where the device's rounding could legitimately decide otherwise."""
    r = pb.oracle_reference(name)
    for scale in (1.0 - 1e-6, 1.0 + 1e-6):
        s = pb.oracle_reference(name, 1.0, scale)
        assert np.array_equal(r["niter"], s["niter"]) and np.array_equal(r["flags"], s["flags"]), (name, scale)


@pytest.mark.parametrize("name", [b.name for b in pb.all_batches()])
def test_no_pair_is_left_out_of_the_comparison(name):
    """The reference compared with itself (perturbed in the 13th digit): passes, and every pair took part -- numerically, or
    as a NaN pair on niter and flags."""
    r = pb.oracle_reference(name)
    got = {k: (v * (1.0 + 1e-13) if v.dtype.kind in "fc" else v.copy()) for k, v in r.items()}
    covered, worst = pb.compare_with_oracle(got, r, name)
    assert covered.shape == r["niter"].shape and covered.all() and 0.0 < worst < 1e-12
    assert not pb.differing_keys(r, {k: v.copy() for k, v in r.items()}, r.keys()) and pb.differing_keys(got, r, r.keys()) == ["Xi", "B_drag"] + (
        ["F_wave"] if "F_wave" in r else [])


# ------------------------------------------------------------------ seeded faults: the comparison must reject each
FAULT_TWINS = [0, pb.KF_OUTF | pb.KF_MULTI]       # the plain kernel; three headings with F_wave exported


def _copy(r):
    return {k: v.copy() for k, v in r.items()}


def _rejects(got, ref, what):
    with pytest.raises(AssertionError):
        pb.compare_with_oracle(got, ref, what)


def _ordinary_pair(r, after=0):
    """(d, c) of a pair with strips that is not NaN, from flat position `after` on"""
    nD, nC = r["niter"].shape
    for p in range(after, nD * nC):
        d, c = divmod(p, nC)
        if not (r["flags"][d, c] & FLAG_NAN) and np.abs(r["B_drag"][d, c]).max() > 0:
            return d, c
    raise AssertionError("no ordinary pair")


@pytest.mark.parametrize("flags", FAULT_TWINS)
def test_a_pair_never_claimed_is_rejected(flags):
    """The checked launch follows one with tripled amplitudes on the same context: a pair no workgroup claims keeps those
    results."""
    name = pb.twin_batch(flags).name
    r, r3 = pb.oracle_reference(name), pb.oracle_reference(name, 3.0)
    for after in (0, 11, 26 - 3):
        d, c = _ordinary_pair(r, after)
        got = _copy(r)
        for k in got:
            got[k][d, c] = r3[k][d, c]
        _rejects(got, r, "never claimed (%d, %d)" % (d, c))
        if r3["niter"][d, c] == r["niter"][d, c] and r3["flags"][d, c] == r["flags"][d, c]:     # the numbers alone give it away too
            got["niter"], got["flags"] = r["niter"], r["flags"]
            _rejects(got, r, "never claimed, same counts")


@pytest.mark.parametrize("flags", FAULT_TWINS)
def test_a_pair_started_from_its_predecessor_s_response_is_rejected(flags, oracle_lib):
    """XiLast not re-seeded: the pair starts its fixed point from the final response of the pair before it, not from XiStart
    (the oracle through set_linearisation_point)."""
    b = pb.twin_batch(flags)
    r = pb.oracle_reference(b.name)
    flat = r["Xi"].reshape((b.pairs,) + r["Xi"].shape[2:])
    for after in (2, 13):
        d, c = _ordinary_pair(r, after)
        p = d * b.nC + c
        pred = p - 1
        while r["flags"].ravel()[pred] & FLAG_NAN:
            pred -= 1
        X0 = np.full((b.nD, b.nC, 6, pb.NW), pb.XI_START, dtype=np.complex128)
        X0[d, c] = flat[pred][0]
        ctx = oracle_lib.context(0)
        try:
            pb.upload_designs(ctx, b)
            leak = pb.solve(ctx, b, XiLast0=X0)
        finally:
            ctx.close()
        for dd in range(b.nD):                                     # every other pair started from XiStart as always
            for cc in range(b.nC):
                if (dd, cc) != (d, c) and dd != pb.NAN_D:
                    assert np.array_equal(leak["Xi"][dd, cc], r["Xi"][dd, cc])
        got = _copy(r)
        for k in got:
            got[k][d, c] = leak[k][d, c]
        _rejects(got, r, "leaked XiLast (%d, %d)" % (d, c))
        got["niter"], got["flags"] = r["niter"], r["flags"]          # ... by its numbers, whatever the counts
        _rejects(got, r, "leaked XiLast, same counts")


@pytest.mark.parametrize("flags", FAULT_TWINS)
def test_a_nan_flag_carried_to_the_next_pair_is_rejected(flags):
    r = pb.oracle_reference(pb.twin_batch(flags).name)
    got = _copy(r)
    got["flags"][pb.NAN_D + 1, 0] |= FLAG_NAN                       # the pair after the last NaN pair
    _rejects(got, r, "NaN flag carried over")
    got = _copy(r)
    got["flags"][pb.NAN_D, 2] &= ~FLAG_NAN                          # and a NaN pair that lost its flag
    _rejects(got, r, "NaN flag lost")


@pytest.mark.parametrize("flags", FAULT_TWINS)
def test_two_pairs_swapped_between_sea_states_are_rejected(flags):
    r = pb.oracle_reference(pb.twin_batch(flags).name)
    for d, (c0, c1) in ((0, (0, 1)), (3, (1, 2)), (8, (0, 2))):
        got = _copy(r)
        for k in got:
            got[k][d, c0], got[k][d, c1] = r[k][d, c1], r[k][d, c0]
        _rejects(got, r, "swapped")
        got["niter"], got["flags"] = r["niter"], r["flags"]
        _rejects(got, r, "swapped, same counts")


@pytest.mark.parametrize("flags", FAULT_TWINS)
def test_an_iteration_count_off_by_one_is_rejected(flags):
    """... with responses within TOL: the counts are compared for equality, not through the responses."""
    r = pb.oracle_reference(pb.twin_batch(flags).name)
    for delta in (1, -1):
        got = _copy(r)
        got["niter"][4, 1] += delta
        _rejects(got, r, "niter off by one")
