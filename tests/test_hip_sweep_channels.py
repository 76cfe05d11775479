"""Output channels of a sweep crossing on the device (include/raftx_channels.h, k_sweep_channels).

Tolerance: the derived forward-error bound of tests/stats_reference.py (stats, poly_coef, used, bound_factors(6, nHead, nw)),
evaluated in longdouble on the responses the crossing itself returned (want_Xi=True), so it owes nothing to the solver.  The
kernel's arithmetic per term is that of k_channel_stats_poly, so the same bound holds; it is not tuned.  Two results that sit
within the bound of ONE reference differ by at most twice the bound: |std_a^2 - std_b^2| <= 2 Kv env_var.

The recorded reference (tests/golden/refgold_sweep_outputs.npz) is held to the gate of its CPU test
(tests/test_sweep_channels.py): 1e-8 x the key's largest value + 1e-12.

The design with non-finite responses: the all-zero, no-strip design of test_stats_reference._resident cannot be expressed
in a crossing (its designs are member descriptions, which generate strips), and a described design whose M0 = C0 = 0 is NOT
singular there -- the linearised drag of its strips alone gives a solvable system (flags 0 / 1, finite responses; measured on
the CPU oracle's crossing).  The design used instead carries NaN in its M_extra: flag 2 and non-finite responses in all its
pairs, which is the property under test."""
import numpy as np
import pytest

from raft_amd._abi import RaftxError
from raft_amd.sweep import GeometrySweep
from tests import stats_reference as R
from tests.test_geometry import C3, _c3_crossing_inputs
from tests.test_hip_modal import _variant_sweep
from tests.test_stats_reference import XI_FLOOR, W_MIN, _poly_rows
from tests.test_sweep_channels import KEYS, check_against_reference, fixture_rows, fixture_sweep
from tests.util import synthetic_cases

pytestmark = pytest.mark.gpu
N_D = 5
CUR = dict(speed=[2.0, 0.6], heading=[15.0, 400.0], Zref=-12.0, shearExp=0.2)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def c3_sweep(nw, nHead, M_extra=None):
    """Five C3 variants as member descriptions on two synthetic sea states."""
    D, M0, B0, C0 = _c3_crossing_inputs(N_D)
    depth = float(C3["depth"])
    w, k, zeta, beta = synthetic_cases(np.random.default_rng([nw, nHead]), 2, nHead, nw, depth=depth, wmin=W_MIN)
    return GeometrySweep(D, M0 if M_extra is None else M_extra, B0, C0, w, k, depth, zeta, beta, int(C3["nIter"]), float(C3["XiStart"]))


def rows(rng, nD, nChan, nw):
    """(L [nD,nChan,3,6], Gw [nD,nChan,6,nw]) from test_stats_reference._poly_rows: blocks of its four channels side by side;
    its three designs (rows 1, 1000 and 1e-3 times a common scale) carry on as designs 3, 4 = designs 0, 1 times 1e2 / 1e-2,
    so that no two designs share rows and a wrong design index is off by orders of magnitude."""
    blocks = [_poly_rows(rng, nw) for _ in range((nChan + 3) // 4)]
    L = np.concatenate([b[0] for b in blocks], axis=1)[:, :nChan]
    G = np.concatenate([b[1] for b in blocks], axis=1)[:, :nChan]
    pick, scale = np.arange(nD) % 3, np.where(np.arange(nD) < 3, 1.0, np.where(np.arange(nD) % 3 == 0, 1e2, 1e-2))
    return (np.ascontiguousarray(L[pick] * scale[:, None, None, None]), np.ascontiguousarray(G[pick] * scale[:, None, None, None]))


def reference(w, L, Gw, Xi):
    """Stats of the channels in longdouble on Xi [nD,nCase,nHead,6,nw]; L / Gw shared ([nChan,..]) or per design."""
    L, Gw = np.asarray(L), (None if Gw is None else np.asarray(Gw))
    if L.ndim == 3 and Gw is not None and Gw.ndim == 4:
        L = np.broadcast_to(L, (Gw.shape[0],) + L.shape)
    if Gw is not None and Gw.ndim == 3 and L.ndim == 4:
        Gw = np.broadcast_to(Gw, (L.shape[0],) + Gw.shape)
    coef = R.poly_coef(w, L, Gw)
    if coef.ndim == 4:
        coef = coef[:, None]                                  # [d,1,c,j,w] against Xi [d,case,h,j,w]
    return R.stats(coef, Xi, w[1] - w[0])


def within(ref, std, nHead, what, factor=1.0):
    _, f_var = R.used(ref, std, None, 6, nHead)
    print("%s: uses %.3g of the variance bound" % (what, f_var))
    assert f_var <= factor, (what, f_var)


def floor_ok(Xi):
    mag = np.abs(Xi[np.isfinite(Xi)])
    assert mag.size and mag.min() > XI_FLOOR, "a response so small that its square leaves fp64's normal range"


# ------------------------------------------------------------------ 1. shapes and forms against the bound
@pytest.mark.parametrize("nw,nHead", [(8, 3), (64, 1), (65, 1), (129, 3), (257, 1)])
def test_shapes_and_forms_within_the_bound(hip_ctx, nw, nHead):
    sw = c3_sweep(nw, nHead)
    Xi0 = None
    for nChan in (1, 8, 9, 19):
        L, G = rows(np.random.default_rng([7, nw, nHead, nChan]), N_D, nChan, nw)
        forms = [("shared L", L[0], None), ("per-design L and Gw", L, G)]
        if nChan == 9:
            forms += [("per-design L", L, None), ("shared L and Gw", L[0], G[0]), ("per-design L, shared Gw", L, G[2]),
                      ("shared L, per-design Gw", L[1], G)]
        for name, l, g in forms:
            out = sw.run_crossing(hip_ctx, want_Xi=True, channels=dict(L=l, Gw=g))
            assert out["chan_std"].shape == (N_D, 2, nChan) and not np.any(out["flags"] & 2)
            floor_ok(out["Xi"])
            if Xi0 is None:
                Xi0 = out["Xi"].copy()
            assert same_bits(out["Xi"], Xi0)                  # the request does not touch the solve
            within(reference(sw.w, l, g, out["Xi"]), out["chan_std"], nHead, "nw %d nHead %d nChan %d, %s" % (nw, nHead, nChan, name))


# ------------------------------------------------------------------ 2. the resident path
@pytest.mark.parametrize("nw,nHead", [(65, 1), (129, 3)])
def test_crossing_agrees_with_the_resident_path(hip_ctx, nw, nHead):
    sw = c3_sweep(nw, nHead)
    L, G = rows(np.random.default_rng([8, nw, nHead]), N_D, 9, nw)
    _, Kv = R.bound_factors(6, nHead, nw)
    for name, l, g in [("shared L", L[0], None), ("per-design L and Gw", L, G)]:
        a = sw.run_crossing(hip_ctx, want_Xi=True, channels=dict(L=l, Gw=g))
        sw.upload(hip_ctx)
        b = sw.run_channels(hip_ctx, l, Gw=g)
        assert same_bits(hip_ctx.fetch_results(want_Xi=True)["Xi"], a["Xi"])     # one set of responses, so one reference
        ref = reference(sw.w, l, g, a["Xi"])
        within(ref, a["chan_std"], nHead, "crossing, " + name)
        within(ref, b["std"], nHead, "resident, " + name)
        err = np.abs(a["chan_std"].astype(R.LD) ** 2 - b["std"].astype(R.LD) ** 2)
        assert np.all(err <= 2 * Kv * ref.env_var), (name, float(np.max(err / (Kv * ref.env_var))))


# ------------------------------------------------------------------ 3. bit identity
def shared_rows(with_G, nChan=10, nw=None, seed=9):
    nw = len(C3["w"]) if nw is None else nw
    L, G = rows(np.random.default_rng(seed), 3, nChan, nw)
    return dict(L=L[0], Gw=G[0] if with_G else None)


@pytest.mark.parametrize("with_G", [False, True])
def test_bits_do_not_depend_on_how_the_crossing_is_run(hip_ctx, with_G):
    n = 64
    sw = _variant_sweep(n)
    CH = shared_rows(with_G)
    base = sw.run_crossing(hip_ctx, n_chunk=1, channels=CH)
    ch = base["chan_std"]
    assert ch.shape == (n, 1, 10) and np.all(np.isfinite(ch)) and np.all(ch > 0)
    assert same_bits(sw.run_crossing(hip_ctx, n_chunk=3, channels=CH)["chan_std"], ch)
    with_xi = sw.run_crossing(hip_ctx, n_chunk=1, want_Xi=True, channels=CH)
    assert same_bits(with_xi["chan_std"], ch)
    within(reference(sw.w, CH["L"], CH["Gw"], with_xi["Xi"]), ch, 1, "64 C3 variants, ten shared rows")
    assert same_bits(sw.run_crossing(hip_ctx, n_chunk=3, want_Xi=True, channels=CH)["chan_std"], ch)
    assert same_bits(sw.run_crossing(hip_ctx, slot=2, channels=CH)["chan_std"], ch)
    # the same designs alone, and embedded in a batch of other designs
    assert same_bits(sw.take(0, 16).run_crossing(hip_ctx, channels=CH)["chan_std"], ch[:16])
    other = _variant_sweep(n, seed=5)
    params = other.params.copy()
    params[20:36] = sw.params[:16]
    other.set_params(params)
    assert same_bits(other.run_crossing(hip_ctx, n_chunk=2, channels=CH)["chan_std"][20:36], ch[:16])
    # whatever else rides along
    rest = sw.run_crossing(hip_ctx, n_chunk=3, modal=True, want_props=True, current=CUR)
    every = sw.run_crossing(hip_ctx, n_chunk=3, modal=True, want_props=True, current=CUR, channels=CH)
    assert same_bits(every["chan_std"], ch) and "chan_std" not in rest
    for k in ("std", "niter", "flags", "fn", "modes", "modal_flags", "props", "D_hydro"):
        assert same_bits(every[k], rest[k]), k
    plain = sw.run_crossing(hip_ctx, n_chunk=1)
    assert "chan_std" not in plain
    for k in ("std", "niter", "flags"):
        assert same_bits(plain[k], base[k]) and same_bits(plain[k], every[k]), k


# ------------------------------------------------------------------ 4. two slots in flight
def test_two_slots_in_flight_keep_their_own_rows(hip_ctx):
    n = 64
    sw = _variant_sweep(n)
    pA, pB = sw.params.copy(), _variant_sweep(n, seed=7).params.copy()
    CA, CB = shared_rows(False, nChan=10, seed=9), shared_rows(True, nChan=3, seed=10)
    alone = []
    for p, CH in ((pA, CA), (pB, CB)):
        sw.set_params(p)
        alone.append(sw.run_crossing(hip_ctx, channels=CH))
    sw.set_params(pA)
    hA = sw.prepare_crossing(hip_ctx, 0, channels=CA)
    sw.set_params(pB)
    hB = sw.prepare_crossing(hip_ctx, 1, channels=CB)
    sw.launch_crossing(hip_ctx, hA)
    sw.launch_crossing(hip_ctx, hB)
    outA, outB = sw.wait_crossing(hip_ctx, hA), sw.wait_crossing(hip_ctx, hB)
    assert outA["chan_std"].shape == (n, 1, 10) and outB["chan_std"].shape == (n, 1, 3)
    for out, ref in ((outA, alone[0]), (outB, alone[1])):
        for k in ("chan_std", "std", "niter", "flags"):
            assert same_bits(out[k], ref[k]), k
    assert not same_bits(outA["std"], outB["std"])


# ------------------------------------------------------------------ 5. the fused generation
def test_fused_generation_stays_on_with_channels(hip_ctx, monkeypatch):
    """The responses are resident in every block whichever kernel generated the tables: RAFTX_FUSED_GEN=1 keeps its route
    with channels requested and returns the bits of the default route."""
    sw = _variant_sweep(64)
    CH = shared_rows(True)
    ref = sw.run_crossing(hip_ctx, n_chunk=2, channels=CH)
    monkeypatch.setenv("RAFTX_FUSED_GEN", "1")
    out = sw.run_crossing(hip_ctx, n_chunk=2, channels=CH)
    assert out["generation_fused_blocks"][0] > 0
    for k in ("std", "niter", "flags", "chan_std"):
        assert same_bits(ref[k], out[k]), k


# ------------------------------------------------------------------ 6. a design with non-finite responses
def test_non_finite_pair_leaves_its_neighbours_alone(hip_ctx):
    nw, nHead, bad, good = 65, 3, 2, [0, 1, 3, 4]
    D, M0, B0, C0 = _c3_crossing_inputs(N_D)
    M_bad = M0.copy()
    M_bad[bad] = np.nan
    L, G = rows(np.random.default_rng(13), N_D, 9, nw)
    for name, l, g in [("shared L", L[0], None), ("per-design L and Gw", L, G)]:
        clean = c3_sweep(nw, nHead).run_crossing(hip_ctx, channels=dict(L=l, Gw=g))
        out = c3_sweep(nw, nHead, M_extra=M_bad).run_crossing(hip_ctx, want_Xi=True, channels=dict(L=l, Gw=g))
        assert np.all(out["flags"][bad] & 2) and not np.any(out["flags"][good] & 2), name
        assert not np.any(np.isfinite(out["Xi"][bad])) and np.all(np.isfinite(out["Xi"][good])), name
        assert not np.any(np.isfinite(out["chan_std"][bad])), name
        assert np.all(np.isfinite(out["chan_std"][good])) and same_bits(out["chan_std"][good], clean["chan_std"][good]), name
        lg = l[good] if l.ndim == 4 else l
        gg = None if g is None else g[good]
        within(reference(c3_sweep(nw, nHead).w, lg, gg, out["Xi"][good]), out["chan_std"][good], nHead,
               "next to a design with non-finite responses, " + name)


# ------------------------------------------------------------------ 7. slot errors, argument errors, cancel
def test_sweep_channels_on_idle_or_launched_slot_and_argument_errors(hip_ctx):
    n = 64
    sw = _variant_sweep(n)
    nw = sw.nw
    L = shared_rows(False)["L"]
    h = sw.prepare_crossing(hip_ctx, 2)
    fake = {"slot": 3, "out": h["out"], "inputs": h["inputs"]}
    with pytest.raises(RaftxError, match="nothing prepared"):
        hip_ctx.sweep_channels(fake, L)
    with pytest.raises(RaftxError, match="slot must be"):
        hip_ctx.sweep_channels({"slot": 9, "out": h["out"], "inputs": h["inputs"]}, L)
    with pytest.raises(RaftxError, match="nChan=65 must be 1 .. 64"):
        hip_ctx.sweep_channels(h, np.zeros((65, 3, 6)))
    with pytest.raises(RaftxError, match="nChan=0 must be 1 .. 64"):
        hip_ctx.sweep_channels(h, np.zeros((0, 3, 6)))
    with pytest.raises(RaftxError, match="nL=3 must be 1"):
        hip_ctx.sweep_channels(h, np.zeros((3, 10, 3, 6)))
    with pytest.raises(RaftxError, match="nG=2 must be 0"):
        hip_ctx.sweep_channels(h, L, Gw=np.zeros((2, 10, 6, nw), dtype=complex))
    with pytest.raises(ValueError, match="Gw has shape"):
        hip_ctx.sweep_channels(h, L, Gw=np.zeros((10, 6, nw + 1), dtype=complex))
    with pytest.raises(ValueError, match="L has shape"):
        hip_ctx.sweep_channels(h, np.zeros((10, 3, 5)))
    lib = hip_ctx.rlib.lib                                   # (the NULL arguments the Python layer never passes)
    std = np.zeros((n, 1, 10))
    ptr = lambda a: a.ctypes.data
    for args, msg in (((10, 1, None, 0, None, ptr(std)), "bad arguments"), ((10, 1, ptr(L), 0, None, None), "bad arguments"),
                      ((10, 1, ptr(L), 1, None, ptr(std)), "nG=1 without Gw")):
        assert lib.raftx_sweep_channels(hip_ctx._h, 2, *args) == -1
        err = (lib.raftx_last_error(hip_ctx._h) or b"").decode()
        assert msg in err, (msg, err)
    # none of the refused requests stuck; a second request replaces the first
    hip_ctx.sweep_channels(h, np.full((64, 3, 6), 7.0))
    hip_ctx.sweep_channels(h, L)
    sw.launch_crossing(hip_ctx, h)
    with pytest.raises(RaftxError, match="has been launched"):
        hip_ctx.sweep_channels(h, L)
    out = sw.wait_crossing(hip_ctx, h)
    alone = sw.run_crossing(hip_ctx, slot=0, channels=dict(L=L))
    assert out["chan_std"].shape == (n, 1, 10) and same_bits(out["chan_std"], alone["chan_std"]) and same_bits(out["std"], alone["std"])
    assert "chan_std" not in sw.run_crossing(hip_ctx, slot=2)             # the request ended with its crossing


def test_cancel_after_sweep_channels_leaves_the_output_untouched(hip_ctx):
    sw = _variant_sweep(64)
    CH = shared_rows(True)
    h = sw.prepare_crossing(hip_ctx, 1, channels=CH)
    S = h["out"]["chan_std"]
    S[:] = -7.25
    hip_ctx.sweep_cancel(h)
    assert np.all(S == -7.25)
    out = sw.run_crossing(hip_ctx, slot=1)                    # the slot is free again and carries no request
    assert "chan_std" not in out and np.all(S == -7.25)
    with pytest.raises(ValueError, match=r"channels=dict\(L="):
        sw.prepare_crossing(hip_ctx, 1, channels=dict(Gw=CH["Gw"]))
    assert "chan_std" not in sw.run_crossing(hip_ctx, slot=1)  # the refused request cancelled its crossing


# ------------------------------------------------------------------ 8. the recorded reference through a crossing
def test_recorded_reference_through_a_crossing(hip_ctx):
    sw = fixture_sweep()
    L, Gw = fixture_rows()
    out = sw.run_crossing(hip_ctx, channels=dict(L=L, Gw=Gw))
    assert np.all(out["flags"] & 1) and not np.any(out["flags"] & 2)
    got = {key: out["std"][:, :, i] for i, key in enumerate(KEYS[:6])}
    got.update({key: out["chan_std"][:, :, i] for i, key in enumerate(KEYS[6:])})
    check_against_reference(got, "device, crossing")
