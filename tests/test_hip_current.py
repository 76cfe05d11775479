"""Mean current loads on the device (include/raftx_current.h): Engine.calcCurrentLoads on the stand-ins of the reference's
decks, raftx_current_loads on the 64 C3 variants (reference-packed and device-generated tables) and on synthetic tables
with every edge the kernel has, all against the extended-precision evaluation of tests/current_reference.py under the gate
|x - ref| <= C eps E of DESIGN.md section 4; the streamed crossings bit for bit against the resident call.

Bounds that are not the gate itself:
  * device against a RECORDED reference value on the same table: 2 C eps E -- both lie within C eps E of the
    extended-precision value (the recorded ones: tests/test_current.py), the triangle inequality gives the rest;
  * device on a GENERATED table against a recorded value: the generator reproduces the reference-built records to 1e-11
    of the largest entry of a field (tests/test_geometry.py check_c3) and an addend is a product of at most eight record
    fields (coefficient, the profile through z twice, four direction components, the arm), so to first order the loads
    move by at most 8e-11 of the envelope.  A unit vector is reproduced to 1e-11 of its LENGTH, not of each component
    (an upright column's q has a horizontal component of 1e-17 in one table and another 1e-17 in the other), which moves
    load between the three components of the force and between those of the moment: the envelope of this comparison is,
    per design and current, the largest of the three force envelopes and the largest of the three moment envelopes.
    The bound is (2 C eps + 1.6e-10) times that (1.6e-10: twice the first-order figure).
"""
import json
from types import SimpleNamespace

import numpy as np
import pytest

from raft_amd import dropin
from raft_amd import geometry as G
from raft_amd import snapshot as standin
from raft_amd._abi import RaftxError
from raft_amd.sweep import GeometrySweep
from tests import current_reference as cr
from tests.test_current import CURRENTS, DECKS, FX, UNITS, unit_model, unit_reference
from tests.test_hip_modal import _variant_sweep
from tests.util import random_strips

pytestmark = pytest.mark.gpu
C = cr.GATE_C
SPEED, HEAD = np.ascontiguousarray(CURRENTS[:, 0]), np.ascontiguousarray(CURRENTS[:, 1])
C3_UNITS = [u for u in UNITS if u["name"].startswith("C3-variant-")]


def gate(x, D, E, what, mult=C, extra=0.0):
    """Every entry of x within (mult eps + extra) E of D, exact zeros where E is 0, NaN where D is NaN; prints the worst
    multiple of eps E."""
    x = np.asarray(x)
    assert x.shape == np.asarray(D).shape, what
    m = cr.gate_multiples(x, D, E)
    print("%s: worst %.2f eps E over %d entries" % (what, m.max(), m.size))
    assert np.all(m <= mult + extra / cr.EPS), (what, float(m.max()), np.argwhere(m > mult + extra / cr.EPS)[:4].tolist())
    return float(m.max())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------ fixture parity
def test_dropin_decks_and_pose_model(hip_ctx):
    eng = dropin.Engine(hip_ctx)
    pick = {p["name"]: p for p in FX["pickle"]}
    for u in [x for x in UNITS if not x["name"].startswith("C3-variant-")]:
        model, fowt = unit_model(u)
        Dref, E = unit_reference(u)
        dev = np.array([eng.calcCurrentLoads(fowt, {"current_speed": s, "current_heading": h}) for s, h in CURRENTS])
        assert fowt.D_hydro.shape == (6,) and same_bits(fowt.D_hydro, dev[-1])
        gate(dev, Dref, E, u["name"] + " drop-in")
        gate(dev, u["D"], E, u["name"] + " drop-in against the live reference", mult=2 * C)
        if u["name"] in pick:
            ic = [i for i, (s, h) in enumerate(CURRENTS) if (s, h) == (2.0, 15.0)][0]
            gate(dev[ic], pick[u["name"]]["D"], E[ic], u["name"] + " drop-in against the reference's pickle", mult=2 * C)
    assert set(pick) == set(DECKS)
    # the reference's defaults: no current in the case -> exact zeros
    assert np.all(eng.calcCurrentLoads(fowt, {}) == 0)
    # the submerged-rotor rule (raft_fowt.py:1971-1974) and the unit's own exponent
    z = FX["zref"]
    u = UNITS[[x["name"] for x in UNITS].index(z["name"])]
    model, fowt = unit_model(u)
    fowt.rotorList = [SimpleNamespace(r3=np.array([0.0, 0.0, 150.0])), SimpleNamespace(r3=np.array([0.0, 0.0, float(z["Zref"])]))]
    fowt.shearExp_water = float(z["shearExp"])
    Dref, E = unit_reference(u, Zref=float(z["Zref"]), shearExp=float(z["shearExp"]))
    dev = np.array([eng.calcCurrentLoads(fowt, {"current_speed": s, "current_heading": h}) for s, h in CURRENTS])
    gate(dev, Dref, E, "Zref -25, exponent 0.2")
    gate(dev, z["D"], E, "Zref -25, exponent 0.2 against the live members", mult=2 * C)


def test_c3_variants_on_the_reference_packed_tables(hip_ctx):
    c3 = standin.load_fixture("c3_variants.npz")
    n = len(C3_UNITS)
    off = np.asarray(c3["strip_offsets"])[:n + 1]
    zero = np.zeros((n, 6, 6))
    hip_ctx.upload_designs_raw(off, np.asarray(c3["strips"])[:off[-1]], zero, zero, zero, 4)
    dev = hip_ctx.current_loads(SPEED, HEAD, float(c3["depth"]))
    ref = [unit_reference(u) for u in C3_UNITS]
    Dref, E = np.array([r[0] for r in ref]), np.array([r[1] for r in ref])
    gate(dev, Dref, E, "C3 variants, packed tables")
    gate(dev, np.array([u["D"] for u in C3_UNITS]), E, "C3 variants, packed tables against the live reference", mult=2 * C)


def test_c3_variants_generated_by_build_designs(hip_ctx):
    n = len(C3_UNITS)
    sw = _variant_sweep(n)
    sw.upload(hip_ctx)                                        # raftx_build_designs
    assert np.array_equal(sw.off, np.asarray(standin.load_fixture("c3_variants.npz")["strip_offsets"])[:n + 1])
    dev = sw.run_current(hip_ctx, SPEED, HEAD)
    strips, _ = hip_ctx.fetch_strips(sw.off[-1])
    Dref, E = cr.current_loads(strips, sw.off, SPEED, HEAD, sw.depth)
    gate(dev, Dref, E, "C3 variants, generated tables")
    Eg = np.concatenate([np.repeat(E[..., :3].max(axis=-1, keepdims=True), 3, axis=-1),
                         np.repeat(E[..., 3:].max(axis=-1, keepdims=True), 3, axis=-1)], axis=-1)
    gate(dev, np.array([u["D"] for u in C3_UNITS]), Eg, "C3 variants, generated tables against the live reference",
         mult=2 * C, extra=1.6e-10)
    assert same_bits(dev, sw.run_current(hip_ctx, SPEED, HEAD))


# ------------------------------------------------------------------ synthetic tables
DEPTH = 120.0


def synthetic_batch():
    """One batch of designs (strip tables [n,32]) with every path of the kernel: strip counts 0, 1, 63, 64, 65, 130 (below,
    at and above one strip per lane; a third round of the lane loop), a rectangular member, a member parallel to the
    current of heading 0 (|vp| == 0 exactly), a strip exactly at the seabed, a design with one strip below the seabed and
    a dry strip in an otherwise wet design."""
    rng = np.random.default_rng(2024)
    tabs = [random_strips(rng, S).strips for S in (0, 1, 63, 64, 65, 130)]
    rect = random_strips(rng, 7).strips
    rect[:, 23] = 0.0
    rect[:, 6:15] = np.array([0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
    par = random_strips(rng, 5).strips
    par[:, 23] = 1.0
    par[:, 6:15] = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    par[:, 20:22] = rng.uniform(1e3, 4e4, size=(5, 2))
    bed = random_strips(rng, 9).strips
    bed[4, 2] = -DEPTH
    below = random_strips(rng, 66).strips
    below[65, 2] = -DEPTH - 3.0
    dry = random_strips(rng, 6).strips
    dry[2, 2] = 0.0
    dry[3, 2] = 1.5
    tabs += [rect, par, bed, below, dry]
    names = ["S0", "S1", "S63", "S64", "S65", "S130", "rectangular", "parallel", "seabed", "below", "dry"]
    off = np.concatenate([[0], np.cumsum([len(t) for t in tabs])]).astype(np.int64)
    return names, off, np.concatenate(tabs, axis=0)


@pytest.mark.parametrize("nCur", [1, 3])
def test_synthetic_tables(hip_ctx, nCur):
    names, off, strips = synthetic_batch()
    n = len(names)
    zero = np.zeros((n, 6, 6))
    hip_ctx.upload_designs_raw(off, strips, zero, zero, zero, 4)
    speed = np.array([1.7, 0.0, 0.9])[:nCur]
    head = np.array([0.0, 33.0, -145.0])[:nCur]
    Zref = np.where(np.arange(n) % 2 == 1, -18.5, 0.0)         # a submerged rotor on every other design
    dev = hip_ctx.current_loads(speed, head, DEPTH, Zref=Zref, shearExp=1.0 / 7.0)
    Dref, E = cr.current_loads(strips, off, speed, head, DEPTH, Zref=Zref, shearExp=1.0 / 7.0)
    gate(dev, Dref, E, "synthetic tables, nCur %d" % nCur)
    ib = names.index("below")
    assert np.all(np.isnan(dev[ib])) and np.all(np.isfinite(np.delete(dev, ib, axis=0)))
    assert np.all(dev[names.index("S0")] == 0)
    ip = names.index("parallel")
    assert np.all(E[ip, 0, 1:3] == 0) and np.all(dev[ip, 0, 1:3] == 0) and dev[ip, 0, 0] != 0   # axial drag only
    if nCur > 1:
        assert np.all(np.delete(dev, ib, axis=0)[:, 1] == 0)    # speed 0
    assert same_bits(dev, hip_ctx.current_loads(speed, head, DEPTH, Zref=Zref, shearExp=1.0 / 7.0))
    # the bits of a design do not depend on the batch: alone, and for one current alone
    for d in (names.index("S130"), names.index("rectangular")):
        hip_ctx.upload_designs_raw(off[d:d + 2] - off[d], strips[off[d]:off[d + 1]], zero[:1], zero[:1], zero[:1], 4)
        one = hip_ctx.current_loads(speed, head, DEPTH, Zref=Zref[d:d + 1], shearExp=1.0 / 7.0)
        assert same_bits(one[0], dev[d])
        last = hip_ctx.current_loads(speed[-1:], head[-1:], DEPTH, Zref=Zref[d:d + 1], shearExp=1.0 / 7.0)
        assert same_bits(last[0, 0], dev[d, nCur - 1])


def test_more_currents_than_one_tile(hip_ctx):
    """Nine currents are three waves per design: the same bits as the currents one by one."""
    names, off, strips = synthetic_batch()
    keep = [i for i, nm in enumerate(names) if nm != "below"]
    tabs = [strips[off[i]:off[i + 1]] for i in keep]
    off2 = np.concatenate([[0], np.cumsum([len(t) for t in tabs])]).astype(np.int64)
    s2 = np.concatenate(tabs, axis=0)
    zero = np.zeros((len(keep), 6, 6))
    hip_ctx.upload_designs_raw(off2, s2, zero, zero, zero, 4)
    dev = hip_ctx.current_loads(SPEED, HEAD, DEPTH)
    Dref, E = cr.current_loads(s2, off2, SPEED, HEAD, DEPTH)
    gate(dev, Dref, E, "synthetic tables, nine currents")
    assert np.all(np.isfinite(dev))
    for i in (0, 4, 8):
        assert same_bits(hip_ctx.current_loads(SPEED[i:i + 1], HEAD[i:i + 1], DEPTH)[:, 0], dev[:, i])


def test_argument_errors(hip_lib):
    ctx = hip_lib.context(0)
    try:
        with pytest.raises(RaftxError, match="no design set"):
            ctx.current_loads([1.0], [0.0], 100.0)
        names, off, strips = synthetic_batch()
        zero = np.zeros((len(names), 6, 6))
        ctx.upload_designs_raw(off, strips, zero, zero, zero, 4)
        with pytest.raises(RaftxError, match="nCur must be positive"):
            ctx.current_loads([], [], 100.0)
        for bad in (dict(speed=[np.nan]), dict(heading=[np.inf]), dict(depth=np.nan), dict(shearExp=np.inf), dict(Zref=np.nan)):
            a = dict(speed=[1.0], heading=[0.0], depth=100.0, shearExp=0.12, Zref=None)
            a.update(bad)
            with pytest.raises(RaftxError, match="finite"):
                ctx.current_loads(a["speed"], a["heading"], a["depth"], Zref=a["Zref"], shearExp=a["shearExp"])
        with pytest.raises(RaftxError, match="depth \\+ Zref must be positive"):
            ctx.current_loads([1.0], [0.0], 100.0, Zref=-100.0)
        with pytest.raises(RaftxError, match="depth \\+ Zref must be positive"):
            ctx.current_loads([1.0], [0.0], 0.0)
    finally:
        ctx.close()


# ------------------------------------------------------------------ sweep crossings: bitwise identity
CUR = dict(speed=[2.0, 0.0, 0.6], heading=[15.0, 90.0, 400.0], Zref=-12.0, shearExp=0.2)


def _geometry_sweep(n):
    fg = standin.load_fixture("geom_units.npz")
    c3 = standin.load_fixture("c3_variants.npz")
    vs = _variant_sweep(n)
    D = G.volturnus_sweep(json.loads(fg["c3_base_json"]), np.asarray(c3["scales"])[:n]).tables()
    return GeometrySweep(D, vs.M0, vs.B0, vs.C0, vs.w, vs.k, vs.depth, vs.zeta, vs.beta, vs.nIter, vs.XiStart)


@pytest.mark.parametrize("kind", ["variant", "geometry"])
@pytest.mark.parametrize("n_chunk", [1, 3])
def test_crossing_equals_the_resident_call(hip_ctx, kind, n_chunk):
    n = 64
    sw = _variant_sweep(n) if kind == "variant" else _geometry_sweep(n)
    plain = sw.run_crossing(hip_ctx, n_chunk=n_chunk)
    assert "D_hydro" not in plain
    out = sw.run_crossing(hip_ctx, n_chunk=n_chunk, current=CUR)
    for k in ("std", "niter", "flags"):
        assert same_bits(plain[k], out[k]), k
    assert out["D_hydro"].shape == (n, 3, 6)
    sw.upload(hip_ctx)
    res = sw.run_current(hip_ctx, CUR["speed"], CUR["heading"], Zref=CUR["Zref"], shearExp=CUR["shearExp"])
    assert same_bits(out["D_hydro"], res)
    assert np.all(np.isfinite(res)) and np.all(res[:, 1] == 0) and np.all(res[:, 0, 0] > 0)


def test_current_and_modal_in_one_crossing(hip_ctx):
    n = 64
    sw = _variant_sweep(n)
    both = sw.run_crossing(hip_ctx, n_chunk=3, modal=True, want_props=True, current=CUR)
    modal = sw.run_crossing(hip_ctx, n_chunk=3, modal=True, want_props=True)
    cur = sw.run_crossing(hip_ctx, n_chunk=3, current=CUR)
    for k in ("std", "niter", "flags", "fn", "modes", "modal_flags", "props"):
        assert same_bits(both[k], modal[k]), k
    assert same_bits(both["D_hydro"], cur["D_hydro"]) and "fn" not in cur and "D_hydro" not in modal


def test_fused_generation_is_bypassed_with_current_loads(hip_ctx, monkeypatch):
    """RAFTX_FUSED_GEN=1 leaves no tables in device memory: a crossing with current loads takes the k_geom_design route
    for all its blocks and returns the same bits."""
    sw = _variant_sweep(64)
    ref = sw.run_crossing(hip_ctx, n_chunk=2, current=CUR)
    monkeypatch.setenv("RAFTX_FUSED_GEN", "1")
    fused = sw.run_crossing(hip_ctx, n_chunk=2)
    out = sw.run_crossing(hip_ctx, n_chunk=2, current=CUR)
    assert fused["generation_fused_blocks"][0] > 0 and out["generation_fused_blocks"][0] == 0
    for k in ("std", "niter", "flags", "D_hydro"):
        assert same_bits(ref[k], out[k]), k
    assert same_bits(fused["std"], out["std"])


# ------------------------------------------------------------------ slot errors
def test_sweep_current_on_idle_or_launched_slot(hip_ctx):
    sw = _variant_sweep(64)
    h = sw.prepare_crossing(hip_ctx, 2)
    fake = {"slot": 3, "out": h["out"]}
    with pytest.raises(RaftxError, match="nothing prepared"):
        hip_ctx.sweep_current(fake, [1.0], [0.0])
    with pytest.raises(RaftxError, match="depth \\+ Zref must be positive"):
        hip_ctx.sweep_current(h, [1.0], [0.0], Zref=-1e4)
    sw.launch_crossing(hip_ctx, h)
    with pytest.raises(RaftxError, match="has been launched"):
        hip_ctx.sweep_current(h, [1.0], [0.0])
    out = sw.wait_crossing(hip_ctx, h)
    assert "D_hydro" not in out
    alone = sw.run_crossing(hip_ctx, slot=0)
    assert same_bits(out["std"], alone["std"])


def test_cancel_after_sweep_current_leaves_the_output_untouched(hip_ctx):
    sw = _variant_sweep(64)
    h = sw.prepare_crossing(hip_ctx, 1, current=CUR)
    D = h["out"]["D_hydro"]
    D[:] = -7.25
    hip_ctx.sweep_cancel(h)
    assert np.all(D == -7.25)
    out = sw.run_crossing(hip_ctx, slot=1)                    # the slot is free again and carries no request
    assert "D_hydro" not in out and np.all(D == -7.25)
    with pytest.raises(ValueError, match="speed"):
        sw.prepare_crossing(hip_ctx, 1, current=dict(heading=[0.0]))
    assert "D_hydro" not in sw.run_crossing(hip_ctx, slot=1)  # the refused request cancelled its crossing
