"""Variant sweeps read their rows from the program: no expansion per crossing.

A crossing of a variant program keeps no member, station or cap rows in device memory.  The member pass, the ballast
trim and the table generation evaluate a row where they load it -- the program's base row, patched with the functions
k_geom_expand writes rows with.  The reference of every check here is the same designs as HOST-MADE descriptors
(VariantSweep.expanded_tables into a GeometrySweep, which has no program and reads plain rows): strip offsets, responses,
statistics, iteration counts and flags agree bit for bit (np.array_equal on the bit patterns), and props, fn and modes
where the eigen analysis rides along.

The shapes are the smallest at which an on-read row can go wrong: both sides of the 64-design switch of the member
kernels' layout, blocks that start at a design other than 0, each kind of edit alone, a heading, edited cap rows, and the
readers besides the member pass (ballast trim, MacCamy-Fuchs rows, another rho / g, per-design poses, which VariantSweep
does pass on).
"""
import os

import numpy as np
import pytest

from raft_amd import geometry as G
from raft_amd.sweep import GeometrySweep, VariantSweep
from tests.test_geometry import C3, _c3_crossing_inputs
from tests.test_fixed_members import (BASE, TOWER, TRIM, _assert_same, _check, _columns_only_program, _host_form, _message, _scales,
                                      _sweep)

MCF = 2                                                   # RAFTX_GM_FLAG_MCF
_coef = lambda c0=0.0, ccD=0.0, ocD=0.0, T=0.0, ocR=0.0, pH=0.0: [c0, ccD, ocD, T, ocR, pH]


def _params(n, rows=0):
    return G.volturnus_params(_scales(n, rows))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 130])
def test_hip_rows_on_read_across_the_layout_switch(hip_ctx, n):
    """the member kernels take the (member position, design) layout from 64 designs on: base-row addresses uniform over a
    wave there, gathered per lane below it; 65 and 130 leave a partly filled last wave"""
    _check(hip_ctx, _sweep(G.volturnus_program(BASE), _params(n)), "C3 program, n = %d" % n)


@pytest.mark.gpu
def test_hip_rows_on_read_in_blocks_that_start_past_design_zero(hip_ctx):
    """n = 70 in 7 blocks on three workers: blocks start at lo != 0 and are no multiple of 64 -- the block's parameter rows
    and the base indices of its members, stations and caps"""
    _check(hip_ctx, _sweep(G.volturnus_program(BASE), _params(70)), "blocks", 7, 3, modal=False)


def _ends_only_program():
    """the braces' ends follow the columns; no diameter is edited anywhere"""
    P = G.VariantProgram(G.describe_unit(BASE), 5)
    heads = np.atleast_1d(np.array(BASE["platform"]["members"][3]["heading"], dtype=float))
    z = _coef()
    for k in range(3):
        P.ends(7 + k, [_coef(ccD=0.5), z, _coef(14.545)], [_coef(ocD=-0.5, ocR=1.0), z, _coef(14.545)], heading=heads[k])
    assert not P.dia_edit.any()
    return P


def _diameter_only_program():
    """the centre column's diameter alone: S stays the base row's, D is edited"""
    P = G.VariantProgram(G.describe_unit(BASE), 5)
    P.diameter(0, _coef(ccD=1.0))
    assert not P.end_edit.any()
    return P


def _no_fixed_member_program():
    P = G.volturnus_program(BASE)
    P.diameter(TOWER, [6.5, 0, 0, 0, 0, 0])
    return P


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["ends only", "diameter only", "columns only", "no fixed member", "heading"])
def test_hip_each_kind_of_edit_alone(hip_ctx, which):
    P = {"ends only": _ends_only_program, "diameter only": _diameter_only_program, "columns only": _columns_only_program,
         "no fixed member": _no_fixed_member_program, "heading": lambda: G.volturnus_program(BASE, heading_adjust=30.0)}[which]()
    _check(hip_ctx, _sweep(P, _params(5)), which)
    _check(hip_ctx, _sweep(P, _params(66)), which + ", member grid", modal=False)


def _with_top_cap(P):
    """a cap at the upper end of the centre column, whose ends are edited: S = capFrac L with capFrac = 1"""
    b = P.base
    L = b.members[0, G.GM_L]
    assert b.stations[b.station_off[1] - 1, G.GS_S] == L and b.cap_off[1] == 1 and P.end_edit[0]
    b.caps = np.ascontiguousarray(np.vstack([b.caps[:1], [[L, 0.02, 0.0, 0.0]], b.caps[1:]]))
    b.cap_off = b.cap_off.copy()
    b.cap_off[1:] += 1
    return P


@pytest.mark.gpu
def test_hip_edited_cap_rows(hip_ctx):
    P = _with_top_cap(G.volturnus_program(BASE))
    vs = _sweep(P, _params(5))
    D = vs.expanded_tables(hip_ctx)
    assert len(np.unique(D.caps[1::len(P.base.caps), 0])) == 5                        # the cap does move with the draft
    got = _check(hip_ctx, vs, "top cap")
    plain = _sweep(G.volturnus_program(BASE), _params(5)).run_crossing(hip_ctx, modal=True, want_props=True)
    assert not np.array_equal(got["props"], plain["props"])                            # ... and its mass is in the statics
    _check(hip_ctx, _sweep(P, _params(5), add_mask=7 | TRIM), "top cap, ballast trim")
    _check(hip_ctx, _sweep(P, _params(66)), "top cap, member grid", modal=False)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 66])
def test_hip_the_other_readers_of_a_row(hip_ctx, n):
    """ballast trim (k_geom_reinertia reads the rows a second time), MacCamy-Fuchs columns (their rows hang on the
    generation's strips), another rho and g, and a per-design pose (no fixed record then: every member through the loader)"""
    P = G.volturnus_program(BASE)
    params = _params(n)
    _check(hip_ctx, _sweep(P, params, add_mask=7 | TRIM), "ballast trim", modal=(n == 5))
    _check(hip_ctx, _sweep(P, params, rho=1000.0, g=9.80665), "other rho / g", modal=False)
    Pm = G.volturnus_program(BASE)
    Pm.base.members[:4, G.GM_FLAGS] = MCF
    _check(hip_ctx, _sweep(Pm, params), "MacCamy-Fuchs columns", modal=False)
    # per-design poses
    rng = np.random.default_rng(3)
    pose = np.concatenate([rng.uniform(-2.0, 2.0, size=(n, 3)), rng.uniform(-0.05, 0.05, size=(n, 3))], axis=1)
    _, M0, B0, C0 = _c3_crossing_inputs(1)
    rep = lambda a: np.repeat(a[:1], n, axis=0)
    vs = VariantSweep(P, params, rep(M0), rep(B0), rep(C0), C3["w"], C3["k"], float(C3["depth"]), np.asarray(C3["zeta"])[None],
                      np.asarray(C3["beta"])[None], int(C3["nIter"]), float(C3["XiStart"]), pose=pose)
    host = GeometrySweep(vs.expanded_tables(hip_ctx), vs.M0, vs.B0, vs.C0, vs.w, vs.k, vs.depth, vs.zeta, vs.beta, vs.nIter,
                         vs.XiStart, tol=vs.tol, pose=pose, add_mask=vs.add_mask, rho=vs.rho, g=vs.g)
    got, want = vs.run_crossing(hip_ctx, want_Xi=True), host.run_crossing(hip_ctx, want_Xi=True)
    _assert_same(got, want, "per-design pose")
    unposed = _sweep(P, params).run_crossing(hip_ctx, want_Xi=True)
    assert not np.array_equal(got["std"], unposed["std"])


@pytest.mark.gpu
def test_hip_three_slots_with_their_own_parameter_rows(hip_ctx):
    ctx = hip_ctx
    n = 70
    P = G.volturnus_program(BASE)
    sweeps = [_sweep(P, _params(n, rows=i * n)) for i in range(3)]
    alone = [s.run_crossing(ctx, want_Xi=True) for s in sweeps]
    hs = [s.prepare_crossing(ctx, i, want_Xi=True) for i, s in enumerate(sweeps)]
    for h in hs:
        ctx.sweep_launch(h)
    for i, (s, h) in enumerate(zip(sweeps, hs)):
        _assert_same(s.wait_crossing(ctx, h), alone[i], "slot %d" % i)
    for i in (0, 2):
        _assert_same(alone[i], _host_form(ctx, sweeps[i]).run_crossing(ctx, want_Xi=True), "isolated %d" % i)
    assert not np.array_equal(alone[0]["std"], alone[1]["std"]) and not np.array_equal(alone[1]["std"], alone[2]["std"])


@pytest.mark.gpu
@pytest.mark.parametrize("case,match", [("length", "and length"), ("dls", "dlsMax")])
def test_hip_rejected_edited_member_fails_like_the_host_path(hip_ctx, case, match):
    ctx = hip_ctx
    P = G.volturnus_program(BASE)
    params = _params(5)
    if case == "length":
        # ccD / 2 = ocR - ocD / 2 (exactly, in the program's left-to-right sums): pontoons and braces of design 3 have no length
        params[3, 0], params[3, 1], params[3, 3] = 10.0, 12.5, 11.25
    else:
        P.base.members[0, G.GM_DLSMAX] = -1.0             # the centre column, whose ends and diameter are edited
    vs = _sweep(P, params)
    host = _host_form(ctx, vs)
    if case == "length":
        assert (host.tables.members[:, G.GM_L] == 0.0).sum() == 6
    got = _message(lambda: vs.run_crossing(ctx))
    want = _message(lambda: host.run_crossing(ctx))
    assert match in got and got[got.index("member"):] == want[want.index("member"):], (got, want)
    _check(ctx, _sweep(G.volturnus_program(BASE), _params(5)), "the context still works", modal=False)


@pytest.mark.gpu
def test_hip_generating_form_then_rows_on_read_in_one_process(hip_ctx):
    """RAFTX_FUSED_GEN=1 (read when the crossing is prepared): the job materialises its rows with k_geom_expand and the
    fused kernel builds the tables; without it the next crossing of the same program keeps no rows"""
    ctx = hip_ctx
    vs = _sweep(G.volturnus_program(BASE), _params(70))
    want = _host_form(ctx, vs).run_crossing(ctx, want_Xi=True)
    prev = os.environ.get("RAFTX_FUSED_GEN")

    def setenv(on):
        if on:
            os.environ["RAFTX_FUSED_GEN"] = "1"
        else:
            os.environ.pop("RAFTX_FUSED_GEN", None)

    def staged(at_prepare, at_launch):
        """two crossings in flight, as a stream has them (an isolated crossing that downloads its responses is cut into slabs
        and never takes the generating form): the second one's result"""
        setenv(at_prepare)
        hs = [vs.prepare_crossing(ctx, slot, n_chunk=1, want_Xi=True) for slot in (0, 1)]      # one block: its rows are decided here
        setenv(at_launch)
        for h in hs:
            ctx.sweep_launch(h)
        first, second = [vs.wait_crossing(ctx, h) for h in hs]
        _assert_same(first, second, "the two in flight")
        return second

    try:
        fused = staged(True, True)
        on_read = staged(False, False)
        mixed = staged(False, True)                       # no rows in memory: the generation kernel it is
    finally:
        if prev is None:
            os.environ.pop("RAFTX_FUSED_GEN", None)
        else:
            os.environ["RAFTX_FUSED_GEN"] = prev
    assert fused["generation_fused_blocks"][0] >= 1 and fused["generation_fused_blocks"][0] == fused["generation_fused_blocks"][1]
    assert on_read["generation_fused_blocks"][0] == 0 and mixed["generation_fused_blocks"][0] == 0
    for got, what in ((fused, "generating form"), (on_read, "rows on read"), (mixed, "prepared without, launched with")):
        _assert_same(got, want, what)
