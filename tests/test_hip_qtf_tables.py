"""GPU suite for the second-order QTF tables generated on the device (include/raftx_qtfgen.h): the records against
raft_amd.qtf.pack_qtf of the LIVE reference (tests/golden/refgold_qtf_tables.npz), the Kim & Yue items, the QTF entry on
resident tables against the existing entry fed the same records, the variant route, the reference's own QTF golden from
the deck's descriptors, and Sweep.run_second_order without host tables.  Small shapes: nw2 = 8, two headings, 3-4 designs."""
import ctypes as C
import json

import numpy as np
import pytest

from raft_amd import geometry as G
from raft_amd import qtf as rq
from raft_amd import snapshot as standin
from raft_amd import waves
from raft_amd._abi import RaftxError
from raft_amd.sweep import GeometrySweep
from tests.util import group_rel_err, rel_err

pytestmark = pytest.mark.gpu

GEOM = standin.load_fixture("geom_units.npz")
GOLD = standin.load_fixture("refgold_qtf_tables.npz")
UNITS = {u["name"]: u for u in GEOM["units"]}
QU = {u["name"]: u for u in GOLD["units"]}
NAMES = list(UNITS)
HEADINGS = np.asarray(GOLD["headings"], dtype=float)
TOL = 1e-11          # tests/test_geometry.py holds the first-order generator to the same bound against the same reference
W2 = np.linspace(0.35, 1.6, 8)
K2 = np.array([waves.wave_number(x, 200.0) for x in W2])
S_GROUPS = [(0, 3), (3, 6), (6, 9), (9, 12), (12, 15), (15, 16), (16, 17), (17, 18)]      # r q p1 p2 Ca v_side v_end a_i
M_GROUPS = [(1, 4), (4, 5), (5, 7), (7, 10), (10, 13)]                                   # r_int a_wl Ca p1 p2


def tables_of(u):
    return G.describe_unit(json.loads(u["design_json"]), heading_adjust=float(u["heading_adjust"]))


def empty_unit():
    """One member wholly above water: the tower of OC3spar."""
    e = GOLD["empty"]
    t, m = tables_of(UNITS[str(e["unit"])]), int(e["member"])
    assert t.members[m, G.GM_RA + 2] > 0 and t.members[m, G.GM_RB + 2] > 0
    return G.MemberTable([t.members[m]], [t.stations[t.station_off[m]:t.station_off[m + 1]]], [t.caps[t.cap_off[m]:t.cap_off[m + 1]]])


def batch(names):
    """DesignTables + pose of the named golden units; None stands for the empty design (pose 0)."""
    D = G.concat_units([empty_unit() if n is None else tables_of(UNITS[n]) for n in names])
    pose = np.array([np.zeros(6) if n is None else np.asarray(UNITS[n]["pose"], dtype=float) for n in names])
    return D, pose


def gold_table(name):
    u = QU[name]
    return rq.QtfTable(u["strips"], u["members"], [dict(g) for g in u["kay_geom"]])


def close(a, b, groups, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    for c0, c1 in groups:
        if b[:, c0:c1].size:
            assert rel_err(a[:, c0:c1], b[:, c0:c1]) < TOL, (what, c0)


def smooth_xi(rng, n_set, w):
    amp = np.array([1.0, 0.3, 0.7, 0.01, 0.02, 0.004])[None, :, None] / (1.0 + (w[None, None, :] / 0.6) ** 2)
    return amp * np.exp(1j * (rng.uniform(0, 6, (n_set, 6, 1)) + 1.5 * w[None, None, :]))


# ------------------------------------------------------------------ 1. records
def test_records_of_every_golden_unit_in_one_ragged_batch(hip_ctx):
    names = NAMES[:5] + [None] + NAMES[5:]
    D, pose = batch(names)
    soff, moff = hip_ctx.qtf_tables_build(D, pose)
    want_s = [0 if n is None else len(QU[n]["strips"]) for n in names]
    want_m = [0 if n is None else len(QU[n]["members"]) for n in names]
    assert np.array_equal(soff, np.concatenate([[0], np.cumsum(want_s)]))
    assert np.array_equal(moff, np.concatenate([[0], np.cumsum(want_m)]))
    assert hip_ctx.qtf_tables_counts()[:3] == (len(names), sum(want_s), sum(want_m))
    tabs = hip_ctx.qtf_tables_fetch()
    assert len(tabs) == len(names)
    n_mcf = 0
    for n, t in zip(names, tabs):
        if n is None:
            assert t.strips.shape == (0, rq.QS_N) and t.members.shape == (0, rq.QM_N) and not t.kay_geom
            continue
        g = QU[n]
        gs, gm = np.asarray(g["strips"]).reshape(-1, rq.QS_N), np.asarray(g["members"]).reshape(-1, rq.QM_N)
        assert np.array_equal(t.strips[:, 18:], gs[:, 18:]), n            # member index among the kept members; spare fields
        assert np.array_equal(t.members[:, 0], gm[:, 0]) and np.array_equal(t.members[:, 13:], gm[:, 13:]), n
        close(t.strips, gs, S_GROUPS, n)
        close(t.members, gm, M_GROUPS, n)
        assert len(t.kay_geom) == len(g["kay_geom"]), n
        for a, b in zip(t.kay_geom, g["kay_geom"]):
            n_mcf += 1
            assert a["r"].shape == np.asarray(b["r"]).shape
            for key in ("rA", "rB", "r", "ds", "dls", "p1", "p2"):
                assert rel_err(a[key], b[key]) < TOL, (n, key)
            assert np.array_equal(a["dls"] != 0, np.asarray(b["dls"]) != 0)      # kay_items branches on it
    assert n_mcf >= 8


@pytest.mark.parametrize("name", ["VolturnUS-S-test@pose", "OC4semi@heel", "synthetic@heel", "farm-unit-2"])
def test_strip_nodes_are_the_first_order_generator_bits(name, hip_ctx):
    """r, q, p1, p2 of the QTF strips against RAFTX_F_X / Q / P1 / P2 of raftx_build_designs + raftx_fetch_strips at the
    same pose: the same device functions, the same bits."""
    u = UNITS[name]
    D, pose = batch([name])
    Z = np.zeros((1, 6, 6))
    off = hip_ctx.build_designs(D.member_off, D.members, D.station_off, D.stations, Z, Z, Z, len(u["w"]), pose=pose,
                                rho=u["rho"], g=u["g"], k=u["k"], cap_off=D.cap_off, caps=D.caps)
    first, _ = hip_ctx.fetch_strips(off[-1], len(u["cm"]))
    hip_ctx.qtf_tables_build(D, pose)
    t = hip_ctx.qtf_tables_fetch()[0]
    assert t.strips.shape[0] == first.shape[0] > 0
    assert np.array_equal(t.strips[:, 0:3].view(np.uint64), first[:, 0:3].view(np.uint64))        # RAFTX_F_X
    assert np.array_equal(t.strips[:, 3:12].view(np.uint64), first[:, 6:15].view(np.uint64))      # RAFTX_F_Q, P1, P2


# ------------------------------------------------------------------ 2. Kim & Yue items
def test_kim_yue_items_at_the_golden_headings(hip_ctx):
    names = ["VolturnUS-S-test@pose", "C3-variant-0", "OC4semi", None, "OC4semi@heel"]
    D, pose = batch(names)
    hip_ctx.qtf_tables_build(D, pose)
    ioff, items = hip_ctx.qtf_tables_kay_items(HEADINGS)
    nC = len(HEADINGS)
    assert len(ioff) == len(names) * nC + 1 and ioff[-1] == len(items)
    total = 0
    for d, n in enumerate(names):
        for c in range(nC):
            want = np.zeros((0, rq.QK_N)) if n is None else np.asarray(QU[n]["kay_items"][c]).reshape(-1, rq.QK_N)
            got = items[ioff[d * nC + c]:ioff[d * nC + c + 1]]
            assert got.shape == want.shape, (n, c)
            if len(want):
                assert np.array_equal(got[:, 1], want[:, 1]), (n, c)                   # kind
                for c0, c1 in [(0, 1), (2, 4), (4, 7), (7, 10), (10, 12)]:           # R | z1 z2 | arm | pforce | waterline point
                    assert rel_err(got[:, c0:c1], want[:, c0:c1]) < TOL, (n, c, c0)
            total += len(want)
    assert total > 100


# ------------------------------------------------------------------ 3. same kernels, same bits
def test_resident_entry_is_the_existing_entry_on_the_fetched_records(hip_ctx):
    names = ["VolturnUS-S-test@pose", "synthetic@heel", "OC4semi@heel"]
    rng = np.random.default_rng(31)
    nD, nC = len(names), len(HEADINGS)
    Xi = smooth_xi(rng, nD * nC, W2)
    Ms = np.array([np.asarray(UNITS[n]["M_struc"]) for n in names])
    depth, rho, g = 200.0, 1025.0, 9.81
    D, pose = batch(names)
    hip_ctx.qtf_tables_build(D, pose)
    tabs = hip_ctx.qtf_tables_fetch()
    assert sum(len(t.kay_geom) for t in tabs) >= 6
    q0 = hip_ctx.qtf_slender_resident(Xi, HEADINGS, W2, K2, depth, rho, g, Ms, Nm=0)
    rep_t = [tabs[d] for d in range(nD) for _ in range(nC)]
    rep_b = np.tile(HEADINGS, nD)
    rep_M = np.repeat(Ms, nC, axis=0)
    ref0 = hip_ctx.qtf_slender(rep_t, Xi, rep_b, W2, K2, depth, rho, g, rep_M, None)
    assert np.any(q0) and np.array_equal(q0.view(np.float64), ref0.view(np.float64))
    # Kim & Yue correction built on the device against the existing path fed the host table (SciPy Hankel functions)
    kay = np.array([rq.kay_correction(t.kay_geom, W2, K2, b, depth, rho=rho, g=g, Nm=10) for t, b in zip(rep_t, rep_b)])
    q10 = hip_ctx.qtf_slender_resident(Xi, HEADINGS, W2, K2, depth, rho, g, Ms, Nm=10)
    ref10 = hip_ctx.qtf_slender(rep_t, Xi, rep_b, W2, K2, depth, rho, g, rep_M, kay)
    assert rel_err(q10, ref10) < 1e-10
    assert rel_err(q10, q0) > 1e-6                                       # the correction is there
    # the design order permuted: set s reads the table of design s // nCase
    perm = [2, 0, 1]
    Dp, posep = batch([names[i] for i in perm])
    hip_ctx.qtf_tables_build(Dp, posep)
    sets = np.array([i * nC + c for i in perm for c in range(nC)])
    qp = hip_ctx.qtf_slender_resident(Xi[sets], HEADINGS, W2, K2, depth, rho, g, Ms[perm], Nm=0)
    assert np.array_equal(qp.view(np.float64), q0[sets].view(np.float64))


# ------------------------------------------------------------------ 4. variants
def test_variant_route_gives_the_records_of_the_expanded_descriptors(hip_ctx):
    P = G.volturnus_program(json.loads(GEOM["c3_base_json"]))
    params = G.volturnus_params(np.random.default_rng(0).uniform(0.75, 1.25, size=(4, 5)))
    hip_ctx.variant_program(P)
    soff, moff = hip_ctx.qtf_tables_build_variants(params)
    a = hip_ctx.qtf_tables_fetch(raw=True)
    assert soff[-1] > 100 and len(set(np.diff(soff))) > 1                 # the variants differ
    T = P.tables(hip_ctx.expand_variants(params), 4)
    soff2, moff2 = hip_ctx.qtf_tables_build(T)
    b = hip_ctx.qtf_tables_fetch(raw=True)
    assert np.array_equal(soff, soff2) and np.array_equal(moff, moff2)
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64))
    # ... and at a pose
    pose = np.tile([1.0, -2.0, 0.2, 0.03, -0.02, 0.1], (4, 1))
    hip_ctx.qtf_tables_build_variants(params, pose)
    a = hip_ctx.qtf_tables_fetch(raw=True)
    hip_ctx.qtf_tables_build(T, pose)
    b = hip_ctx.qtf_tables_fetch(raw=True)
    for x, y in zip(a, b):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64))


# ------------------------------------------------------------------ 5. against the reference's numbers
def test_reference_golden_qtf_from_the_decks_descriptors(hip_ctx):
    """tests/test_hip_qtf.py::test_reference_golden_qtf_fixed_body with the tables generated from the deck's descriptors
    and the Kim & Yue correction built on the device: same bound, same gate."""
    fx = standin.load_fixture("refgold_qtf_VolturnUS-S.npz")
    f = standin.build_model(fx["model"]).fowtList[0]
    d = GOLD["deck"]
    n = len(d["gm"])
    T = G.DesignTables(np.array([0, n], dtype=np.int64), d["gm"], d["station_off"], d["gs"], d["cap_off"], d["caps"])
    hip_ctx.qtf_tables_build(T)
    w2, k2 = f.w1_2nd, f.k1_2nd
    q = hip_ctx.qtf_slender_resident(np.zeros((1, 6, len(w2))), [fx["fixed_beta"]], w2, k2, f.depth, f.rho_water, f.g,
                                     f.M_struc[None], Nm=10)[0]
    np.testing.assert_allclose(q, fx["fixed_qtf"], rtol=1e-5, atol=1e-3)      # the reference's own gate
    assert rel_err(q, fx["fixed_qtf"]) < 1e-9


# ------------------------------------------------------------------ 6. end to end
def test_run_second_order_without_host_tables(hip_ctx):
    names = ["VolturnUS-S-test@pose", "C3-variant-1", "OC4semi@heel"]
    D, pose = batch(names)
    nw = 40
    w = np.arange(1, nw + 1) * 0.05
    depth = 200.0
    k = np.array([waves.wave_number(x, depth) for x in w])
    us = [UNITS[n] for n in names]
    M_extra = np.array([np.asarray(u["M_struc"]) - np.asarray(u["M_struc_bare"]) for u in us])
    C_extra = np.array([np.asarray(u["C_struc"]) - np.asarray(u["C_struc_bare"]) + np.diag([7e4, 7e4, 0, 0, 0, 1e8]) for u in us])
    rng = np.random.default_rng(9)
    zeta = rng.uniform(0.2, 0.6, size=(2, 1, nw)) / (1.0 + ((w - 0.6) / 0.25) ** 2)[None, None, :]
    beta = np.array([[0.0], [0.4]])
    S0 = 0.5 * zeta[:, 0, :] ** 2 / (w[1] - w[0])
    sw = GeometrySweep(D, M_extra, np.zeros((3, 6, 6)), C_extra, w, k, depth, zeta, beta, nIter=12, XiStart=0.1, pose=pose)
    dev = sw.run_second_order(hip_ctx, None, None, W2, K2, S0)
    host = sw.run_second_order(hip_ctx, [gold_table(n) for n in names], np.array([np.asarray(u["M_struc"]) for u in us]), W2, K2, S0)
    assert np.array_equal(dev["niter"], host["niter"]) and np.array_equal(dev["flags"], host["flags"])
    assert np.any(dev["flags"] & 1)                                       # converged pairs take the second stage
    assert group_rel_err(dev["Xi"].reshape(-1, 6, nw), host["Xi"].reshape(-1, 6, nw)) < 1e-9
    assert np.any(dev["Fhydro_2nd"] != 0) and rel_err(dev["Fhydro_2nd"], host["Fhydro_2nd"]) < 1e-9


# ------------------------------------------------------------------ 7. errors
def test_argument_errors_come_before_any_launch(hip_lib):
    ctx = hip_lib.context(0)
    L, h = hip_lib.lib, ctx._h
    Ms = np.zeros((1, 6, 6))
    good = (np.zeros((1, 6, 8)), [0.3], W2, K2, 200.0, 1025.0, 9.81, Ms)
    try:
        with pytest.raises(RaftxError, match="no resident tables"):
            ctx.qtf_slender_resident(*good)
        with pytest.raises(RaftxError, match="no resident tables"):
            ctx.qtf_tables_counts()
        with pytest.raises(RaftxError, match="no program"):
            ctx._check(L.raftx_qtf_tables_build_variants(h, 1, None, None, None, None), "raftx_qtf_tables_build_variants")
        D, pose = batch(["OC3spar"])
        soff, _ = ctx.qtf_tables_build(D, pose)
        ref = ctx.qtf_slender_resident(*good, Nm=0)
        ms = ctx.last_kernel_ms()
        # builds that must fail, and leave the resident tables alone
        bad = G.DesignTables(D.member_off, D.members.copy(), D.station_off, D.stations, D.cap_off, D.caps)
        bad.members[1, G.GM_RA] = np.nan
        with pytest.raises(RaftxError, match="not finite"):
            ctx.qtf_tables_build(bad, pose)
        with pytest.raises(RaftxError, match="not finite"):
            ctx.qtf_tables_build(D, np.full_like(pose, np.inf))
        D2, pose2 = batch(["C3-variant-0"])
        so = D2.station_off.copy()
        assert len(so) > 4
        so[1], so[2] = so[2], so[1] - 1
        with pytest.raises(RaftxError, match="not monotone"):
            ctx.qtf_tables_build(G.DesignTables(D2.member_off, D2.members, so, D2.stations, D2.cap_off, D2.caps), pose2)
        mo = np.array([0, D.member_off[-1], D.member_off[-1] - 1], dtype=np.int64)
        rc = L.raftx_qtf_tables_build(h, 2, mo.ctypes.data_as(C.c_void_p), D.members.ctypes.data_as(C.c_void_p),
                                      D.station_off.ctypes.data_as(C.c_void_p), D.stations.ctypes.data_as(C.c_void_p), None, None, None)
        assert rc != 0 and b"not monotone" in L.raftx_last_error(h)
        assert L.raftx_qtf_tables_build(h, 1, None, None, None, None, None, None, None) != 0
        # the QTF entry
        cases = [dict(beta=[]), dict(w2=np.zeros(0), k2=np.zeros(0), Xi=np.zeros((1, 6, 0))), dict(Nm=11), dict(Nm=-1)]
        for kw in cases:
            a = dict(Xi=good[0], beta=good[1], w2=W2, k2=K2, Nm=0)
            a.update(kw)
            with pytest.raises((RaftxError, ValueError)):
                ctx.qtf_slender_resident(a["Xi"] if len(a["beta"]) else None, a["beta"], a["w2"], a["k2"], 200.0, 1025.0, 9.81, Ms, Nm=a["Nm"])
        p = lambda x: np.ascontiguousarray(x, dtype=np.float64).ctypes.data_as(C.c_void_p)
        for drop in range(4):                                            # NULL w2 / k2 / beta / Mstruc
            ptrs = [p(W2), p(K2), p([0.3]), p(Ms)]
            ptrs[drop] = None
            rc = L.raftx_qtf_slender_resident(h, 1, 8, ptrs[0], ptrs[1], 200.0, 1025.0, 9.81, p(good[0].view(np.float64)), ptrs[2],
                                              ptrs[3], 0, None)
            assert rc != 0 and b"bad arguments" in L.raftx_last_error(h), drop
        with pytest.raises(RaftxError, match="nothing is resident"):       # Xi == NULL without first-order responses
            ctx.qtf_slender_resident(None, [0.3], W2, K2, 200.0, 1025.0, 9.81, Ms, Nm=0)
        assert ctx.last_kernel_ms() == ms                                # none of them ran a kernel
        # ... the tables are still there, and a valid call gives what it gave
        assert ctx.qtf_tables_counts()[1] == soff[-1]
        again = ctx.qtf_slender_resident(*good, Nm=0)
        assert np.array_equal(again.view(np.float64), ref.view(np.float64)) and np.any(ref)
        # Xi == NULL with resident responses of another pair count
        u = UNITS["OC3spar"]
        Z = np.zeros((1, 6, 6))
        M0 = np.asarray(u["M_struc"])[None]
        C0 = (np.asarray(u["C_struc"]) + np.diag([7e4, 7e4, 0, 0, 0, 1e8]))[None]
        ctx.build_designs(D.member_off, D.members, D.station_off, D.stations, M0, Z, C0, len(u["w"]), pose=pose, rho=u["rho"],
                          g=u["g"], k=u["k"], cap_off=D.cap_off, caps=D.caps, add_mask=3)
        ctx.upload_cases(u["w"], u["k"], 320.0, 1025.0, 9.81, np.full((1, 1, len(u["w"])), 0.3), np.array([[0.3]]))
        ctx.solve_dynamics_device(4, 0.01, 0.1)
        with pytest.raises(RaftxError, match="pairs are not these"):
            ctx.qtf_slender_resident(None, [0.3, 0.5], W2, K2, 320.0, 1025.0, 9.81, Ms, Nm=0)
        q = ctx.qtf_slender_resident(None, [0.3], W2, K2, 320.0, 1025.0, 9.81, Ms, Nm=0)
        assert np.all(np.isfinite(q.view(np.float64))) and np.any(q)
    finally:
        ctx.close()
