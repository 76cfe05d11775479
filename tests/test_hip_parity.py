"""GPU suite (-m gpu): the HIP library against the CPU oracle and the committed
golden vectors, all through the C-ABI.  fp64 end to end; gates are
group-relative 1e-9 (north_star asks 1e-6; SURVEY.md 8d expects ~1e-12)."""
import numpy as np
import pytest

from raft_amd import dropin
from raft_amd._abi import RaftxError
from tests.util import (group_rel_err, rel_err, case_from_fixture, load_model_fixture, ref_headings,
                        random_strips, random_matrices, synthetic_cases, add_mcf_rows)

pytestmark = pytest.mark.gpu
TOL = 1e-9
REFGOLD = ["refgold_OC3spar.npz", "refgold_VolturnUS-S.npz", "refgold_VolturnUS-S-pointInertia.npz",
           "refgold_OC4semi-WAMIT_Coefs.npz"]


def test_device_library_is_the_product(hip_lib):
    assert hip_lib.is_device and hip_lib.version == 100
    assert hip_lib.path.endswith("raft_amd/csrc/libraftx_hip.so")


@pytest.mark.parametrize("name", REFGOLD)
def test_reference_golden_hydroExcitation(name, hip_ctx):
    fx, model = load_model_fixture(name)
    eng = dropin.Engine(hip_ctx)
    fowt = model.fowtList[0]
    worst = 0.0
    for i, c in enumerate(fx["exc_cases"]):
        eng.calcHydroExcitation(fowt, dict(c), memberList=fowt.memberList)
        true = fx["exc_F_hydro_iner"][i]
        np.testing.assert_allclose(fowt.F_hydro_iner, true, rtol=1e-5, atol=1e-3)
        worst = max(worst, rel_err(fowt.F_hydro_iner, true))
    assert worst < TOL, worst


@pytest.mark.parametrize("name", REFGOLD)
def test_reference_golden_hydroLinearization(name, hip_ctx):
    fx, model = load_model_fixture(name)
    eng = dropin.Engine(hip_ctx)
    fowt = model.fowtList[0]
    case = {'wave_spectrum': 'unit', 'wave_heading': 0, 'wave_period': 10, 'wave_height': 2}
    eng.calcHydroExcitation(fowt, case, memberList=fowt.memberList)
    phase = np.linspace(0, 2 * np.pi, fowt.nw * fowt.nDOF).reshape(fowt.nDOF, fowt.nw)
    Xi = 0.1 * np.exp(1j * phase)
    B = eng.calcHydroLinearization(fowt, Xi)
    F = eng.calcDragExcitation(fowt, 0)
    np.testing.assert_allclose(B, fx["lin_B_hydro_drag"], rtol=1e-5, atol=1e-10)
    np.testing.assert_allclose(F, fx["lin_F_hydro_drag"], rtol=1e-5)
    assert rel_err(B, fx["lin_B_hydro_drag"]) < TOL
    assert rel_err(F, fx["lin_F_hydro_drag"]) < TOL


@pytest.mark.parametrize("name", ["c1_oc3spar.npz", "c2_volturnus.npz", "pose_volturnus_mcf.npz", "c4_farm.npz"])
def test_live_reference_solveDynamics(name, hip_ctx):
    fx, model = load_model_fixture(name)
    if "coupling_C" in fx:
        class _MS:
            def getCoupledStiffnessA(self, lines_only=True):
                return fx["coupling_C"]
        model.ms = _MS()
        model.moorMod = 0
    eng = dropin.Engine(hip_ctx)
    for c in fx["cases"]:
        Xi = eng.solveDynamics(model, case_from_fixture(c))
        Xr, nH = ref_headings(c)
        assert Xi.shape[0] == nH + 1 and np.all(Xi[nH] == 0)
        assert group_rel_err(Xi[:nH], Xr) < TOL
        for i, fowt in enumerate(model.fowtList):
            u = c["units"][i]
            assert int(model._raftx_niter[i]) == int(u["niter"])
            assert rel_err(fowt.B_hydro_drag, u["B_hydro_drag"]) < TOL
            if "Z" in u:                                   # lean cases of the many-case fixtures keep B_drag only
                assert rel_err(fowt.Z, u["Z"]) < TOL
                assert rel_err(fowt.F_hydro_iner, u["F_hydro_iner"]) < TOL


@pytest.mark.parametrize("name,nIter", [("c1_oc3spar.npz", 10), ("c2_volturnus.npz", 2), ("c4_farm.npz", 6)])
def test_dynamic_mooring_stepped_solve(name, nIter, hip_ctx, oracle_ctx):
    """moorMod == 2 (raft_model.py:1022-1030,1069-1072): one launch per iteration with the host's mooring-damping
    update in between; device vs oracle through the same drop-in code, same host call sequence (the NumPy path is
    compared with it on live objects in tests/test_dropin_live_reference.py)."""
    from tests.util import attach_fake_lines
    fx, m_gpu = load_model_fixture(name)
    _, m_cpu = load_model_fixture(name)
    for m in (m_gpu, m_cpu):
        m.nIter = nIter
        attach_fake_lines(m)
        if "coupling_C" in fx:
            class _MS:
                def getCoupledStiffnessA(self, lines_only=True):
                    return fx["coupling_C"]
            m.ms = _MS()
            m.moorMod = 0
    case = fx["cases"][0]
    Xi_gpu = dropin.Engine(hip_ctx).solveDynamics(m_gpu, case_from_fixture(case)).copy()
    Xi_cpu = dropin.Engine(oracle_ctx).solveDynamics(m_cpu, case_from_fixture(case)).copy()
    nH = Xi_gpu.shape[0] - 1
    assert group_rel_err(Xi_gpu[:nH], Xi_cpu[:nH]) < TOL
    assert np.array_equal(m_gpu._raftx_niter, m_cpu._raftx_niter)
    for fg, fc in zip(m_gpu.fowtList, m_cpu.fowtList):
        assert fg.ms.calls == fc.ms.calls and fg.ms.calls >= 3
        assert rel_err(fg.Z, fc.Z) < TOL
        assert rel_err(fg.B_hydro_drag, fc.B_hydro_drag) < TOL


@pytest.mark.parametrize("unit_lines", [False, True])
def test_array_level_dynamic_mooring(unit_lines, hip_ctx, oracle_ctx):
    """Array-level moorMod == 2 (raft_model.py:1173-1182): the shared lines' M + A, B, C -- linearised on the host about
    the motions the units' loops ended on (:1156,1178) -- enter the coupled 24-DOF solve as Mc, Bc, Cc of
    raftx_solve_system.  Device vs oracle through the same drop-in code (the NumPy path is compared with it on live
    objects in tests/test_dropin_live_reference.py); with unit-level dynamic lines too, the linearisation point comes from
    the stepped loop instead of the device's export."""
    from tests.util import attach_fake_lines, attach_fake_array_lines
    fx, m_gpu = load_model_fixture("c4_farm.npz")
    _, m_cpu = load_model_fixture("c4_farm.npz")
    for m in (m_gpu, m_cpu):
        m.nIter = 6
        if unit_lines:
            attach_fake_lines(m)
        attach_fake_array_lines(m)
    case = fx["cases"][1]
    Xi_gpu = dropin.Engine(hip_ctx).solveDynamics(m_gpu, case_from_fixture(case)).copy()
    Xi_cpu = dropin.Engine(oracle_ctx).solveDynamics(m_cpu, case_from_fixture(case)).copy()
    nH = Xi_gpu.shape[0] - 1
    assert m_gpu.ms.calls == 1 and m_cpu.ms.calls == 1
    assert m_gpu.ms.level == pytest.approx(m_cpu.ms.level, rel=1e-10) and m_gpu.ms.level > 0
    assert all(rel_err(a, b) < TOL for a, b in zip(m_gpu.ms.seen, m_cpu.ms.seen))
    assert group_rel_err(Xi_gpu[:nH], Xi_cpu[:nH]) < TOL
    # the coupling matters: without it the response is a different one
    fx0, m0 = load_model_fixture("c4_farm.npz")
    m0.nIter = 6
    Xi0 = dropin.Engine(oracle_ctx).solveDynamics(m0, case_from_fixture(case)).copy()
    assert group_rel_err(Xi_cpu[:nH], Xi0[:nH]) > 1e-3


def _both(hip_ctx, oracle_ctx, tables, mats, cases, depth=200.0):
    M0, B0, C0, MBw = mats
    w, k, zeta, beta = cases
    for ctx in (hip_ctx, oracle_ctx):
        ctx.upload_designs(tables, M0, B0, C0, len(w), MBw)
        ctx.upload_cases(w, k, depth, 1025.0, 9.81, zeta, beta)


@pytest.mark.parametrize("S_list,nw,nC,nH,fdep,mcf", [
    ([0, 1, 5], 7, 2, 1, False, 0.0),          # empty design, single strip, tiny nw
    ([63, 64, 65], 64, 1, 2, True, 0.3),       # around one wave of strips, freq-dependent M/B, MCF rows
    ([130, 17], 200, 2, 3, False, 0.2),        # ragged, three headings
    ([53], 256, 1, 1, True, 0.0),              # last size of the 2-wave shape
    ([26], 1, 1, 1, False, 0.0),               # single frequency bin
    ([40, 3], 100, 2, 1, False, 0.0),          # one wave, two bins per lane
    ([31], 300, 1, 2, False, 0.2),             # 4 waves x 2 bins per lane
    ([45, 9], 600, 1, 1, True, 0.0),           # 8 waves x 2 bins per lane
    ([22], 1100, 1, 1, False, 0.0),            # 8 waves x 3 bins per lane
    ([12], 2048, 1, 2, False, 0.0),            # maximum bins per workgroup (8 waves x 4)
])
def test_synthetic_parity(hip_ctx, oracle_ctx, S_list, nw, nC, nH, fdep, mcf):
    rng = np.random.default_rng(1234 + nw + len(S_list))
    tables = [random_strips(rng, S, nw, mcf) for S in S_list]
    mats = random_matrices(rng, len(S_list), nw, fdep)
    cases = synthetic_cases(rng, nC, nH, nw)
    _both(hip_ctx, oracle_ctx, tables, mats, cases)
    Fh, Fo = hip_ctx.excitation(), oracle_ctx.excitation()
    assert rel_err(Fh, Fo) < TOL
    Xi0 = 0.3 * (rng.normal(size=(len(S_list), nC, 6, nw)) + 1j * rng.normal(size=(len(S_list), nC, 6, nw)))
    Xi0[:, :, 3:] *= 0.02
    Bh, Fdh = hip_ctx.linearize(Xi0)
    Bo, Fdo = oracle_ctx.linearize(Xi0)
    assert rel_err(Bh, Bo) < TOL
    assert rel_err(Fdh, Fdo) < TOL
    Fe = 1e4 * (rng.normal(size=Fh.shape) + 1j * rng.normal(size=Fh.shape))
    oh = hip_ctx.solve_dynamics(8, 0.01, 0.1, F_extra=Fe, want_B=True, want_F=True, want_Z=True)
    oo = oracle_ctx.solve_dynamics(8, 0.01, 0.1, F_extra=Fe, want_B=True, want_F=True, want_Z=True)
    assert np.array_equal(oh["niter"], oo["niter"])
    assert np.array_equal(oh["flags"], oo["flags"])
    for d in range(len(S_list)):
        assert group_rel_err(oh["Xi"][d], oo["Xi"][d]) < TOL
    assert rel_err(oh["Z"], oo["Z"]) < TOL
    assert rel_err(oh["F_wave"], oo["F_wave"]) < TOL
    assert rel_err(oh["B_drag"], oo["B_drag"]) < TOL


@pytest.mark.parametrize("S_list,nw,nC", [([53, 44, 63, 0, 17], 200, 2), ([30], 64, 1), ([30, 31], 128, 3), ([20], 700, 1)])
def test_lean_sweep_kernel_parity(hip_ctx, oracle_ctx, S_list, nw, nC):
    """The specialisation the sweeps run (no optional inputs/outputs, results fetched from HBM)."""
    rng = np.random.default_rng(77 + nw)
    tables = [_member_run_table(rng, max(1, S // 10), 10) if S else random_strips(rng, 0) for S in S_list]
    mats = random_matrices(rng, len(S_list))
    cases = synthetic_cases(rng, nC, 1, nw)
    _both(hip_ctx, oracle_ctx, tables, mats, cases)
    res = []
    for ctx in (hip_ctx, oracle_ctx):
        ctx.solve_dynamics_device(6, 0.01, 0.1)
        res.append(ctx.fetch_results(want_Xi=True))
    assert np.array_equal(res[0]["niter"], res[1]["niter"])
    assert np.array_equal(res[0]["flags"], res[1]["flags"])
    for d in range(len(S_list)):
        assert group_rel_err(res[0]["Xi"][d], res[1]["Xi"][d]) < TOL


def test_c2_sea_states_as_one_batch(hip_ctx):
    """BASELINE configs[1]: the sea states of VolturnUS-S_example solved as ONE launch of the sweep kernel
    (cases axis), against the live-reference response of each case."""
    fx, model = load_model_fixture("c2_volturnus.npz")
    single = [c for c in fx["cases"] if np.isscalar(c["case"]["wave_heading"]) or len(np.atleast_1d(c["case"]["wave_heading"])) == 1]
    assert len(single) >= 3
    sweep = dropin.sweep_from_models([model], [case_from_fixture(c) for c in single])
    out = sweep.run(hip_ctx)
    assert out["Xi"].shape == (1, len(single), 1, 6, model.nw)
    for i, c in enumerate(single):
        assert int(out["niter"][0, i]) == int(c["units"][0]["niter"])
        assert group_rel_err(out["Xi"][0, i, :1], c["Xi"][:1]) < TOL
    st = sweep.run_stats(hip_ctx)
    f = model.fowtList[0]
    for i, c in enumerate(single):
        ref = np.sqrt(0.5 * np.sum(np.abs(c["Xi"][:1, 0, :]) ** 2))
        assert abs(st["std"][0, i, 0] - ref) < 1e-9 * ref


def test_c4_farm_as_one_batch(hip_ctx, oracle_ctx):
    """BASELINE configs[3]: 4-unit array, all sea states in one batch: per-unit fixed points (one launch) +
    coupled 24x24 solves fed from the resident Z / F_wave (second launch)."""
    fx, model = load_model_fixture("c4_farm.npz")
    sweep = dropin.sweep_from_units(model, [case_from_fixture(c) for c in fx["cases"]])
    out = sweep.run_farm(hip_ctx, 4, Cc=fx["coupling_C"][None])
    ref = sweep.run_farm(oracle_ctx, 4, Cc=fx["coupling_C"][None])
    assert np.array_equal(out["niter"], ref["niter"])
    assert len(fx["cases"]) == 50 and out["Xi"].shape == (1, 50, 1, 24, 200)      # configs[3]: 4 units x 50 sea states x 200 bins
    for i, c in enumerate(fx["cases"]):
        Xr, nH = ref_headings(c)
        assert group_rel_err(out["Xi"][0, i, :nH], Xr) < TOL
        assert group_rel_err(out["Xi"][0, i], ref["Xi"][0, i]) < TOL
        assert [int(out["niter"][u, i]) for u in range(4)] == [int(c["units"][u]["niter"]) for u in range(4)]


@pytest.mark.parametrize("n_unit,n_head,nw", [(4, 1, 200), (2, 2, 200), (3, 3, 200), (6, 1, 200), (2, 1, 96)])
def test_farm_path_without_Z_is_bit_identical_to_the_path_that_exports_it(hip_ctx, oracle_ctx, n_unit, n_head, nw):
    """Sweep.run_farm on units with constant matrices: the fixed points run as the LEAN kernel (two waves per SIMD in the
    200-bin shape) exporting only F_wave and B_drag, and the coupled solve assembles every unit's 6 x 6 impedance itself
    (k_solve_system_rows<.., ASM>; for shapes without a register-resident solver k_assemble_unit_z + the LDS solver) --
    the same bits as the path that exports Z from the full-featured kernel and reads it back, and the oracle's numbers."""
    from raft_amd._abi import WANT_FWAVE, WANT_Z
    from raft_amd.sweep import Sweep
    rng = np.random.default_rng(77 + n_unit + n_head)
    nG = 3
    tables = [random_strips(rng, S, nw, 0.0) for S in rng.integers(8, 60, size=nG * n_unit)]
    M0, B0, C0, _ = random_matrices(rng, nG * n_unit, nw, False)
    w, k, zeta, beta = synthetic_cases(rng, 2, n_head, nw)
    off = np.concatenate([[0], np.cumsum([len(t.strips) for t in tables])]).astype(np.int64)
    sweep = Sweep(off, np.concatenate([t.strips for t in tables]), M0, B0, C0, w, k, 200.0, zeta, beta, 5, 0.1)
    n = 6 * n_unit
    Cc = rng.normal(size=(nG, n, n)) * 1e5
    Cc = Cc + np.transpose(Cc, (0, 2, 1))
    Bc, Mc = 1e3 * rng.normal(size=(nG, n, n)), 1e4 * rng.normal(size=(nG, n, n))
    lean = sweep.run_farm(hip_ctx, n_unit, Cc=Cc, Mc=Mc, Bc=Bc)
    sweep.upload(hip_ctx)
    hip_ctx.solve_dynamics_device(sweep.nIter, sweep.tol, sweep.XiStart, want_mask=WANT_Z | WANT_FWAVE)
    flags_full, _, _ = hip_ctx.last_solve_kernel()
    full = hip_ctx.solve_system_resident(n_unit, Mc, Bc, Cc)
    assert np.array_equal(lean["Xi"].view(np.uint64), full.view(np.uint64))
    sweep.upload(hip_ctx)
    from raft_amd._abi import WANT_BDRAG
    hip_ctx.solve_dynamics_device(sweep.nIter, sweep.tol, sweep.XiStart, want_mask=WANT_BDRAG | WANT_FWAVE)
    flags_lean, waves_lean, _ = hip_ctx.last_solve_kernel()
    assert flags_full == 127
    if nw == 200:                                       # the shape with lean specialisations: F_wave export (4), + headings (32)
        assert flags_lean == (4 | (32 if n_head > 1 else 0)) and waves_lean == 2
    ref = sweep.run_farm(oracle_ctx, n_unit, Cc=Cc, Mc=Mc, Bc=Bc)
    assert np.array_equal(lean["niter"], ref["niter"])
    assert rel_err(lean["Xi"], ref["Xi"]) < TOL


@pytest.mark.gpu
def test_lean_farm_after_a_wider_export_does_not_read_the_stale_impedances(hip_ctx, oracle_ctx):
    """a solve that exported Z leaves its buffer allocated; a same-shape Sweep.run_farm that follows on the
    same context asks only for B_drag | F_wave, the buffers are kept (superset) and Z is NOT rewritten -- the coupled solve
    must assemble the impedances of the NEW designs, not read the old ones, and fetching Z must fail."""
    from raft_amd._abi import WANT_FWAVE, WANT_Z, WANT_BDRAG, RaftxError
    from raft_amd.sweep import Sweep
    rng = np.random.default_rng(505)
    n_unit, nG, nw = 2, 2, 200
    w, k, zeta, beta = synthetic_cases(rng, 2, 1, nw)
    S_list = rng.integers(8, 60, size=nG * n_unit)

    def make(seed):
        r = np.random.default_rng(seed)
        tables = [random_strips(r, S, nw, 0.0) for S in S_list]                     # same strip counts: same buffer shapes
        M0, B0, C0, _ = random_matrices(r, nG * n_unit, nw, False)
        off = np.concatenate([[0], np.cumsum([len(t.strips) for t in tables])]).astype(np.int64)
        return Sweep(off, np.concatenate([t.strips for t in tables]), M0, B0, C0, w, k, 200.0, zeta, beta, 5, 0.1)
    first, second = make(1), make(2)
    n = 6 * n_unit
    Cc = rng.normal(size=(nG, n, n)) * 1e5
    Cc = Cc + np.transpose(Cc, (0, 2, 1))
    first.upload(hip_ctx)
    hip_ctx.solve_dynamics_device(first.nIter, first.tol, first.XiStart, want_mask=WANT_Z | WANT_FWAVE | WANT_BDRAG)
    out = second.run_farm(hip_ctx, n_unit, Cc=Cc)                                   # B_drag | F_wave: a subset, nothing reallocated
    ref = second.run_farm(oracle_ctx, n_unit, Cc=Cc)
    assert np.array_equal(out["niter"], ref["niter"])
    assert rel_err(out["Xi"], ref["Xi"]) < TOL
    with pytest.raises(RaftxError):
        hip_ctx.fetch_results(want_Xi=False, want_Z=True)


@pytest.mark.parametrize("name,icase", [("c2_volturnus.npz", 4), ("pose_volturnus_mcf.npz", 1), ("c4_farm.npz", 0)])
def test_materialised_members_through_the_dropin(name, icase, hip_ctx, oracle_ctx):
    """Engine(materialise_members=True): after solveDynamics every member of every unit carries u, ud, pDyn [nWaves,ns,3,nw],
    Bmat [ns,3,3] of the linearisation the loop exited with and F_exc_drag of the last heading (raft_member.py:1927-1937,
    2117, 2122; raft_model.py:1063, 1214) -- device vs oracle through the same drop-in code on the stand-in units (live
    reference objects: tests/test_dropin_live_reference.py); two headings, MacCamy-Fuchs columns at a mean pose, a farm."""
    fx, m_gpu = load_model_fixture(name)
    _, m_cpu = load_model_fixture(name)
    case = fx["cases"][icase]
    if "coupling_C" in fx:
        for m in (m_gpu, m_cpu):
            class _MS:
                def getCoupledStiffnessA(self, lines_only=True):
                    return fx["coupling_C"]
            m.ms, m.moorMod = _MS(), 0
    Xg = dropin.Engine(hip_ctx, materialise_members=True).solveDynamics(m_gpu, case_from_fixture(case)).copy()
    Xc = dropin.Engine(oracle_ctx, materialise_members=True).solveDynamics(m_cpu, case_from_fixture(case)).copy()
    nH = Xg.shape[0] - 1
    assert group_rel_err(Xg[:nH], Xc[:nH]) < TOL
    wet = 0
    for fg, fc in zip(m_gpu.fowtList, m_cpu.fowtList):
        for a, b in zip(fg.memberList, fc.memberList):
            assert a.u.shape == (nH, a.ns, 3, m_gpu.nw) and a.Bmat.shape == (a.ns, 3, 3) and a.F_exc_drag.shape == (a.ns, 3, m_gpu.nw)
            if np.any(b.u):
                wet += 1
                assert rel_err(a.u, b.u) < 1e-12 and rel_err(a.ud, b.ud) < 1e-12 and rel_err(a.pDyn, b.pDyn) < 1e-12
                assert rel_err(a.Bmat, b.Bmat) < 1e-9 and rel_err(a.F_exc_drag, b.F_exc_drag) < 1e-9
            dry = np.asarray(a.r)[:, 2] >= 0
            assert not np.any(a.u[:, dry]) and not np.any(a.Bmat[dry])
    assert wet >= 2


@pytest.mark.parametrize("S_list,nw,nH,mcf", [([40, 7], 200, 2, 0.0), ([53], 300, 1, 0.3), ([5, 0, 12], 48, 3, 0.0)])
def test_strip_exports_parity(hip_ctx, oracle_ctx, S_list, nw, nH, mcf):
    """raftx_strip_kinematics / raftx_strip_drag (what the reference keeps on its Member objects: u, ud, pDyn,
    raft_member.py:1927-1937; Bmat, F_exc_drag, :2117,2122), device vs oracle per strip, every design and sea state of
    the resident set; and consistent with the device's own linearisation: sum_s translate(Bmat_s) = B_drag."""
    rng = np.random.default_rng(31 + nw)
    tables = [random_strips(rng, S, nw, mcf) for S in S_list]
    mats = random_matrices(rng, len(S_list), nw, False)
    cases = synthetic_cases(rng, 2, nH, nw)
    _both(hip_ctx, oracle_ctx, tables, mats, cases)
    Xi = (rng.normal(size=(len(S_list), 2, 6, nw)) + 1j * rng.normal(size=(len(S_list), 2, 6, nw))) * \
        np.array([1.0, 1.0, 1.0, 0.02, 0.02, 0.02])[None, None, :, None]
    Bd, _ = hip_ctx.linearize(Xi)
    for d, S in enumerate(S_list):
        for ic in range(2):
            g, o = hip_ctx.strip_kinematics(d, S, icase=ic), oracle_ctx.strip_kinematics(d, S, icase=ic)
            for a, b in zip(g, o):
                assert a.shape == b.shape
                if S:
                    assert rel_err(a, b) < 1e-12
            for ih in range(nH):
                Bg, Fg = hip_ctx.strip_drag(d, S, Xi[d, ic], ih=ih, icase=ic)
                Bo, Fo = oracle_ctx.strip_drag(d, S, Xi[d, ic], ih=ih, icase=ic)
                if S:
                    assert rel_err(Bg, Bo) < 1e-11 and rel_err(Fg, Fo) < 1e-11
            if S:                                        # translateMatrix3to6DOF summed over the strips (raft_member.py:2118)
                from raft_amd.strips import F_AX
                tot = np.zeros((6, 6))
                for s in range(S):
                    r = tables[d].strips[s, F_AX:F_AX + 3]
                    H = np.array([[0, r[2], -r[1]], [-r[2], 0, r[0]], [r[1], -r[0], 0]])
                    tot[:3, :3] += Bg[s]
                    tot[:3, 3:] += Bg[s] @ H
                    tot[3:, :3] += H.T @ Bg[s]
                    tot[3:, 3:] += H.T @ Bg[s] @ H
                assert rel_err(tot, Bd[d, ic]) < 1e-10
    from raft_amd._abi import RaftxError
    with pytest.raises(RaftxError):
        hip_ctx.strip_kinematics(len(S_list), 1)
    with pytest.raises(RaftxError):
        hip_ctx.strip_drag(0, S_list[0], Xi[0, 0], ih=nH)


def test_resident_system_solve_many_groups(hip_ctx, oracle_ctx):
    """Three arrays of two synthetic units x 3 cases x 2 headings, full coupling matrices."""
    rng = np.random.default_rng(404)
    tables = [random_strips(rng, S) for S in (20, 31, 9, 40, 17, 25)]
    mats = random_matrices(rng, 6)
    cases = synthetic_cases(rng, 3, 2, 48)
    _both(hip_ctx, oracle_ctx, tables, mats, cases)
    n = 12
    Cc = rng.normal(size=(3, n, n)) * 1e5
    Cc = Cc + np.transpose(Cc, (0, 2, 1))
    Bc = 1e3 * rng.normal(size=(3, n, n))
    Mc = 1e4 * rng.normal(size=(3, n, n))
    res = []
    for ctx in (hip_ctx, oracle_ctx):
        ctx.solve_dynamics_device(5, 0.01, 0.1, want_mask=6)
        res.append(ctx.solve_system_resident(2, Mc, Bc, Cc))
    assert res[0].shape == (3, 3, 2, 12, 48)
    assert rel_err(res[0], res[1]) < TOL


def test_motion_stats_parity(hip_ctx, oracle_ctx):
    rng = np.random.default_rng(5150)
    tables = [random_strips(rng, S) for S in (40, 53, 7)]
    mats = random_matrices(rng, 3)
    cases = synthetic_cases(rng, 2, 3, 200)
    _both(hip_ctx, oracle_ctx, tables, mats, cases)
    out = []
    for ctx in (hip_ctx, oracle_ctx):
        ctx.solve_dynamics_device(5, 0.01, 0.1)
        out.append(ctx.motion_stats(0.031, want_psd=True))
    assert rel_err(out[0][0], out[1][0]) < TOL
    assert rel_err(out[0][1], out[1][1]) < TOL
    std_only, none = hip_ctx.motion_stats(0.031)
    assert none is None and np.array_equal(std_only, out[0][0])


def test_channel_stats_parity(hip_ctx, oracle_ctx):
    rng = np.random.default_rng(808)
    tables = [random_strips(rng, S) for S in (40, 53, 7)]
    mats = random_matrices(rng, 3)
    cases = synthetic_cases(rng, 2, 2, 200)
    _both(hip_ctx, oracle_ctx, tables, mats, cases)
    L = rng.normal(size=(3, 5, 6)) * np.array([1, 1, 1, 50, 50, 50])
    pw = [0, 2, 2, 1, 4]
    out = []
    for ctx in (hip_ctx, oracle_ctx):
        ctx.solve_dynamics_device(5, 0.01, 0.1)
        out.append(ctx.channel_stats(L, pw, 0.031, want_psd=True))
    assert rel_err(out[0][0], out[1][0]) < TOL
    assert rel_err(out[0][1], out[1][1]) < TOL


def test_channel_stats_poly_parity(hip_ctx, oracle_ctx):
    """Mixed displacement / velocity / acceleration channels with a complex frequency-dependent transfer (the
    tower-base moment pattern, raft_fowt.py:2500-2537); nw = 90 exercises the ragged last wave."""
    rng = np.random.default_rng(909)
    tables = [random_strips(rng, S) for S in (40, 53, 7)]
    mats = random_matrices(rng, 3)
    cases = synthetic_cases(rng, 2, 2, 90)
    _both(hip_ctx, oracle_ctx, tables, mats, cases)
    L = rng.normal(size=(3, 4, 3, 6)) * np.array([1, 1, 1, 50, 50, 50])
    Gw = rng.normal(size=(3, 4, 6, 90)) + 1j * rng.normal(size=(3, 4, 6, 90))
    out, out_nog = [], []
    for ctx in (hip_ctx, oracle_ctx):
        ctx.solve_dynamics_device(5, 0.01, 0.1)
        out.append(ctx.channel_stats_poly(L, 0.031, Gw=Gw, want_psd=True))
        out_nog.append(ctx.channel_stats_poly(L, 0.031))
    assert rel_err(out[0][0], out[1][0]) < TOL and rel_err(out[0][1], out[1][1]) < TOL
    assert rel_err(out_nog[0][0], out_nog[1][0]) < TOL and out_nog[0][1] is None
    # pure powers reproduce raftx_channel_stats
    Lp = np.zeros((3, 2, 3, 6))
    Lp[:, 0, 0] = L[:, 0, 0]
    Lp[:, 1, 2] = L[:, 1, 2]
    a, _ = hip_ctx.channel_stats_poly(Lp, 0.031)
    b, _ = hip_ctx.channel_stats(np.stack([L[:, 0, 0], L[:, 1, 2]], axis=1), [0, 2], 0.031)
    assert rel_err(a, b) < 1e-12


def test_repeat_runs_are_bitwise_identical(hip_ctx):
    rng = np.random.default_rng(7)
    tables = [random_strips(rng, 53) for _ in range(4)]
    M0, B0, C0, _ = random_matrices(rng, 4)
    w, k, zeta, beta = synthetic_cases(rng, 3, 1, 200)
    hip_ctx.upload_designs(tables, M0, B0, C0, 200)
    hip_ctx.upload_cases(w, k, 200.0, 1025.0, 9.81, zeta, beta)
    a = hip_ctx.solve_dynamics(6, want_Z=True)
    b = hip_ctx.solve_dynamics(6, want_Z=True)
    assert np.array_equal(a["Xi"].view(np.uint64), b["Xi"].view(np.uint64))
    assert np.array_equal(a["Z"].view(np.uint64), b["Z"].view(np.uint64))
    assert np.array_equal(a["niter"], b["niter"])


def test_excitation_is_linear_in_wave_amplitude(hip_ctx):
    """Size-independent property at the full C2 shape: F_iner(a*zeta) = a*F_iner(zeta)."""
    rng = np.random.default_rng(11)
    tables = [random_strips(rng, 53) for _ in range(8)]
    M0, B0, C0, _ = random_matrices(rng, 8)
    w, k, zeta, beta = synthetic_cases(rng, 2, 2, 200)
    hip_ctx.upload_designs(tables, M0, B0, C0, 200)
    hip_ctx.upload_cases(w, k, 200.0, 1025.0, 9.81, zeta, beta)
    F1 = hip_ctx.excitation()
    hip_ctx.upload_cases(w, k, 200.0, 1025.0, 9.81, 2.0 * zeta, beta)
    F2 = hip_ctx.excitation()
    assert rel_err(F2, 2.0 * F1) < 1e-14


def test_still_water_gives_zero_response(hip_ctx):
    rng = np.random.default_rng(3)
    tables = [random_strips(rng, 20)]
    M0, B0, C0, _ = random_matrices(rng, 1)
    w, k, zeta, beta = synthetic_cases(rng, 1, 1, 50)
    hip_ctx.upload_designs(tables, M0, B0, C0, 50)
    hip_ctx.upload_cases(w, k, 200.0, 1025.0, 9.81, 0.0 * zeta, beta)
    out = hip_ctx.solve_dynamics(4, XiStart=0.0)
    assert np.all(out["Xi"] == 0)
    assert out["niter"][0, 0] == 1 and out["flags"][0, 0] == 1


def test_singular_system_is_flagged_not_hidden(hip_ctx, oracle_ctx):
    """All-zero M/B/C with no strips: Z is singular -> NaN flag (the reference raises, raft_model.py:1098)."""
    rng = np.random.default_rng(5)
    tables = [random_strips(rng, 0)]
    Z6 = np.zeros((1, 6, 6))
    w, k, zeta, beta = synthetic_cases(rng, 1, 1, 16)
    Fe = np.ones((1, 1, 1, 6, 16), dtype=complex)
    for ctx in (hip_ctx, oracle_ctx):
        ctx.upload_designs(tables, Z6, Z6, Z6, 16)
        ctx.upload_cases(w, k, 200.0, 1025.0, 9.81, zeta, beta)
        out = ctx.solve_dynamics(2, F_extra=Fe)
        assert out["flags"][0, 0] & 2


def test_deep_water_and_zero_wavenumber_branches(hip_ctx, oracle_ctx):
    """helpers.py:211-222: k==0 and k*h>89.4 branches."""
    rng = np.random.default_rng(9)
    tables = [random_strips(rng, 12)]
    mats = random_matrices(rng, 1)
    nw = 8
    w = np.linspace(0.0, 3.5, nw)
    k = w * w / 9.81
    k[0] = 0.0
    zeta = np.full((1, 1, nw), 0.5)
    beta = np.array([[0.4]])
    for depth in (200.0, 2000.0):
        _both(hip_ctx, oracle_ctx, tables, mats, (w, k, zeta, beta), depth=depth)
        assert rel_err(hip_ctx.excitation(), oracle_ctx.excitation()) < TOL


def test_bins_beyond_workgroup_capacity_fail_loudly(hip_ctx):
    rng = np.random.default_rng(2)
    w, k, zeta, beta = synthetic_cases(rng, 1, 1, 3000)
    with pytest.raises(RaftxError):
        hip_ctx.upload_cases(w, k, 200.0, 1025.0, 9.81, zeta, beta)


@pytest.mark.parametrize("nUnit,nRhs,nw,coupled", [(1, 1, 5, False), (4, 2, 50, True), (10, 3, 7, True)])
def test_solve_system_parity(hip_ctx, oracle_ctx, nUnit, nRhs, nw, coupled):
    rng = np.random.default_rng(100 + nUnit)
    nS, n = 3, 6 * nUnit
    w = np.linspace(0.1, 1.5, nw)
    Zblk = rng.normal(size=(nS, nUnit, 6, 6, nw)) + 1j * rng.normal(size=(nS, nUnit, 6, 6, nw))
    Zblk += 8.0 * np.eye(6)[None, None, :, :, None]
    F = rng.normal(size=(nS, nRhs, n, nw)) + 1j * rng.normal(size=(nS, nRhs, n, nw))
    Mc = Bc = Cc = None
    if coupled:
        Cc = rng.normal(size=(nS, n, n))
        Cc = Cc + np.transpose(Cc, (0, 2, 1))
        Bc = 0.1 * rng.normal(size=(nS, n, n))
        Mc = 0.1 * rng.normal(size=(nS, n, n))
    Xh = hip_ctx.solve_system(w, Zblk, F, Mc, Bc, Cc)
    Xo = oracle_ctx.solve_system(w, Zblk, F, Mc, Bc, Cc)
    assert rel_err(Xh, Xo) < TOL
    # independent check with LAPACK
    for s in range(nS):
        for i in range(nw):
            A = np.zeros((n, n), dtype=complex)
            for u in range(nUnit):
                A[6 * u:6 * u + 6, 6 * u:6 * u + 6] = Zblk[s, u, :, :, i]
            if coupled:
                A += -w[i] ** 2 * Mc[s] + 1j * w[i] * Bc[s] + Cc[s]
            X = np.linalg.solve(A, F[s, :, :, i].T).T
            assert rel_err(Xh[s, :, :, i], X) < 1e-9


def test_device_sincos_exp_accuracy(hip_ctx):
    """The kernels' own straight-line fp64 sincos/exp vs libm: <= 4 ulp-ish over the problem's range."""
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-50, 50, 20000), rng.uniform(-5000, 5000, 20000),
                        np.linspace(-1e-3, 1e-3, 101), [0.0, np.pi / 4, -np.pi / 4, np.pi / 2, 1e5, -1e5]])
    for table in (False, True):          # straight-line polynomials; the table-driven form of the fused kernel's run starts
        s, c, _ = hip_ctx.debug_math(x, table=table)
        assert np.max(np.abs(s - np.sin(x))) < 4e-16
        assert np.max(np.abs(c - np.cos(x))) < 4e-16
    xe = np.concatenate([rng.uniform(-700, 0, 20000), rng.uniform(0, 60, 20000), [0.0, -1e-300, 1e-9, -745.0]])
    _, _, e = hip_ctx.debug_math(xe)
    ref = np.exp(np.maximum(xe, -740.0))
    assert np.max(np.abs(e - ref) / ref) < 5e-16


def _member_run_table(rng, n_members=6, n_per=14):
    """Strips laid out along straight members with (1,2,4)-multiples of a unit spacing:
    exercises the rotor recurrence (RAFTX_F_STEP/UNIT) incl. vertical and horizontal members."""
    from raft_amd import strips as st
    base = random_strips(rng, n_members * n_per)
    rec = base.strips
    for mbr in range(n_members):
        A = np.array([rng.uniform(-40, 40), rng.uniform(-40, 40), rng.uniform(-28, -22)])
        if mbr == 0:
            q = np.array([0.0, 0.0, 1.0])
        elif mbr == 1:
            q = np.array([np.cos(0.7), np.sin(0.7), 0.0])
        else:
            q = rng.normal(size=3)
            q[2] = abs(q[2]) * 0.1
            q /= np.linalg.norm(q)
        B = np.linalg.qr(np.column_stack([q, rng.normal(size=3), rng.normal(size=3)]))[0]
        p1 = B[:, 1] - q * (q @ B[:, 1])
        p1 /= np.linalg.norm(p1)
        p2 = np.cross(q, p1)
        unit = rng.uniform(0.2, 0.6)
        pos = 0.0
        for j in range(n_per):
            i = mbr * n_per + j
            step = 0 if j == 0 else int(rng.choice([1, 2, 2, 4]))
            pos += step * unit
            r = A + pos * q
            rec[i, st.F_AX:st.F_AX + 3] += r - rec[i, st.F_X:st.F_X + 3]
            rec[i, st.F_X:st.F_X + 3] = r
            rec[i, st.F_Q:st.F_Q + 3] = q
            rec[i, st.F_P1:st.F_P1 + 3] = p1
            rec[i, st.F_P2:st.F_P2 + 3] = p2
            rec[i, st.F_STEP] = step
            rec[i, st.F_UNIT] = unit
        assert rec[mbr * n_per + n_per - 1, st.F_X + 2] < 0, "synthetic member left the water"
    return base


def test_member_runs_use_rotors_and_match_exact_evaluation(hip_ctx, oracle_ctx):
    rng = np.random.default_rng(21)
    tables = [_member_run_table(rng) for _ in range(3)]
    mats = random_matrices(rng, 3)
    cases = synthetic_cases(rng, 2, 2, 200)
    _both(hip_ctx, oracle_ctx, tables, mats, cases)
    assert rel_err(hip_ctx.excitation(), oracle_ctx.excitation()) < TOL
    oh = hip_ctx.solve_dynamics(8, want_B=True, want_F=True)
    oo = oracle_ctx.solve_dynamics(8, want_B=True, want_F=True)
    assert np.array_equal(oh["niter"], oo["niter"])
    for d in range(3):
        assert group_rel_err(oh["Xi"][d], oo["Xi"][d]) < TOL
    assert rel_err(oh["F_wave"], oo["F_wave"]) < TOL
    # the same tables with the hints stripped (every strip evaluated exactly) agree to round-off
    from raft_amd import strips as st
    from raft_amd.strips import StripTable
    plain = []
    for t in tables:
        r = t.strips.copy()
        r[:, st.F_STEP] = 0
        plain.append(StripTable(r))
    M0, B0, C0, _ = mats
    hip_ctx.upload_designs(plain, M0, B0, C0, 200)
    op = hip_ctx.solve_dynamics(8)
    for d in range(3):
        assert group_rel_err(op["Xi"][d], oh["Xi"][d]) < 1e-12


def _oriented_run_table(rng, axes, n_per=9):
    """Members along the given axes (None = one-strip members with random triads), circular and rectangular mixed."""
    from raft_amd import strips as st
    n = sum(n_per if a is not None else 3 for a in axes)
    base = random_strips(rng, n)
    rec = base.strips
    i = 0
    for a in axes:
        if a is None:                       # three unrelated strips: runs of one
            i += 3
            continue
        upright = len(a) == 4                # (x, y, 0, "up"): a pontoon -- rectangular, p1 = +-z (DSI_AXAL)
        q = np.asarray(a[:3], dtype=float)
        q = q / np.linalg.norm(q)
        h = np.array([0.0, 0.0, 1.0]) if abs(q[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
        p1 = np.cross(h, q)
        p1 /= np.linalg.norm(p1)
        p2 = np.cross(q, p1)
        if upright:
            p1 = np.array([0.0, 0.0, -1.0 if i % 2 else 1.0])
            p2 = np.cross(q, p1)
        A = np.array([rng.uniform(-30, 30), rng.uniform(-30, 30), rng.uniform(-28, -22)])
        unit, pos = rng.uniform(0.3, 0.7), 0.0
        for j in range(n_per):
            pos += 0 if j == 0 else int(rng.choice([1, 2])) * unit
            r = A + pos * q
            rec[i, st.F_AX:st.F_AX + 3] += r - rec[i, st.F_X:st.F_X + 3]
            rec[i, st.F_X:st.F_X + 3] = r
            rec[i, st.F_Q:st.F_Q + 3], rec[i, st.F_P1:st.F_P1 + 3], rec[i, st.F_P2:st.F_P2 + 3] = q, p1, p2
            rec[i, st.F_CIRC] = 0.0 if upright else float(j % 3 != 0)
            i += 1
    return base


@pytest.mark.parametrize("nw,nH", [(200, 1), (200, 2), (64, 1), (300, 1)])
def test_run_type_loops_of_the_lean_kernel(hip_ctx, oracle_ctx, nw, nH):
    """The sweeps iterate over runs with inner loops specialised by run type (vertical / horizontal / inclined):
    every type, runs of one strip, a horizontal member square to the waves (no phase rotation without being vertical),
    members pointing down and against the axes, circular and rectangular strips, two sea states -- lean kernel (one heading) and the multi-heading one vs the oracle."""
    rng = np.random.default_rng(77 + nw)
    axes_a = [(0, 0, 1), (1, 0, 0), (0, 1, 0), None, (0.3, -0.5, 0.4), (0, 0, -1), (-1, 0, 0), (0.6, 0.8, 0), (0, 0, 1)]
    axes_b = [None, (0, -1, 0), (0, 0, 1), (0.2, 0.1, -0.9), None]
    # upright pontoons in several directions -- one of them square to the waves of the first sea state: no phase rotation
    # without being vertical, it takes the pontoon loops with the identity rotor -- beside vertical columns (the shape of C3)
    axes_c = [(1, 0, 0, "up"), (0, 0, 1), (0.6, 0.8, 0, "up"), (0, 1, 0, "up"), (0, 0, 1), (-0.5, 0.866, 0, "up")]
    tables = [_oriented_run_table(rng, axes_a), _oriented_run_table(rng, axes_b), _oriented_run_table(rng, axes_c, n_per=12)]
    mats = random_matrices(rng, 3)
    w, k, zeta, beta = synthetic_cases(rng, 2, nH, nw)
    beta = np.array([[0.0, 1.1], [0.4, -2.0]])[:, :nH]    # sin(0) = 0 exactly: the y-aligned member gets no phase rotation
    _both(hip_ctx, oracle_ctx, tables, mats, (w, k, zeta, beta))
    oh = hip_ctx.solve_dynamics(6)                         # no optional outputs: with one heading the lean specialisation
    oo = oracle_ctx.solve_dynamics(6)
    assert np.array_equal(oh["niter"], oo["niter"])
    assert np.array_equal(oh["flags"], oo["flags"])
    for d in range(3):
        assert group_rel_err(oh["Xi"][d], oo["Xi"][d]) < TOL
    B, F = hip_ctx.linearize(oo["Xi"][:, :, 0])             # k_linearize shares the pass-A / pass-B loops
    Bo, Fo = oracle_ctx.linearize(oo["Xi"][:, :, 0])
    assert rel_err(B, Bo) < TOL and rel_err(F, Fo) < TOL


def test_collinear_members_with_different_sections_do_not_share_a_run(hip_ctx, oracle_ctx):
    """The sweeps load the unit triad once per run and pick the run's inner loop from its first strip, so the library
    must start a new run where collinear, equally spaced members differ in their cross-section axes or shape
    (derive_design_tables): three members end to end on one horizontal line and on one vertical line -- rectangular,
    the same twisted by 35 degrees, circular."""
    from raft_amd import strips as st
    rng = np.random.default_rng(5)
    n_per = 5
    tabs = []
    for q in (np.array([0.6, 0.8, 0.0]), np.array([0.0, 0.0, 1.0])):
        base = random_strips(rng, 3 * n_per)
        rec = base.strips
        h = np.array([0.0, 0.0, 1.0]) if abs(q[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
        p1 = np.cross(h, q) / np.linalg.norm(np.cross(h, q))
        p2 = np.cross(q, p1)
        A = np.array([3.0, -7.0, -26.0])
        for i in range(3 * n_per):
            mbr = i // n_per
            r = A + 0.5 * (i + 1) * q                  # one spacing all along the line
            ang = 0.0 if mbr != 1 else np.deg2rad(35.0)
            rec[i, st.F_AX:st.F_AX + 3] += r - rec[i, st.F_X:st.F_X + 3]
            rec[i, st.F_X:st.F_X + 3] = r
            rec[i, st.F_Q:st.F_Q + 3] = q
            rec[i, st.F_P1:st.F_P1 + 3] = np.cos(ang) * p1 + np.sin(ang) * p2
            rec[i, st.F_P2:st.F_P2 + 3] = -np.sin(ang) * p1 + np.cos(ang) * p2
            rec[i, st.F_CIRC] = float(mbr == 2)
        tabs.append(base)
    mats = random_matrices(rng, 2)
    cases = synthetic_cases(rng, 1, 1, 200)
    _both(hip_ctx, oracle_ctx, tabs, mats, cases)
    oh = hip_ctx.solve_dynamics(6)
    oo = oracle_ctx.solve_dynamics(6)
    assert np.array_equal(oh["niter"], oo["niter"])
    for d in range(2):
        assert group_rel_err(oh["Xi"][d], oo["Xi"][d]) < TOL
    B, F = hip_ctx.linearize(oo["Xi"][:, :, 0])
    Bo, Fo = oracle_ctx.linearize(oo["Xi"][:, :, 0])
    assert rel_err(B, Bo) < TOL and rel_err(F, Fo) < TOL


def test_arms_that_do_not_follow_the_positions_get_no_runs(hip_ctx, oracle_ctx):
    """The run-type loops keep arm components that cannot change along a run's axis out of the strip loop; a table whose
    arms are not position minus one reference point (the C-ABI does not forbid it) must therefore not form runs."""
    from raft_amd import strips as st
    rng = np.random.default_rng(9)
    axes = [(0, 0, 1), (1, 0, 0), (0.6, 0.8, 0)]
    tab = _oriented_run_table(rng, axes, n_per=7)
    tab.strips[:, st.F_AX:st.F_AX + 3] += rng.normal(scale=0.3, size=(tab.strips.shape[0], 3))     # per-strip offsets
    mats = random_matrices(rng, 1)
    w, k, zeta, beta = synthetic_cases(rng, 1, 1, 200)
    _both(hip_ctx, oracle_ctx, [tab], mats, (w, k, zeta, np.array([[0.0]])))
    oh, oo = hip_ctx.solve_dynamics(6), oracle_ctx.solve_dynamics(6)
    assert np.array_equal(oh["niter"], oo["niter"])
    assert group_rel_err(oh["Xi"][0], oo["Xi"][0]) < TOL


def test_bad_run_hints_are_demoted_not_trusted(hip_ctx, oracle_ctx):
    """A wrong STEP/UNIT hint must not change results (verified at upload)."""
    from raft_amd import strips as st
    rng = np.random.default_rng(22)
    t = _member_run_table(rng, 3, 10)
    t.strips[5, st.F_STEP] = 3          # inconsistent with the actual spacing
    t.strips[17, st.F_UNIT] = 9.0
    t.strips[0, st.F_STEP] = 2          # first strip can never be a step
    mats = random_matrices(rng, 1)
    cases = synthetic_cases(rng, 1, 1, 64)
    _both(hip_ctx, oracle_ctx, [t], mats, cases)
    assert rel_err(hip_ctx.excitation(), oracle_ctx.excitation()) < TOL


def test_ragged_batch_is_launched_per_lds_class(hip_ctx, oracle_ctx):
    """Designs whose strip counts put different numbers of pairs on a CU (5 ... 210 strips at nw = 200) in one batch:
    the fused kernel is launched once per LDS class through a pair list (raftx_hip.hip: lds_classes, launch_classes); every design,
    wherever its class puts it, gets the response the oracle computes for it."""
    rng = np.random.default_rng(77)
    S_list, nw, nC = [20, 150, 53, 53, 97, 5, 210, 53], 200, 2
    tables = [random_strips(rng, S, nw, 0.0) for S in S_list]
    mats = random_matrices(rng, len(S_list), nw, False)
    cases = synthetic_cases(rng, nC, 1, nw)
    _both(hip_ctx, oracle_ctx, tables, mats, cases)
    oh = hip_ctx.solve_dynamics(6, 0.01, 0.1)               # no optional outputs: the lean (sweep) specialisation
    oo = oracle_ctx.solve_dynamics(6, 0.01, 0.1)
    assert hip_ctx.last_solve_launch() == (0, 0, len(S_list) * nC)      # several grids, one workgroup per pair: not the persistent form
    assert np.array_equal(oh["niter"], oo["niter"]) and np.array_equal(oh["flags"], oo["flags"])
    for d in range(len(S_list)):
        assert group_rel_err(oh["Xi"][d], oo["Xi"][d]) < TOL
    again = hip_ctx.solve_dynamics(6, 0.01, 0.1)
    assert np.array_equal(oh["Xi"].view(np.uint8), again["Xi"].view(np.uint8))


# feature bits of the fused kernel (raftx_last_solve_kernel): the lean specialisations of the 200-bin shape
KF_FDEP, KF_EXTRA, KF_MCF, KF_MULTI, KF_ALL = 1, 8, 16, 32, 127


@pytest.mark.parametrize("fdep,mcf,nH,extra,expect", [
    (False, 0.0, 1, False, 0),
    (True, 0.0, 1, False, KF_FDEP),                                   # turbine aerodynamics: M(w), B(w)
    (False, 0.3, 1, False, KF_MCF),                                   # MacCamy-Fuchs columns
    (False, 0.0, 3, False, KF_MULTI),                                 # several wave headings
    (True, 0.0, 1, True, KF_FDEP | KF_EXTRA),                         # + a resident extra excitation (BEM, second-order)
    (False, 0.0, 1, True, KF_FDEP | KF_EXTRA),                        # extra excitation alone: the same kernel, empty M/B buffer
    (True, 0.3, 1, False, KF_FDEP | KF_MCF),
    (True, 0.0, 2, False, KF_FDEP | KF_MULTI),
    (False, 0.3, 2, False, KF_MCF | KF_MULTI),
    (True, 0.0, 2, True, KF_FDEP | KF_EXTRA | KF_MULTI),
    (True, 0.3, 2, False, KF_FDEP | KF_MCF | KF_MULTI),
    (True, 0.3, 2, True, KF_ALL),                                     # no lean kernel covers this: full-featured
])
def test_featured_sweep_kernels_run_lean_and_match_the_oracle(hip_ctx, oracle_ctx, fdep, mcf, nH, extra, expect):
    """Every lean specialisation of the C2/C3 shape (two waves per SIMD, results resident) against the oracle, and the
    dispatch itself: the smallest kernel that covers the sweep's features, the full-featured one only as the last resort
    (raft_model.py:1006-1007,1045-1048 frequency-dependent terms; :1200-1236 headings; raft_member.py:1415-1420 MCF)."""
    rng = np.random.default_rng(4242 + expect)
    nw, nC = 200, 2
    S_list = [53, 47, 0, 60]
    tables = [(_member_run_table(rng, max(1, S // 10), 10) if S else random_strips(rng, 0)) for S in S_list]
    if mcf:
        tables = add_mcf_rows(rng, tables, mcf, nw)                   # member-run geometry, MacCamy-Fuchs rows on some strips
    mats = random_matrices(rng, len(S_list), nw, fdep)
    cases = synthetic_cases(rng, nC, nH, nw)
    _both(hip_ctx, oracle_ctx, tables, mats, cases)
    Fe = None
    if extra:
        Fe = 2e4 * (rng.normal(size=(len(S_list), nC, nH, 6, nw)) + 1j * rng.normal(size=(len(S_list), nC, nH, 6, nw)))
    res = []
    for ctx in (hip_ctx, oracle_ctx):
        ctx.solve_dynamics_device(7, 0.01, 0.1, F_extra=Fe)
        res.append(ctx.fetch_results(want_Xi=True))
    flags, waves, _ = hip_ctx.last_solve_kernel()
    assert flags == expect, (flags, expect)
    assert waves == (1 if expect == KF_ALL else 2)
    assert np.array_equal(res[0]["niter"], res[1]["niter"])
    assert np.array_equal(res[0]["flags"], res[1]["flags"])
    for d in range(len(S_list)):
        assert group_rel_err(res[0]["Xi"][d], res[1]["Xi"][d]) < TOL


def test_submerged_rotor_on_the_device(hip_ctx, oracle_ctx):
    """Submerged rotors (raft_fowt.py:1861-1883) through the drop-in on the GPU: the rotor's pseudo-strips (force block +
    moment couples) ride along as further designs of the excitation launch and the fused solve takes their excitation
    as part of F_extra.  Device against the oracle on a stand-in unit whose rotor sits below the surface (the same
    scenario is pinned on the live reference in tests/test_dropin_live_reference.py); the rotor term must matter."""
    from raft_amd.snapshot import Obj
    from raft_amd.rigid import alternator
    out = {}
    for name, ctx in (("hip", hip_ctx), ("oracle", oracle_ctx)):
        fx, model = load_model_fixture("c2_volturnus.npz")
        f = model.fowtList[0]
        rng = np.random.default_rng(11)
        rot = Obj()
        rot.r3 = np.array([f.x_ref + 6.0, f.y_ref + 2.0, -14.0])
        th = 0.4
        rot.R_q = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
        I3, off = np.zeros((3, 3)), np.zeros((3, 3))
        for _ in range(3):
            A = rng.normal(size=(3, 3))
            Ii = 3e5 * (A @ A.T)
            I3 += Ii
            off += Ii @ alternator(rng.uniform(-15, 15, size=3))
        rot.I_hydro = np.zeros((6, 6))
        rot.I_hydro[:3, :3], rot.I_hydro[:3, 3:], rot.I_hydro[3:, :3] = I3, off, off.T
        node = Obj()
        node.id, node.nDOF, node.T = 0, 6, np.eye(6)
        rot.nodeList = [node]
        f.rotorList = [rot]
        if not hasattr(f, "r6"):
            f.r6 = np.r_[f.x_ref, f.y_ref, 0.0, 0.0, 0.0, 0.0]
        eng = dropin.Engine(ctx)
        case = case_from_fixture(fx["cases"][0])
        eng.calcHydroExcitation(f, dict(case), memberList=f.memberList)
        F1 = f.F_hydro_iner.copy()
        Xi = eng.solveDynamics(model, dict(case)).copy()
        out[name] = (F1, Xi, f.F_hydro_iner.copy(), rot.ud.copy())
        if name == "hip":
            f.rotorList = []
            eng.calcHydroExcitation(f, dict(case), memberList=f.memberList)
            assert rel_err(f.F_hydro_iner[-1], F1[-1]) > 1e-3
    for a, b in zip(out["hip"], out["oracle"]):
        assert rel_err(a, b) < TOL
