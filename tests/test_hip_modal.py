"""Eigen analysis on the device (include/raftx_modal.h): raftx_modal_batch against a numpy restatement of the reference
procedure and against the live reference's recorded results (tests/golden/modal_reference.npz), seeded synthetic sets
with every flag, the drop-in solveEigen on stand-ins, the resident path and the streamed sweep crossings."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from raft_amd import geometry as G
from raft_amd import snapshot as standin
from raft_amd._abi import (RaftxError, MODAL_SMALL_DIAG, MODAL_NONPOSITIVE, MODAL_COMPLEX, MODAL_SINGULAR_M)
from raft_amd.strips import UnsupportedFOWT
from raft_amd.sweep import VariantSweep, periods
from tests.test_modal import UNITS, reference_eigen, unit_matrices

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_modes(fn_dev, modes_dev, fn_ref, modes_ref, gap_tol=1e-6, tol=1e-9, sub_tol=1e-7):
    """Per mode 1 - |<v_dev, v_ref>| <= tol where the eigenvalue is separated (relative gap >= gap_tol); clusters by the
    largest principal angle between the spanned subspaces.  Sign: largest |component| positive."""
    lam = np.asarray(fn_ref) ** 2
    for j in range(6):
        big = int(np.argmax(np.abs(modes_dev[:, j])))
        assert modes_dev[big, j] > 0
        assert abs(np.linalg.norm(modes_dev[:, j]) - 1) < 1e-12
        others = np.delete(np.arange(6), j)
        gap = np.min(np.abs(lam[others] - lam[j])) / abs(lam[j])
        if gap >= gap_tol:
            assert 1 - abs(np.dot(modes_dev[:, j], modes_ref[:, j])) <= tol, (j, gap)
        else:
            cl = [k for k in range(6) if abs(lam[k] - lam[j]) / abs(lam[j]) < gap_tol]
            qa, _ = np.linalg.qr(modes_dev[:, cl])
            qb, _ = np.linalg.qr(np.asarray(modes_ref)[:, cl])
            s = np.linalg.svd(qa.T @ qb, compute_uv=False)
            assert np.arccos(np.clip(s.min(), -1, 1)) <= sub_tol, (j, cl)


def test_fixture_units(hip_ctx):
    Ms, Cs = zip(*[unit_matrices(u) for u in UNITS])
    r = hip_ctx.modal_batch(np.array(Ms), np.array(Cs))
    n_ok = 0
    for i, u in enumerate(UNITS):
        if u["error"]:
            assert r["flags"][i] & MODAL_SMALL_DIAG, u["name"]
            continue
        n_ok += 1
        assert r["flags"][i] == 0, u["name"]
        fn_np, modes_np = reference_eigen(Ms[i], Cs[i])
        assert np.max(np.abs(r["fn"][i] - fn_np) / fn_np) <= 1e-10, u["name"]
        assert np.max(np.abs(r["fn"][i] - u["model_fns"]) / u["model_fns"]) <= 1e-9, u["name"]
        check_modes(r["fn"][i], r["modes"][i], fn_np, modes_np)
        check_modes(r["fn"][i], r["modes"][i], u["model_fns"], u["model_modes"])
    assert n_ok >= 60


def _realistic(rng, n):
    M = np.zeros((n, 6, 6))
    d = np.array([1e7, 1e7, 1e7, 1e10, 1e10, 1e10]) * rng.uniform(0.5, 2.0, size=(n, 6))
    M[:, np.arange(6), np.arange(6)] = d
    cpl = rng.uniform(-0.3, 0.3, size=n) * np.sqrt(d[:, 0] * d[:, 4])
    M[:, 0, 4] = M[:, 4, 0] = cpl
    M[:, 1, 3] = M[:, 3, 1] = -cpl
    C = np.zeros((n, 6, 6))
    C[:, np.arange(6), np.arange(6)] = np.array([1e5, 1e5, 1e7, 1e9, 1e9, 1e8]) * rng.uniform(0.5, 2.0, size=(n, 6))
    off = rng.uniform(-0.2, 0.2, size=(n, 6, 6)) * np.sqrt(C[:, np.arange(6), np.arange(6)][:, :, None] *
                                                            C[:, np.arange(6), np.arange(6)][:, None, :])
    off = 0.5 * (off + np.swapaxes(off, 1, 2))
    off[:, np.arange(6), np.arange(6)] = 0
    C = C + off * 0.3
    C = C * (1 + 1e-3 * rng.uniform(-1, 1, size=(n, 6, 6)))                     # 1e-3 relative asymmetry
    return M, C


def test_synthetic_well_conditioned(hip_ctx):
    rng = np.random.default_rng(11)
    M, C = _realistic(rng, 10000)
    r = hip_ctx.modal_batch(M, C)
    bad = []
    for i in range(len(M)):
        lam = np.linalg.eigvals(np.linalg.solve(M[i], C[i]))
        if np.any(np.abs(lam.imag) > 0) or np.any(lam.real <= 0):
            assert r["flags"][i] & (MODAL_COMPLEX | MODAL_NONPOSITIVE)
            continue
        assert r["flags"][i] == 0
        fn_np, modes_np = reference_eigen(M[i], C[i])
        if np.max(np.abs(r["fn"][i] - fn_np) / fn_np) > 1e-9:
            bad.append(i)
        check_modes(r["fn"][i], r["modes"][i], fn_np, modes_np)
    assert not bad, bad[:5]
    assert np.all(np.isfinite(r["fn"][r["flags"] == 0]))


def test_synthetic_flags(hip_ctx):
    rng = np.random.default_rng(5)
    n = 10000
    M, C = _realistic(rng, n)
    kind = np.arange(n) % 6
    # 0: exactly degenerate pairs (two identical decoupled blocks); 1: skew-dominated C; 2: indefinite C; 3: small diagonal;
    # 4: singular M; 5: unchanged
    for i in np.where(kind == 0)[0]:
        M[i] = np.diag([2e7, 2e7, 3e7, 4e10, 4e10, 5e10])
        C[i] = np.diag([1e5, 1e5, 3e7, 2e9, 2e9, 1e8])
    C[kind == 1, 0, 4] += 1e9
    C[kind == 1, 4, 0] -= 1e9
    C[kind == 1, 1, 3] += 1e9
    C[kind == 1, 3, 1] -= 1e9
    C[kind == 2, 2, 2] = -abs(C[kind == 2, 2, 2])
    for i in np.where(kind == 3)[0]:                        # a heave stiffness below 1, still a well-posed problem
        M[i] = np.diag([2e7, 2e7, 3e7, 4e10, 4e10, 5e10]) + np.diag(rng.uniform(0, 1e6, size=6))
        C[i] = np.diag([1e5, 1e5, 0.5, 2e9, 2e9, 1e8])
        C[i, 0, 4] = C[i, 4, 0] = 1e6
    M[kind == 4, 5, :] = 0.0
    M[kind == 4, :, 5] = 0.0
    r = hip_ctx.modal_batch(M, C)
    fl, fn = r["flags"], r["fn"]
    assert np.all(np.isfinite(fn[fl == 0])) and np.all(np.isfinite(r["modes"][fl == 0]))
    assert np.all(np.isnan(fn[(fl & ~MODAL_SMALL_DIAG) != 0]))
    for i in np.where(kind == 0)[0][:200]:
        assert fl[i] == 0
        fn_np, modes_np = reference_eigen(M[i], C[i])
        assert np.max(np.abs(fn[i] - fn_np) / fn_np) <= 1e-9
        check_modes(fn[i], r["modes"][i], fn_np, modes_np)
    for i in np.where(kind == 1)[0]:
        if np.any(np.linalg.eigvals(np.linalg.solve(M[i], C[i])).imag != 0):
            assert fl[i] & MODAL_COMPLEX
    assert np.mean(fl[kind == 1] & MODAL_COMPLEX > 0) > 0.9
    assert np.all(fl[kind == 2] & (MODAL_NONPOSITIVE | MODAL_COMPLEX))
    assert np.all(fl[kind == 2] & MODAL_SMALL_DIAG)
    k3 = kind == 3
    assert np.all(fl[k3] & MODAL_SMALL_DIAG)
    assert np.all(fl[k3] == MODAL_SMALL_DIAG) and np.all(np.isfinite(fn[k3])) and np.all(np.isfinite(r["modes"][k3]))
    assert np.all(fl[kind == 4] & MODAL_SINGULAR_M)


# ------------------------------------------------------------------ drop-in on stand-ins of the fixture units
def _standin(u, nDOF=6):
    f = SimpleNamespace(nDOF=nDOF, M_struc=u["M_struc"], A_hydro_morison=u["A_hydro_morison"],
                        A_BEM=np.asarray(u["A_BEM0"])[:, :, None] * np.ones(3), C_struc=u["C_struc"], C_hydro=u["C_hydro"],
                        C_moor=u["C_moor"], C_elast=u["C_elast"], yawstiff=u["yawstiff"], body=None)
    return SimpleNamespace(fowtList=[f], ms=None, results={}), f


def test_dropin_solveEigen(hip_ctx):
    from raft_amd import dropin
    eng = dropin.Engine(hip_ctx)
    for u in UNITS[:6]:
        model, fowt = _standin(u)
        if u["error"]:
            with pytest.raises(RuntimeError, match="small or negative diagonals"):
                eng.solveEigen(model)
            continue
        fns, modes = eng.solveEigen(model)
        assert np.max(np.abs(fns - u["model_fns"]) / u["model_fns"]) <= 1e-9
        check_modes(fns, modes, u["model_fns"], u["model_modes"])
        assert model.results["eigen"]["frequencies"] is fns
        fns2, modes2 = eng.fowt_solveEigen(fowt)
        assert np.max(np.abs(fns2 - u["fowt_fns"]) / u["fowt_fns"]) <= 1e-9
        check_modes(fns2, modes2, u["fowt_fns"], u["fowt_modes"])
    bad = [u for u in UNITS if u["error"]][0]
    with pytest.raises(RuntimeError, match="small or negative diagonals"):
        eng.fowt_solveEigen(_standin(bad)[1])
    u = UNITS[1]
    model, fowt = _standin(u)                               # positive diagonals, indefinite: a negative eigenvalue
    Cd = np.diag(unit_matrices(u)[1])
    fowt.C_moor = np.array(u["C_moor"]) + 0.0
    k = 3.0 * np.sqrt(Cd[2] * Cd[3])
    fowt.C_moor[2, 3] += k
    fowt.C_moor[3, 2] += k
    with pytest.raises(RuntimeError, match="zero or negative system eigenvalues"):
        eng.solveEigen(model)
    model, fowt = _standin(UNITS[1])
    fowt.C_moor = np.array(UNITS[1]["C_moor"]) + 0.0
    fowt.C_moor[0, 4] += 1e10
    fowt.C_moor[4, 0] -= 1e10
    fowt.C_moor[1, 3] += 1e10
    fowt.C_moor[3, 1] -= 1e10
    with pytest.raises(UnsupportedFOWT):
        eng.solveEigen(model)
    model, _ = _standin(UNITS[1])
    model.fowtList = model.fowtList * 2
    with pytest.raises(UnsupportedFOWT):
        eng.solveEigen(model)
    model, fowt = _standin(UNITS[1], nDOF=12)
    with pytest.raises(UnsupportedFOWT):
        eng.solveEigen(model)


# ------------------------------------------------------------------ resident path and sweep crossings
def _variant_sweep(n, seed=None):
    fg = standin.load_fixture("geom_units.npz")
    c3 = standin.load_fixture("c3_variants.npz")
    base = json.loads(fg["c3_base_json"])
    u0 = [u for u in fg["units"] if u["name"] == "C3-variant-0"][0]
    M_rna = np.asarray(u0["M_struc"]) - np.asarray(u0["M_struc_bare"])
    C_rest = np.asarray(u0["C_struc"]) - np.asarray(u0["C_struc_bare"]) + np.diag([7e4, 7e4, 0, 0, 0, 1e8])
    scales = np.asarray(c3["scales"])[:n] if seed is None else np.random.default_rng(seed).uniform(0.75, 1.25, size=(n, 5))
    rep = lambda a: np.repeat(a[None], n, axis=0)
    return VariantSweep(G.volturnus_program(base), G.volturnus_params(scales), rep(M_rna), np.zeros((n, 6, 6)), rep(C_rest),
                        c3["w"], c3["k"], float(c3["depth"]), np.asarray(c3["zeta"])[None], np.asarray(c3["beta"])[None],
                        int(c3["nIter"]), float(c3["XiStart"]))


def _dMdC(n, seed=3):
    rng = np.random.default_rng(seed)
    dM = np.zeros((n, 6, 6))
    dM[:, np.arange(6), np.arange(6)] = rng.uniform(0, 1e5, size=(n, 6))
    dC = np.zeros((n, 6, 6))
    dC[:, 5, 5] = rng.uniform(0, 1e7, size=n)
    return dM, dC


def _same(a, b, keys=("fn", "modes", "flags", "props")):
    for k in keys:
        x, y = a[k], b[k]
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), k


def test_resident_path(hip_ctx):
    n = 64
    sw = _variant_sweep(n)
    sw.upload(hip_ctx)
    res = sw.run_modal(hip_ctx, want_props=True)
    S = hip_ctx.fetch_statics()
    M = (sw.M0 + S["A_morison"]) + S["M_struc"]                # k_geom_addup's order
    C = (sw.C0 + S["C_hydro"]) + S["C_struc"]
    bat = hip_ctx.modal_batch(M, C)
    _same(res, bat, ("fn", "modes", "flags"))
    assert np.array_equal(res["props"], S["props"])
    n_ok = 0
    for i, u in enumerate([u for u in UNITS if u["name"].startswith("C3-variant-")]):
        if u["error"]:
            assert res["flags"][i] & MODAL_SMALL_DIAG
            continue
        n_ok += 1
        assert res["flags"][i] == 0
        assert np.max(np.abs(res["fn"][i] - u["model_fns"]) / u["model_fns"]) <= 1e-9, i
    assert n_ok >= 55
    dM, dC = _dMdC(n)
    r2 = sw.run_modal(hip_ctx, dM, dC)
    _same(r2, hip_ctx.modal_batch(M + dM, C + dC), ("fn", "modes", "flags"))
    assert np.all(periods(res["fn"][res["flags"] == 0]) > 1.0)


def _crossing_vs_resident(ctx, sw, n_chunk, dM=None, dC=None):
    base = sw.run_crossing(ctx, n_chunk=n_chunk, slot=1)
    out = sw.run_crossing(ctx, n_chunk=n_chunk, slot=0, modal=True, dM=dM, dC=dC, want_props=True)
    for k in ("std", "niter", "flags"):
        assert np.array_equal(np.asarray(base[k]).view(np.uint8), np.asarray(out[k]).view(np.uint8)), k
    sw.upload(ctx)
    res = sw.run_modal(ctx, dM, dC, want_props=True)
    _same({"fn": out["fn"], "modes": out["modes"], "flags": out["modal_flags"], "props": out["props"]}, res)
    return out


def test_crossing_64_variants(hip_ctx):
    sw = _variant_sweep(64)
    out = _crossing_vs_resident(hip_ctx, sw, 0)
    dM, dC = _dMdC(64)
    _crossing_vs_resident(hip_ctx, sw, 0, dM, dC)
    ok = out["modal_flags"] == 0
    assert ok.sum() >= 55


def test_crossing_10k_chunked(hip_ctx):
    sw = _variant_sweep(10000, seed=0)
    dM, dC = _dMdC(10000)
    out = _crossing_vs_resident(hip_ctx, sw, 4, dM, dC)
    assert np.all(np.isnan(out["fn"][(out["modal_flags"] & ~MODAL_SMALL_DIAG) != 0]))
    assert np.all(np.isfinite(out["fn"][out["modal_flags"] == 0]))


def test_stream_alternating_modal(hip_ctx):
    """Four batches on rotating slots, all in flight together, modal on alternate batches: each returns its own results."""
    n = 2000
    sw = _variant_sweep(n, seed=21)
    params = [_variant_sweep(n, seed=s).params for s in (21, 22, 23, 24)]
    hs = []
    for b, p in enumerate(params):
        sw.set_params(p)
        hs.append(sw.submit_crossing(hip_ctx, b % 4, modal=(b % 2 == 0), want_props=(b % 2 == 0)))
    outs = [sw.wait_crossing(hip_ctx, h) for h in hs]
    for b, (p, out) in enumerate(zip(params, outs)):
        sw.set_params(p)
        alone = sw.run_crossing(hip_ctx, slot=0)
        for k in ("std", "niter", "flags"):
            assert np.array_equal(np.asarray(alone[k]), np.asarray(out[k])), (b, k)
        if b % 2 == 0:
            sw.upload(hip_ctx)
            _same({"fn": out["fn"], "modes": out["modes"], "flags": out["modal_flags"], "props": out["props"]},
                  sw.run_modal(hip_ctx, want_props=True))
        else:
            assert "fn" not in out


def test_sweep_modal_on_idle_or_launched_slot(hip_ctx):
    sw = _variant_sweep(64)
    h = sw.prepare_crossing(hip_ctx, 2)
    fake = {"slot": 3, "out": h["out"]}
    with pytest.raises(RaftxError, match="nothing prepared"):
        hip_ctx.sweep_modal(fake)
    sw.launch_crossing(hip_ctx, h)
    with pytest.raises(RaftxError, match="has been launched"):
        hip_ctx.sweep_modal(h)
    out = sw.wait_crossing(hip_ctx, h)
    alone = sw.run_crossing(hip_ctx, slot=0)
    assert np.array_equal(out["std"], alone["std"])


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from raft_amd import backend
from tests.test_hip_modal import _variant_sweep, _dMdC
ctx = backend.default_context(0)
sw = _variant_sweep(3000, seed=7)
dM, dC = _dMdC(3000)
h1 = sw.submit_crossing(ctx, 0, n_chunk=2, modal=True, dM=dM, dC=dC, want_props=True)
sw.set_params(_variant_sweep(3000, seed=8).params)        # a second batch in flight behind the first
h2 = sw.submit_crossing(ctx, 1, modal=True, dM=dM, dC=dC, want_props=True)
o1 = sw.wait_crossing(ctx, h1); o2 = sw.wait_crossing(ctx, h2)
np.savez(sys.argv[1], **{"%%s%%d" %% (k, i): o[k] for i, o in enumerate((o1, o2)) for k in ("fn", "modes", "modal_flags", "props", "std")})
"""


def test_generation_forms_bit_identical(tmp_path):
    runs = {}
    for name, env in (("default", {}), ("fused", {"RAFTX_FUSED_GEN": "1"}), ("addup", {"RAFTX_ADDUP_KERNEL": "1"})):
        out = str(tmp_path / (name + ".npz"))
        e = dict(os.environ)
        e.pop("RAFTX_FUSED_GEN", None)
        e.pop("RAFTX_ADDUP_KERNEL", None)
        e.update(env)
        subprocess.run([sys.executable, "-c", _CHILD % ROOT, out], env=e, check=True, timeout=600, cwd=ROOT)
        runs[name] = np.load(out)
    for name in ("fused", "addup"):
        for k in runs["default"].files:
            assert np.array_equal(runs["default"][k].view(np.uint8), runs[name][k].view(np.uint8)), (name, k)
