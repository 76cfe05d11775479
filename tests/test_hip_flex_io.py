"""raftx_flex_solve / raftx_flex_start: the optional outputs, preallocated outputs, the explicit start and its one-shot rule,
a frequency-dependent B and the refusals -- what tests/test_flexible.py, which always asks for every output and never
sets a start, leaves uncovered.

Every check is one helper, run on the CPU oracle (unmarked) and on the device library with the oracle as the second backend
(``gpu``), as tests/test_flexible.py does.  One problem throughout, that file's smallest: ragged units of 3, 1 and 5 wet
nodes, 20 reduced DOFs (no multiple of the projection's 16-wide tile), two headings, three sea states, frequency-dependent M.
Tolerances are that file's: 1e-9 device against oracle; bit equality within one backend where a check says "same"."""
import functools

import numpy as np
import pytest

from tests.test_flexible import _flex_problem
from tests.util import rel_err

KEYS = ("Xi", "niter", "flags", "B_drag", "F_drag", "Z")
WANT = {"B_drag": "want_B", "F_drag": "want_F", "Z": "want_Z"}


@functools.lru_cache(maxsize=None)
def _problem():
    return _flex_problem(np.random.default_rng(11), 3, [3, 1, 5], 20, 3, 2, True)


def _load(ctx):
    """the problem's node tables and sea states, resident in ctx"""
    P = _problem()
    nw = len(P["w"])
    Z6 = np.zeros((len(P["tabs"]), 6, 6))
    ctx.upload_designs(P["tabs"], Z6, Z6, Z6, nw)
    ctx.upload_cases(P["w"], P["k"], P["depth"], 1025.0, 9.81, P["zeta"], P["beta"])
    return P


def _solve(ctx, P, nIter=12, B=None, want_B=True, want_F=True, want_Z=True, out=None):
    return ctx.flex_solve(P["node_off"], P["Tn"], P["M"], P["B"] if B is None else B, P["C"], P["F_lin"], nIter, 0.01, 0.1,
                          want_B=want_B, want_F=want_F, want_Z=want_Z, out=out)


_FULL = {}


def _full(ctx, P):
    """the plain call with every output: computed once per backend, shared by the checks and left unchanged"""
    if ctx.rlib.is_device not in _FULL:
        _FULL[ctx.rlib.is_device] = _solve(ctx, P)
    return _FULL[ctx.rlib.is_device]


def _same(a, b, keys=KEYS):
    """bit equality of the named results"""
    for key in keys:
        assert a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), key


def _agree(a, b, tol=1e-9):
    """two backends: the iteration counts and flags equal, the arrays within tol"""
    assert np.array_equal(a["niter"], b["niter"]) and np.array_equal(a["flags"], b["flags"])
    for key in ("Xi", "B_drag", "F_drag", "Z"):
        assert rel_err(a[key], b[key]) < tol, key


def _start(P, rng=None):
    """an iterate [nUnit,nCase,n,nw]: the constant XiStart of _solve, or random of that size"""
    shape = P["F_lin"].shape[:2] + P["F_lin"].shape[3:]
    if rng is None:
        return np.full(shape, 0.1, dtype=np.complex128)
    return 0.1 * (rng.normal(size=shape) + 1j * rng.normal(size=shape))


def _check_optional_outputs(ctx):
    """Each of B_drag, F_drag, Z left out, and all three: the omitted entries are None, everything else has the bits of the
    call that asks for all of them."""
    P = _load(ctx)
    full = _full(ctx, P)
    assert len(set(full["niter"].ravel().tolist())) > 1 and int(full["niter"].max()) > 2      # (pairs of different length)
    for off in (("B_drag",), ("F_drag",), ("Z",), ("B_drag", "F_drag", "Z")):
        r = _solve(ctx, P, **{WANT[key]: False for key in off})
        assert all(r[key] is None for key in off), off
        _same(r, full, [key for key in KEYS if key not in off])


def _check_preallocated_outputs(ctx):
    """out= arrays for Xi, B_drag, F_drag, Z: returned as those objects, with the bits of the call that allocates its own."""
    P = _load(ctx)
    full = _full(ctx, P)
    out = {key: np.full(full[key].shape, 7.25, dtype=full[key].dtype) for key in ("Xi", "B_drag", "F_drag", "Z")}
    r = _solve(ctx, P, out=out)
    assert all(r[key] is out[key] for key in out)
    _same(r, full)
    part = {"Xi": out["Xi"], "F_drag": out["F_drag"]}                        # two of them, Z not wanted
    r = _solve(ctx, P, want_Z=False, out=part)
    assert r["Xi"] is part["Xi"] and r["F_drag"] is part["F_drag"] and r["Z"] is None
    _same(r, full, KEYS[:5])


def _check_explicit_start(ctx, other=None):
    """raftx_flex_start with the constant XiStart is the plain call (no iteration allowed: one pass, niter 1); from a random
    iterate the two backends agree."""
    P = _load(ctx)
    plain0 = _solve(ctx, P, nIter=0)
    ctx.flex_start(_start(P))
    r = _solve(ctx, P, nIter=0)
    assert (r["niter"] == 1).all()
    _same(r, plain0)
    X0 = _start(P, np.random.default_rng(12))
    ctx.flex_start(X0)
    a = _solve(ctx, P)
    assert np.isfinite(a["Xi"]).all()
    if other is not None:
        Po = _load(other)
        other.flex_start(X0)
        _agree(a, _solve(other, Po))


def _check_one_shot(ctx):
    """A start is used by one call: the call after it is the plain one; flex_start(None) clears a pending start; a start of
    another size fails the call that meets it ("linearisation point") and is gone after it."""
    P = _load(ctx)
    plain = _solve(ctx, P, nIter=1)
    X0 = _start(P, np.random.default_rng(12))
    ctx.flex_start(X0)
    assert _solve(ctx, P, nIter=1)["Xi"].tobytes() != plain["Xi"].tobytes()  # (the start was used ...)
    _same(_solve(ctx, P, nIter=1), plain)                                    # (... once)
    ctx.flex_start(X0)
    ctx.flex_start(None)
    _same(_solve(ctx, P, nIter=1), plain)
    ctx.flex_start(X0[:2])
    with pytest.raises(Exception, match="linearisation point"):
        _solve(ctx, P, nIter=1)
    _same(_solve(ctx, P, nIter=1), plain)


def _check_frequency_dependent_B(ctx, other=None):
    """B [nUnit,n,n,nw] with the constant B in every bin (mask 3: M is frequency-dependent too) against the constant B"""
    P = _load(ctx)
    nw = len(P["w"])
    Bw = np.ascontiguousarray(np.repeat(P["B"][..., None], nw, axis=-1))
    a = _solve(ctx, P, B=Bw)
    _agree(a, _full(ctx, P), 1e-12)
    if other is not None:
        _agree(a, _solve(other, _load(other), B=Bw))


def _check_refusals(ctx):
    """Offsets that do not end at the resident node count, offsets that go backwards, fewer than 6 reduced DOFs.  The oracle
    has no check of the offsets' order and calls n < 6 "bad arguments": the second refusal and the wording of the third
    are asserted for the device library only."""
    P = _load(ctx)
    dev = ctx.rlib.is_device
    with pytest.raises(Exception, match="nodeOff"):
        ctx.flex_solve([0, 3, 4, 8], P["Tn"][:8], P["M"], P["B"], P["C"], P["F_lin"], 3, 0.01, 0.1)
    if dev:
        with pytest.raises(Exception, match="monotone"):
            ctx.flex_solve([0, 5, 3, 9], P["Tn"], P["M"], P["B"], P["C"], P["F_lin"], 3, 0.01, 0.1)
    with pytest.raises(Exception, match="n = 5 reduced DOFs" if dev else "bad arguments"):
        ctx.flex_solve(P["node_off"], P["Tn"][:, :, :5], P["M"][:, :5, :5], P["B"][:, :5, :5], P["C"][:, :5, :5], P["F_lin"][:, :, :, :5],
                       3, 0.01, 0.1)
    _solve(ctx, P, nIter=0)                                                  # (the context is still good)


def test_oracle_flex_optional_outputs(oracle_ctx):
    _check_optional_outputs(oracle_ctx)


def test_oracle_flex_preallocated_outputs(oracle_ctx):
    _check_preallocated_outputs(oracle_ctx)


def test_oracle_flex_explicit_start(oracle_ctx):
    _check_explicit_start(oracle_ctx)


def test_oracle_flex_start_is_one_shot(oracle_ctx):
    _check_one_shot(oracle_ctx)


def test_oracle_flex_frequency_dependent_B(oracle_ctx):
    _check_frequency_dependent_B(oracle_ctx)


def test_oracle_flex_refusals(oracle_ctx):
    _check_refusals(oracle_ctx)


@pytest.mark.gpu
def test_hip_flex_optional_outputs(hip_ctx):
    _check_optional_outputs(hip_ctx)


@pytest.mark.gpu
def test_hip_flex_preallocated_outputs(hip_ctx):
    _check_preallocated_outputs(hip_ctx)


@pytest.mark.gpu
def test_hip_flex_explicit_start(hip_ctx, oracle_ctx):
    _check_explicit_start(hip_ctx, oracle_ctx)


@pytest.mark.gpu
def test_hip_flex_start_is_one_shot(hip_ctx):
    _check_one_shot(hip_ctx)


@pytest.mark.gpu
def test_hip_flex_frequency_dependent_B(hip_ctx, oracle_ctx):
    _check_frequency_dependent_B(hip_ctx, oracle_ctx)


@pytest.mark.gpu
def test_hip_flex_refusals(hip_ctx):
    _check_refusals(hip_ctx)
