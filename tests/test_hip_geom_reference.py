"""The geometry gate on the device: every case, launch shape and route of tests/geom_cases.py through
raftx_build_designs of the device library, entry by entry under |x - D| <= C eps E against tests/geom_reference.py in
longdouble, with the constant fixed on the CPU (tests/test_geom_reference.py).  Offsets, index columns, the circ flag and the
MacCamy-Fuchs row indices are exact; E == 0 entries must be exactly 0.  A failure names the design and the output entry.

The matrices the ADD_* bits add into stay resident (the ABI exports no copy of them): that route is held to the generated
tables and statics, which must be the ones of add_mask 0, bit for bit.
"""
import numpy as np
import pytest

from raft_amd import geometry as G
from raft_amd._abi import RaftxError
from tests import geom_cases as gc
from tests import geom_reference as gr
from tests.test_geom_reference import add_route_inputs, trim_inputs, trim_references

pytestmark = pytest.mark.gpu

C = gr.GATE_C
UNITS = [u.name for u in gc.ONE + gc.SHAPES + gc.MULTI]
ALONE = {}                                   # name -> what the device generated for the design alone


def gated(out, d, ref, what):
    res = gc.check_design(out, d, ref, what)
    gc.assert_gate(res, C, what)
    return res


def design_bits(out, d):
    lo, hi = int(out.off[d]), int(out.off[d + 1])
    return [out.strips[lo:hi]] + [out.statics[k][d] for k in gr.STATICS]


def same_bits(a, b, what):
    for x, y, k in zip(a, b, ("strips",) + gr.STATICS):
        assert x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64)), (what, k)


def alone(ctx, name):
    if name not in ALONE:
        ALONE[name] = gc.build(ctx, [gc.ALL[name]])
    return ALONE[name]


@pytest.mark.parametrize("name", UNITS)
def test_device_design_alone(name, hip_ctx):
    out = alone(hip_ctx, name)
    ref = gc.reference(gc.ALL[name])
    assert np.array_equal(out.off, [0, len(ref.idx)])
    res = gated(out, 0, ref, name)
    print("%-40s %s" % (name, "  ".join("%s %.2f" % kv for kv in gc.worst(res).items())))


def check_batch(ctx, units, what, refs=None, **kw):
    out = gc.build(ctx, units, **kw)
    refs = [gc.reference(u) for u in units] if refs is None else refs
    assert np.array_equal(out.off, np.concatenate([[0], np.cumsum([len(r.idx) for r in refs])])), (what, "strip offsets")
    for d, (u, ref) in enumerate(zip(units, refs)):
        gated(out, d, ref, "%s, design %d (%s)" % (what, d, u.name))
    return out


@pytest.mark.parametrize("name", list(gc.batches()))
def test_device_batches(name, hip_ctx):
    check_batch(hip_ctx, gc.batches()[name], name)


@pytest.mark.parametrize("n", gc.SCAN_SIZES)
def test_device_scan_batches(n, hip_ctx):
    """One-member designs on either side of the scan chunk: the offsets are the exact cumulative sums, every design gated."""
    units = [gc.SCAN[i % len(gc.SCAN)] for i in range(n)]
    out = check_batch(hip_ctx, units, "%d designs" % n)
    for d in range(len(gc.SCAN), n):                      # every repeat of a design is the first one, bit for bit
        same_bits(design_bits(out, d), design_bits(out, d % len(gc.SCAN)), "%d designs, design %d" % (n, d))


def test_device_batch_of_all_cases_is_each_case_alone_bit_for_bit(hip_ctx):
    """Different members in the same wavefront change nothing: a property of its own."""
    units = gc.ONE + gc.MULTI
    out = gc.build(hip_ctx, units)
    for d, u in enumerate(units):
        one = alone(hip_ctx, u.name)
        same_bits(design_bits(out, d), design_bits(one, 0), u.name)


def test_device_add_route(hip_ctx):
    units = gc.batches()["a dry design in the middle"] + gc.MULTI
    M0, C0 = add_route_inputs(len(units))
    out = check_batch(hip_ctx, units, "ADD_*", add_mask=G.ADD_MORISON | G.ADD_HYDROSTATIC | G.ADD_INERTIA, M0=M0, C0=C0)
    plain = gc.build(hip_ctx, units)
    for d, u in enumerate(units):
        same_bits(design_bits(out, d), design_bits(plain, d), "ADD_* against add_mask 0, " + u.name)


def test_device_trim_route(hip_ctx):
    refs = trim_references()
    out = check_batch(hip_ctx, gc.TRIM, "TRIM_BALLAST", refs=refs, add_mask=G.TRIM_BALLAST, M0=trim_inputs(), Fz_moor=gc.TRIM_FZ)
    assert np.all(out.statics["props"][:, G.SP_DRHO] != 0)


def test_device_variant_route(hip_ctx):
    """Three C3 variants through VariantSweep.upload: fixed members from k_geom_member_fixed, descriptors from the library."""
    out, refs = gc.variant_route(hip_ctx)
    assert np.array_equal(out.off, np.concatenate([[0], np.cumsum([len(r.idx) for r in refs])]))
    for d, ref in enumerate(refs):
        gated(out, d, ref, "C3 variant %d" % d)


@pytest.mark.parametrize("u", gc.REFUSED, ids=[u.name for u in gc.REFUSED])
def test_device_refuses_what_the_oracle_refuses(u, hip_ctx, oracle_ctx):
    with pytest.raises(RaftxError) as eo:
        gc.build(oracle_ctx, [u])
    with pytest.raises(RaftxError) as eh:
        gc.build(hip_ctx, [u])
    for e in (eo, eh):                                    # the same refusal of the same member from both libraries
        assert "member 0: cap/bulkhead layout not supported" in str(e.value), str(e.value)
