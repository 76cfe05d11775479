"""The device half of tests/test_linear_solve.py: every coupled and dense input of tests/linear_solve_cases.py through the HIP
library, held to the same GATE on the normwise backward error against the long-double contract
(tests/linear_solve_reference.py) -- k_solve_system_rows in all its instantiations, k_solve_system at 4, 2 and 1 bins per
workgroup and beyond 64 KiB of LDS, k_solve_dense_reg2 on both sides of every selection edge, k_solve_dense -- on inputs
whose elimination has exactly one acceptable pivot per step (forced), nothing but exact ties (ties), or every pivot off the
diagonal (permuted).  A parametrised case names the family and the instantiation.

Dynamic LDS of the LDS-resident solver as solve_system_shape gives it (bins per workgroup x 16 n (n + nRhs) bytes):
(1,1) 4 x 672 B, (4,5) 4 x 11 136 B, (5,5) 2 x 16 800 B, (6,1) 2 x 21 312 B, (7,7) 1 x 32 928 B, (10,3) 60 480 B = 59.1 KiB,
(11,1) 70 752 B = 69.1 KiB -- the first shape that needs hipFuncSetAttribute -- and (16,4) 153 600 B = exactly 150 KiB;
(17,1) would need 168 096 B and (16,5) 155 136 B: refused by the entry before any launch."""
import numpy as np
import pytest

from tests import linear_solve_cases as K
from tests import test_linear_solve as T

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("family,nUnit,nRhs", T.COUPLED_PARAMS)
def test_hip_coupled_solve_within_gate(hip_ctx, family, nUnit, nRhs):
    T.check_coupled(hip_ctx, family, nUnit, nRhs)


@pytest.mark.parametrize("family,n,nRhs", T.DENSE_PARAMS)
def test_hip_dense_solve_within_gate(hip_ctx, family, n, nRhs):
    T.check_dense(hip_ctx, family, n, nRhs)


def test_hip_dense_resident_with_badd_within_gate(hip_ctx):
    T.check_dense_resident(hip_ctx)


@pytest.mark.parametrize("nUnit,nHead,mode", T.RESIDENT_PARAMS)
def test_hip_resident_coupled_solve_within_gate(hip_ctx, nUnit, nHead, mode):
    T.check_resident(hip_ctx, nUnit, nHead, mode)


def test_hip_shapes_beyond_the_lds_are_refused(hip_ctx):
    T.check_refused(hip_ctx)


@pytest.mark.parametrize("kind", ["nan", "singular"])
@pytest.mark.parametrize("nUnit,nRhs,nw,iw", T.CONTAINMENT)
def test_hip_poisoned_bin_stays_in_its_half_wave(hip_ctx, nUnit, nRhs, nw, iw, kind):
    """(3,2): the rows kernel, two bins per wavefront -- bin 2 shares its wave with bin 3, bin 4 with its own clone; (6,1)
    and (1,1): the LDS solver at 2 and 4 bins per workgroup."""
    T.check_containment(hip_ctx, nUnit, nRhs, nw, iw, kind)


REPEAT = {"rows": lambda ctx: _coupled(ctx, 5, 4, 5), "lds": lambda ctx: _coupled(ctx, 6, 1, 3),
          "dense_reg2": lambda ctx: _dense(ctx, 62, 2), "dense_l2": lambda ctx: _dense(ctx, *K.DENSE_L2_SHAPE)}


def _coupled(ctx, nUnit, nRhs, nw):
    c, _, _ = T.coupled_input("forced", nUnit, nRhs, nw)
    return ctx.solve_system(c["w"], c["Zblk"], c["F"], c["Mc"], c["Bc"], c["Cc"])


def _dense(ctx, n, nRhs):
    c, _, _ = T._dense_case("forced", n, nRhs)
    return ctx.solve_dense_batch(c["w"], c["M"], c["B"], c["C"], c["F"])


@pytest.mark.parametrize("kernel", sorted(REPEAT))
def test_hip_repeat_runs_are_bit_identical(hip_ctx, kernel):
    T.check_repeat(lambda: REPEAT[kernel](hip_ctx))
    assert np.all(np.isfinite(REPEAT[kernel](hip_ctx).view(float)))
