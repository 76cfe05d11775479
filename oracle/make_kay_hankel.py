"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/kay_hankel_ref.npz: J_n(x) and Y_n(x), n = 0 .. 12, with mpmath at
50 digits, for exactly the arguments x = k R the Kim & Yue tests of tests/test_qtf_reference.py use
(tests/qtf_reference.kay_fixture_arguments).  Every value is stored as a (hi, lo) pair of float64 (hi + lo carries
~106 bits, more than the longdouble reference reads); the arguments are stored too, and the tests look theirs up bit
for bit, so the file cannot drift from them.

    python oracle/make_kay_hankel.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import qtf_reference as R          # noqa: E402


def hi_lo(v):
    """mpmath number -> (hi, lo) float64 with hi + lo = v to ~106 bits"""
    hi = float(v)
    return hi, float(v - hi)


def values(xs, digits=50):
    """J_hi, J_lo, Y_hi, Y_lo [len(xs), 13] of the float64 arguments xs (taken exactly)"""
    import mpmath
    mpmath.mp.dps = digits
    out = np.zeros((4, len(xs), R.N_ORDER))
    for i, x in enumerate(xs):
        xm = mpmath.mpf(float(x))
        for n in range(R.N_ORDER):
            out[0, i, n], out[1, i, n] = hi_lo(mpmath.besselj(n, xm))
            out[2, i, n], out[3, i, n] = hi_lo(mpmath.bessely(n, xm))
    return out


if __name__ == "__main__":
    xs = R.kay_fixture_arguments()
    v = values(xs)
    np.savez_compressed(R.GOLDEN, x=xs, J_hi=v[0], J_lo=v[1], Y_hi=v[2], Y_lo=v[3])
    print("%s: %d arguments, %d bytes" % (R.GOLDEN, len(xs), os.path.getsize(R.GOLDEN)))
