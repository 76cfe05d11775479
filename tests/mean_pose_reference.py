"""Independent mean-pose solve of include/raftx_statics.h in ``numpy.longdouble``: the reference of
tests/test_mean_pose.py and tests/test_hip_mean_pose.py.

The root x* of

    Y(x) = F0 + F_env - K_hs (x - x_ref) + F_moor(x) = 0                      Jacobian  -dY/dx = K_hs + C_moor(x)

is found by the plain Newton iteration from x_ref, with F_moor, C_moor and the envelope EF of tests/mooring_reference.py
(``evaluate``, longdouble).  That evaluation takes fp64 poses, so the iterates live on the fp64 grid; the iteration runs
until the step no longer shrinks, and the returned root is the last fp64 iterate plus the Newton step from it, both in
longdouble: quadratic convergence makes that root exact to about eps^2 relative to the step's scale.  None of the
kernel's safeguards (diagonal repair, step caps) is used: a case that needs them is not a case for this reference.

Accuracy gate (component by component):  |x - x*|_i <= GATE eps (|K^-1| E_F)_i  with
    E_F = |F0| + |F_env| + |K_hs| |x* - x_ref| + EF
-- the magnitudes of the addends of Y, EF with the catenary's condition number folded in -- pushed through the
magnitudes of the inverse Jacobian.  The residual the solver returns at its pose is held to ||Y|| <= GATE eps ||E_F||.
"""
import numpy as np

from . import mooring_reference as mr

EPS = mr.EPS
REF_TOL = (0.05, 0.005)           # the reference's stopping tolerances (raft_model.py:664)
STEP_CAPS = np.array([30.0, 30.0, 5.0, 0.1, 0.1, 0.1])       # raft_model.py:667
FLAG_POSE_CAP, FLAG_SINGULAR = 16, 32

# Worst multiple of eps |K^-1| E_F of the fp64 model of the device algorithm (tests/mean_pose_device_model.py) over the
# cases of tests/mean_pose_cases.py, measured on the CPU: 0.26 (the surge of VolturnUS-S-pointInertia under the thrust-like
# load; every single-line case <= 0.04).  GATE is the power of two at or above 4 x that, as GATE_C of
# tests/mooring_reference.py: the library log / sqrt of host and device differ, and the kernel contracts multiply-adds.
GATE_WORST_CPU = 0.27
GATE = 2


def _eval(lines_d, x64, depth, K_hs, F0, F_env, x_ref):
    T = np.longdouble
    m = mr.evaluate(np.asarray(lines_d)[None], np.asarray(x64, dtype=np.float64)[None], depth)
    if m["flags"][0]:
        raise ValueError("the mooring reference flags the pose %s: %d" % (x64, m["flags"][0]))
    dx = np.asarray(x64, dtype=np.float64).astype(T) - x_ref
    Y = F0 + F_env - K_hs @ dx + m["F"][0]
    return Y, K_hs + m["C"][0], m


def newton_step(lines_d, depth, K_hs, F0, F_env=None, x_ref=None, at=None):
    """The Newton step K^-1 Y (longdouble) at the fp64 pose ``at``."""
    T = np.longdouble
    K_hs, F0 = np.asarray(K_hs, dtype=np.float64).astype(T), np.asarray(F0, dtype=np.float64).astype(T)
    F_env = np.zeros(6, dtype=T) if F_env is None else np.asarray(F_env, dtype=np.float64).astype(T)
    x_ref = np.zeros(6, dtype=T) if x_ref is None else np.asarray(x_ref, dtype=np.float64).astype(T)
    Y, K, _ = _eval(lines_d, at, depth, K_hs, F0, F_env, x_ref)
    return _solve(K, Y)


def _solve(K, Y):
    """K^-1 Y in longdouble: an fp64 solve refined three times."""
    T = np.longdouble
    K64 = K.astype(np.float64)
    x = np.linalg.solve(K64, Y.astype(np.float64)).astype(T)
    for _ in range(3):
        x = x + np.linalg.solve(K64, (Y - K @ x).astype(np.float64)).astype(T)
    return x


def solve(lines_d, depth, K_hs, F0, F_env=None, x_ref=None, max_it=40):
    """dict of the root x [6] (longdouble), iterations (Newton steps until the step stopped shrinking), K (the Jacobian
    at the root), Kinv_abs = |K^-1|, E_F [6], bound = (|K^-1| E_F) [6] and the mooring reference's result ``moor`` at
    the fp64 rounding of the root."""
    T = np.longdouble
    K_hs, F0 = np.asarray(K_hs, dtype=np.float64).astype(T), np.asarray(F0, dtype=np.float64).astype(T)
    F_env = np.zeros(6, dtype=T) if F_env is None else np.asarray(F_env, dtype=np.float64).astype(T)
    x_ref = np.zeros(6, dtype=T) if x_ref is None else np.asarray(x_ref, dtype=np.float64).astype(T)
    x = x_ref.astype(np.float64)
    last, it = np.inf, 0
    while True:
        Y, K, m = _eval(lines_d, x, depth, K_hs, F0, F_env, x_ref)
        dX = _solve(K, Y)
        size = float(np.max(np.abs(dX)))
        if size >= last or size == 0.0 or it >= max_it:
            break
        x = (x.astype(T) + dX).astype(np.float64)
        last = size
        it += 1
    if it >= max_it:
        raise ValueError("the reference iteration did not stagnate in %d steps" % max_it)
    root = x.astype(T) + dX
    Kinv = np.abs(np.linalg.inv(K.astype(np.float64))).astype(T)
    E_F = np.abs(F0) + np.abs(F_env) + np.abs(K_hs) @ np.abs(root - x_ref) + m["EF"][0]
    return dict(x=root, iterations=it, K=K, Kinv_abs=Kinv, E_F=E_F, bound=Kinv @ E_F, moor=m)


def _multiples(v, ref, scale):
    v, ref, scale = (np.asarray(a, dtype=np.longdouble) for a in (v, ref, scale))
    out = np.full(6, np.inf)
    zero = scale == 0
    out[zero & (v == ref)] = 0.0
    ok = ~zero & np.isfinite(v.astype(np.float64))
    out[ok] = (np.abs(v[ok] - ref[ok]) / (EPS * scale[ok])).astype(np.float64)
    return out


def pose_multiples(x, ref):
    """|x - x*|_i / (eps (|K^-1| E_F)_i), [6]; a non-finite x gives inf; where the bound is 0 the component must be exact."""
    return _multiples(x, ref["x"], ref["bound"])


def residual_multiples(Y, ref):
    """|Y|_i / (eps E_F_i), [6], with the same conventions."""
    return _multiples(Y, np.zeros(6), ref["E_F"])
