"""fp64 restatement of k_mean_pose_nl (raft_amd/csrc/raftx_statics.h), one design at a time: the member terms from
``geom_reference.design_reference(dtype=float64)`` -- the reference procedure's own operation order, which the device
functions keep --, the lines from tests/mooring_device_model.py through ``mean_pose_device_model.moor``, the point masses in
fp64, the sums in the kernel's association, and ``mean_pose_device_model.step``.  It is what the gate's constant of
tests/statics_nl_reference.py is measured with on the CPU and, through ``seed``, the carrier of the deliberate errors the
gates must reject.  The kernel uses the device's library functions and contracts the multiply-adds of the line and step
parts, so the model agrees with it to rounding, not to the bit.
"""
import numpy as np

from . import geom_reference as gr
from . import mean_pose_device_model as mp
from . import statics_nl_reference as nr

FLAG_BAD_MEMBER = 128
SEEDS = ("frozen_hydrostatics", "pm_arm_not_rotated", "drho_ignored")


def hydrostatics(case, x, seed=None):
    """(K_hs [6,6], F0 [6]) at x in fp64, in the kernel's order: (C_struc + C_hydro) + C_pm + C_extra, (W_struc + W_hydro) +
    W_pm + F_extra."""
    stations = case["stations"]
    if case["drho"] is not None and seed != "drho_ignored":
        stations = nr.apply_drho(stations, case["drho"])
    at = case["x_ref"] if seed == "frozen_hydrostatics" else x
    D = gr.design_reference(case["members"], stations, case["caps"], at, case["rho"], case["g"], dtype=np.float64).D
    Kh = np.asarray(D["C_struc"] + D["C_hydro"], dtype=np.float64)
    F0 = np.asarray(D["W_struc"] + D["W_hydro"], dtype=np.float64)
    if seed == "frozen_hydrostatics":
        F0 = F0 - Kh @ (np.asarray(x, dtype=np.float64) - case["x_ref"])
    if len(case["pm"]):
        W, C, _, _ = nr.point_masses(case["pm"], x, case["g"], np.float64, seed)
        Kh, F0 = Kh + C, F0 + W
    if case["C_extra"] is not None:
        Kh = Kh + case["C_extra"]
    if case["F_extra"] is not None:
        F0 = F0 + case["F_extra"]
    return Kh, F0


def residual(case, x, F0, Fm):
    Y = np.zeros(6)
    for i in range(6):
        acc = 0.0
        if case["C_extra"] is not None:
            for j in range(6):
                acc = acc + case["C_extra"][i, j] * (x[j] - case["x_ref"][j])
        Y[i] = ((F0[i] - acc) + case["F_env"][i]) + Fm[i]
    return Y


def solve(case, tol=None, max_iter=0, seed=None):
    """dict pose, K_hs, F0, C, F, T, J, F_res, iterations, flags as raftx_mean_pose_nonlinear gives them for ONE design."""
    assert seed is None or seed in SEEDS
    tol = mp.TOL if tol is None else tol
    max_iter = mp.MAX_ITER if max_iter <= 0 else max_iter
    nL = len(case["lines"])
    x, it, flag, final = np.asarray(case["x_ref"], dtype=np.float64).copy(), 0, 0, False
    nan = dict(pose=np.full(6, np.nan), K_hs=np.full((6, 6), np.nan), F0=np.full(6, np.nan), C=np.full((6, 6), np.nan),
               F=np.full(6, np.nan), T=np.full(2 * nL, np.nan), J=np.full((2 * nL, 6), np.nan), F_res=np.full(6, np.nan))
    while True:
        if not np.all(np.isfinite(x)):
            flag |= mp.FLAG_SINGULAR
            break
        fl, C, Fm, Tn, J = mp.moor(case["lines"], x, case["depth"])
        try:
            Kh, F0 = hydrostatics(case, x, seed)
        except (gr.Refused, ValueError, IndexError):
            fl |= FLAG_BAD_MEMBER
        if fl:
            flag |= fl
            break
        Y = residual(case, x, F0, Fm)
        if final:
            return dict(pose=x, K_hs=Kh, F0=F0, C=C, F=Fm, T=Tn, J=J, F_res=Y, iterations=it, flags=0)
        dX, sing = mp.step(Kh + C, Y)
        if sing:
            flag |= mp.FLAG_SINGULAR
            break
        conv = all(abs(dX[i]) <= tol[0 if i < 3 else 1] for i in range(6))
        x = x + dX
        it += 1
        if conv:
            final = True
        elif it >= max_iter:
            flag |= mp.FLAG_POSE_CAP
            break
    nan.update(iterations=it, flags=flag)
    return nan
