"""Independent mean-pose solve for staticsMod 1 (raftx_mean_pose_nonlinear, include/raftx_statics.h) in
``numpy.longdouble``: the reference of tests/test_statics_nl.py and tests/test_hip_statics_nl.py.

    Y(x) = W_struc(x) + W_hydro(x) + W_pm(x) + F_extra - C_extra (x - x_ref) + F_env + F_moor(x)
    K(x) = C_struc(x) + C_hydro(x) + C_pm(x) + C_extra + C_moor(x)                               x <- x + K^-1 Y

The member terms come from tests/geom_reference.py (``design_reference(pose=x)``), the lines from
tests/mooring_reference.py (``evaluate``), the point masses from ``point_masses`` below: written from the formula in
include/raftx_statics.h, not from the kernel.  Both evaluations take fp64 poses, so the iterates live on the fp64 grid.

K is NOT the exact Jacobian of Y (the reference procedure's stiffness is not: the waterplane width it interpolates, AWP /
cos(phi), rotation-vector increments added to Euler angles), so the iteration converges linearly.  It runs until the step
no longer shrinks (and is below ``STAGNANT``: the first steps may grow); ``rho_hat`` is the ratio of the last two steps before that, in the norm the steps are measured in (the
largest component after scaling translations by 1 and rotations by 10, the ratio of the default tolerances).  The returned
root is the last iterate plus the last step, in longdouble; what is left is about rho_hat / (1 - rho_hat) of a step that is
already at the fp64 grid's size.

Envelopes.  ``evaluate`` returns every addend of Y with its envelope (module docstring of tests/geom_reference.py; EF of
tests/mooring_reference.py); E_F is their sum, E_K that of K.  Gates, per entry:
    evaluation    |F_res, K_hs, F0 of the solver at ITS pose - this file's evaluation at that pose| <= G eps E
    convergence   |x - x*|_i <= rho_hat / (1 - rho_hat) tol_i + G eps (|K^-1| E_F)_i
"""
import numpy as np

from . import geom_reference as gr
from . import mooring_reference as mr

EPS = mr.EPS
T = np.longdouble

# G = the power of two at or above 4 x the worst multiple of the fp64 model (tests/statics_nl_device_model.py) over the cases
# of tests/statics_nl_cases.py, the rule of DESIGN section 4.  Measured by
# tests/test_statics_nl.py::test_gate_constant_is_the_measured_one: F_res 0.34 (tapered columns at the waterline), K_hs 0.26,
# F0 0.16; the pose is inside rho_hat / (1 - rho_hat) tol in every case, so the convergence gate's second term measures 0.
GATE_WORST_CPU = 0.35
GATE = 2


def apply_drho(stations, drho):
    """The station rows of a unit trimmed by ``drho`` (raft_model.py:1780-1787, 1810-1817): zero-density ballast sections lose
    their fill, the others gain drho.  fp64 rows in, fp64 rows out: rho_fill + drho is ONE rounded sum, as the procedure's."""
    out = []
    for s in stations:
        s = np.array(s, dtype=np.float64)
        if len(s):
            s[s[:, gr.GS_RHOFILL] == 0.0, gr.GS_LFILL] = 0.0
            fill = s[:, gr.GS_LFILL] > 0.0
            s[fill, gr.GS_RHOFILL] = s[fill, gr.GS_RHOFILL] + drho
        out.append(s)
    return out


def rotation(ang, dtype=T):
    """The platform rotation R_p(roll, pitch, yaw) = Rz(yaw) Ry(pitch) Rx(roll) (helpers.py:439-466)."""
    r, p, y = (dtype(a) for a in ang)
    Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]], dtype=dtype)
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]], dtype=dtype)
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]], dtype=dtype)
    return Rz @ Ry @ Rx


def point_masses(pm, x, g, dtype=T, seed=None):
    """(W [6], C [6,6], EW, EC) of the point masses pm [nPM,4] = (mass, r) at the pose x: a node with the force f = (0, 0, -m g)
    at the arm a = R_p r;  W = (f, a x f);  C[3+i,3+j] -= (dA_j x f)_i with dA_j = r + (theta + e_j) x a - a;  C symmetrised.
    The envelopes are the sums of the magnitudes of the addends."""
    W, C, EW, EC = np.zeros(6, dtype=dtype), np.zeros((6, 6), dtype=dtype), np.zeros(6, dtype=dtype), np.zeros((6, 6), dtype=dtype)
    x = np.asarray(x, dtype=np.float64)
    R = np.eye(3, dtype=dtype) if seed == "pm_arm_not_rotated" else rotation(x[3:], dtype)
    th = x[3:].astype(dtype)
    for row in np.asarray(pm, dtype=np.float64).reshape(-1, 4):
        m, r = dtype(row[0]), row[1:].astype(dtype)
        a, ea = R @ r, np.abs(R) @ np.abs(r)
        f = np.array([0, 0, -m * dtype(g)], dtype=dtype)
        W[:3] += f
        EW[:3] += np.abs(f)
        W[3:] += np.cross(a, f)
        EW[3:] += np.array([ea[1] * abs(f[2]), ea[0] * abs(f[2]), 0], dtype=dtype)
        for j in range(3):
            tj = th.copy()
            tj[j] += 1
            dA = r + np.cross(tj, a) - a
            edA = np.abs(r) + np.array([abs(tj[1]) * ea[2] + abs(tj[2]) * ea[1], abs(tj[2]) * ea[0] + abs(tj[0]) * ea[2],
                                        abs(tj[0]) * ea[1] + abs(tj[1]) * ea[0]], dtype=dtype) + ea
            C[3:, 3 + j] -= np.cross(dA, f)
            EC[3:, 3 + j] += np.array([edA[1] * abs(f[2]), edA[0] * abs(f[2]), 0], dtype=dtype)
    return W, (C + C.T) / 2, EW, (EC + EC.T) / 2


def evaluate(case, x, dtype=T, seed=None):
    """Everything at the fp64 pose x: dict Y, K, K_hs, F0, moor (C, F, T, J of tests/mooring_reference.py) and the envelopes
    E_F (of Y and of F0: the lines' share apart in E_moor), E_K (of K_hs), plus ``decisions`` of the geometry.  ``seed``: a
    deliberate error (tests of the gates only)."""
    x = np.asarray(x, dtype=np.float64)
    x_ref = np.asarray(case["x_ref"], dtype=np.float64)
    stations = case["stations"]
    if case["drho"] is not None and seed != "drho_ignored":
        stations = apply_drho(stations, case["drho"])
    geo = gr.design_reference(case["members"], stations, case["caps"], x_ref if seed == "frozen_hydrostatics" else x, case["rho"],
                              case["g"], dtype=dtype)
    D, E = geo.D, geo.E
    F0 = (D["W_struc"] + D["W_hydro"]).astype(dtype)
    E0 = (E["W_struc"] + E["W_hydro"]).astype(dtype)
    Kh = (D["C_struc"] + D["C_hydro"]).astype(dtype)
    EK = (E["C_struc"] + E["C_hydro"]).astype(dtype)
    if seed == "frozen_hydrostatics":                             # staticsMod 0 passed off as staticsMod 1
        dxr = (x - x_ref).astype(dtype)
        F0, E0 = F0 - Kh @ dxr, E0 + np.abs(Kh) @ np.abs(dxr)
    if len(case["pm"]):
        W, C, EW, EC = point_masses(case["pm"], x, case["g"], dtype, seed)
        F0, E0, Kh, EK = F0 + W, E0 + EW, Kh + C, EK + EC
    if case["C_extra"] is not None:
        Kh, EK = Kh + case["C_extra"].astype(dtype), EK + np.abs(case["C_extra"]).astype(dtype)
    if case["F_extra"] is not None:
        F0, E0 = F0 + case["F_extra"].astype(dtype), E0 + np.abs(case["F_extra"]).astype(dtype)
    m = mr.evaluate(case["lines"][None], x[None], case["depth"], dtype)
    if m["flags"][0]:
        raise ValueError("the mooring reference flags the pose %s: %d" % (x, m["flags"][0]))
    dx = (x - x_ref).astype(dtype)
    Y, EY = F0 + case["F_env"].astype(dtype) + m["F"][0], E0 + np.abs(case["F_env"]).astype(dtype) + m["EF"][0].astype(dtype)
    if case["C_extra"] is not None:
        Y, EY = Y - case["C_extra"].astype(dtype) @ dx, EY + np.abs(case["C_extra"]).astype(dtype) @ np.abs(dx)
    return dict(Y=Y, K=Kh + m["C"][0], K_hs=Kh, F0=F0, E_F=EY, E_F0=E0, E_K=EK, moor=m, decisions=geo.decisions)


def _solve(K, Y):
    """K^-1 Y in longdouble: an fp64 solve refined three times."""
    K64 = K.astype(np.float64)
    x = np.linalg.solve(K64, Y.astype(np.float64)).astype(T)
    for _ in range(3):
        x = x + np.linalg.solve(K64, (Y - K @ x).astype(np.float64)).astype(T)
    return x


STEP_SCALE = np.array([1.0, 1.0, 1.0, 10.0, 10.0, 10.0])
STAGNANT = 1e-10                  # a step that does not shrink ends the iteration only below this size: the first steps may grow


def solve(case, max_it=120, seed=None):
    """dict of the root x [6] (longdouble), iterations, rho_hat, the evaluation ``at`` the fp64 rounding of the root, Kinv_abs
    = |K^-1| there, E_F and bound = |K^-1| E_F."""
    x = np.asarray(case["x_ref"], dtype=np.float64).copy()
    sizes, it = [], 0
    while True:
        ev = evaluate(case, x, T, seed)
        dX = _solve(ev["K"], ev["Y"])
        size = float(np.max(np.abs(dX) * STEP_SCALE))
        if (sizes and size >= sizes[-1] and size < STAGNANT) or size == 0.0 or it >= max_it:
            break
        x = (x.astype(T) + dX).astype(np.float64)
        sizes.append(size)
        it += 1
    if it >= max_it:
        raise ValueError("the reference iteration did not stagnate in %d steps" % max_it)
    # the ratio of successive steps while they are well above the fp64 grid of the pose (the last few are rounding)
    clean = [s for s in sizes if s > 1e-11]
    rho_hat = max(b / a for a, b in zip(clean[-4:-1], clean[-3:])) if len(clean) >= 4 else 0.0
    Kinv = np.abs(np.linalg.inv(ev["K"].astype(np.float64))).astype(T)
    return dict(x=x.astype(T) + dX, iterations=it, rho_hat=float(rho_hat), at=ev, Kinv_abs=Kinv, E_F=ev["E_F"], bound=Kinv @ ev["E_F"],
                sizes=sizes)


def multiples(v, ref, E):
    """|v - ref| / (eps E) per entry, with the conventions of geom_reference.gate_multiples."""
    return gr.gate_multiples(v, ref, E)


def evaluation_multiples(case, res):
    """The evaluation gate on a solver's result ``res`` (pose, F_res, K_hs, F0): dict of the multiples of eps E per entry
    against this file's evaluation AT THE SOLVER'S POSE."""
    ev = evaluate(case, np.asarray(res["pose"], dtype=np.float64))
    return dict(F_res=multiples(res["F_res"], ev["Y"], ev["E_F"]), K_hs=multiples(res["K_hs"], ev["K_hs"], ev["E_K"]),
                F0=multiples(res["F0"], ev["F0"], ev["E_F0"]))


def convergence_excess(x, ref, tol):
    """(|x - x*| - rho_hat / (1 - rho_hat) tol) / (eps |K^-1| E_F) per component: the convergence gate holds where this is
    <= G.  A non-finite x gives inf."""
    x = np.asarray(x, dtype=T)
    tolv = np.array([tol[0]] * 3 + [tol[1]] * 3, dtype=T)
    r = ref["rho_hat"]
    err = np.abs(x - ref["x"]) - (r / (1 - r)) * tolv
    out = np.full(6, np.inf)
    ok = np.isfinite(x.astype(np.float64))
    out[ok] = (np.maximum(err[ok], 0) / (EPS * ref["bound"][ok])).astype(np.float64)
    return out
