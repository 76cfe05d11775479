"""The mean equilibrium pose of every design on the device (include/raftx_statics.h): Model.solveStatics for staticsMod 0
and 1 / forcingMod 0, rigid 6-DOF units with mooring lines of their own.

``hydrostatics(ctx, ...)`` assembles K_hs and F0 of the resident design set from raftx_fetch_statics and the caller's
terms that do not come from the geometry; ``mean_pose(ctx, ...)`` runs the one-launch Newton solve and returns a
``MeanPose``.
"""
import numpy as np

from . import mooring

FLAG_POSE_CAP, FLAG_SINGULAR, FLAG_BAD_MEMBER = 16, 32, 128
FLAG_NAMES = {mooring.FLAG_BAD_LINE: "bad line", mooring.FLAG_VERTICAL: "vertical line", mooring.FLAG_SLACK: "slack line",
              mooring.FLAG_NO_CONVERGENCE: "line not converged", FLAG_POSE_CAP: "pose iteration cap", FLAG_SINGULAR: "singular system",
              FLAG_BAD_MEMBER: "member refused at an iterate"}


class MeanPose:
    """Result of ``mean_pose``: pose [nD,6] (m, rad), C_moor [nD,6,6], F_moor [nD,6], T [nD,2 nLine] (ends A, then ends
    B), J [nD,2 nLine,6], F_res [nD,6] (the residual at the pose), iterations [nD], flags [nD].  A flagged design's rows
    are NaN.  With ``statics_mod=1`` also K_hs [nD,6,6] and F0 [nD,6], the hydrostatics at the pose (else None)."""

    def __init__(self, res):
        self.pose, self.C_moor, self.F_moor = res["pose"], res["C"], res["F"]
        self.T, self.J, self.F_res = res["T"], res["J"], res["F_res"]
        self.iterations, self.flags = res["iterations"], res["flags"]
        self.K_hs, self.F0 = res.get("K_hs"), res.get("F0")

    @property
    def ok(self):
        """[nD] bool: the design converged and none of its lines was flagged."""
        return self.flags == 0

    def describe_flags(self, d):
        return [name for bit, name in FLAG_NAMES.items() if int(self.flags[d]) & bit]


def hydrostatics(ctx, C_extra=None, F_extra=None, current=None):
    """(K_hs [nD,6,6], F0 [nD,6], F_env [nD,6] or None) of the resident design set (after a design build):
    K_hs = C_struc + C_hydro + ``C_extra`` (the elastic stiffness, the turbine's share, ...), F0 = W_struc + W_hydro +
    ``F_extra`` (f0_additional, the turbine's weight, ...), each extra [6,6] / [6] or per design.  ``current`` =
    dict(speed=, heading=, depth=, Zref=None, shearExp=0.12) makes the library evaluate the mean current load of that ONE
    current (raftx_current_loads) and return it as F_env."""
    st = ctx.fetch_statics()
    K_hs = st["C_struc"] + st["C_hydro"]
    F0 = st["W_struc"] + st["W_hydro"]
    if C_extra is not None:
        K_hs = K_hs + np.asarray(C_extra, dtype=float)
    if F_extra is not None:
        F0 = F0 + np.asarray(F_extra, dtype=float)
    F_env = None
    if current is not None:
        cur = dict(current)
        D = ctx.current_loads([float(cur.pop("speed"))], [float(cur.pop("heading"))], float(cur.pop("depth")), **cur)
        F_env = np.ascontiguousarray(D[:, 0, :])
    return np.ascontiguousarray(K_hs), np.ascontiguousarray(F0), F_env


def mean_pose(ctx, K_hs=None, F0=None, lines=None, depth=None, program=None, params=None, F_env=None, x_ref=None, tol=None, max_iter=0,
              statics_mod=0, designs=None, point_masses=None, drho=None, C_extra=None, F_extra=None, rho=1025.0, g=9.81):
    """Newton's iteration on the mean equilibrium of every design in one launch.  Give either ``lines`` [nD,nLine,16]
    (raft_amd.mooring.lines_from_design), or ``program`` (a MooringProgram, installed here unless it already is; None keeps
    the installed one) with ``params`` [nD,nParam].  ``tol`` = (m, rad), None: 1e-9, 1e-10.

    ``statics_mod=0``: F0 + F_env - K_hs (x - x_ref) + F_moor(x) = 0 with the hydrostatics ``K_hs``, ``F0`` linearised at
    ``x_ref`` (``hydrostatics``).

    ``statics_mod=1``: buoyancy and weight are re-evaluated from the geometry at every iterate.  ``designs`` is a
    raft_amd.geometry batch (member_off, members, station_off, stations, cap_off, caps), or the variant parameters
    [nD,nParam] of the variant program installed on ``ctx`` (they also feed the mooring program when ``lines`` is None).
    ``K_hs`` / ``F0`` are not given; ``C_extra`` / ``F_extra`` are the CONSTANT terms ([6,6] / [6] or per design: C_elast,
    f0_additional), ``point_masses`` [nPM,4] or [nD,nPM,4] (mass, x, y, z about the PRP), ``drho`` [nD] the ballast-density correction of a
    trim made at ``x_ref``.  The result carries K_hs and F0 at the returned pose."""
    if depth is None:
        raise ValueError("mean_pose: the water depth is required")
    if statics_mod not in (0, 1):
        raise ValueError("mean_pose: statics_mod must be 0 or 1 (got %r)" % (statics_mod,))
    if statics_mod == 1:
        if K_hs is not None or F0 is not None:
            raise ValueError("mean_pose: statics_mod=1 evaluates K_hs and F0 itself (constant terms: C_extra, F_extra)")
        if designs is None:
            raise ValueError("mean_pose: statics_mod=1 needs designs (a MemberTable batch, or variant parameters)")
        variants = not hasattr(designs, "member_off")
        if lines is None:
            if not variants:
                raise ValueError("mean_pose: statics_mod=1 on a MemberTable batch needs lines")
            if params is not None and not np.array_equal(np.asarray(params, dtype=float), np.asarray(designs, dtype=float)):
                raise ValueError("mean_pose: statics_mod=1 feeds the mooring program the variant parameters: params must be None or designs")
            if program is not None and getattr(ctx, "_mprog_owner", None) is not program:
                ctx.mooring_program(program)
        elif params is not None or program is not None:
            raise ValueError("mean_pose: lines and a mooring program exclude each other")
        kw = dict(params=designs) if variants else dict(tables=designs)
        return MeanPose(ctx.mean_pose_nonlinear(depth, lines=lines, rho=rho, g=g, drho=drho, point_masses=point_masses, C_extra=C_extra,
                                                F_extra=F_extra, F_env=F_env, x_ref=x_ref, tol=tol, max_iter=max_iter, **kw))
    if any(a is not None for a in (designs, point_masses, drho, C_extra, F_extra)):
        raise ValueError("mean_pose: designs, point_masses, drho, C_extra and F_extra belong to statics_mod=1")
    if lines is None:
        if params is None:
            raise ValueError("mean_pose: give lines, or a mooring program's params")
        if program is not None and getattr(ctx, "_mprog_owner", None) is not program:
            ctx.mooring_program(program)
    elif params is not None or program is not None:
        raise ValueError("mean_pose: lines and a mooring program exclude each other")
    return MeanPose(ctx.mean_pose(K_hs, F0, depth, lines=lines, params=params, F_env=F_env, x_ref=x_ref, tol=tol, max_iter=max_iter))


class ArrayMeanPose:
    """Result of ``array_mean_pose``: pose [nA,nUnit,6], C [nA,6 nUnit,6 nUnit] (the layout of Cc of solve_system), F
    [nA,6 nUnit], T [nA,2 nLine], J [nA,2 nLine,6 nUnit], F_res [nA,6 nUnit], iterations [nA], flags [nA].  A flagged
    array's rows are NaN."""

    def __init__(self, res):
        self.pose, self.C, self.F = res["pose"], res["C"], res["F"]
        self.T, self.J, self.F_res = res["T"], res["J"], res["F_res"]
        self.iterations, self.flags = res["iterations"], res["flags"]

    @property
    def ok(self):
        """[nA] bool: the array converged and none of its rows was flagged."""
        return self.flags == 0

    def describe_flags(self, a):
        names = dict(FLAG_NAMES)
        names[mooring.FLAG_GROUNDED] = "line on or below the seabed"
        return [name for bit, name in names.items() if int(self.flags[a]) & bit]


def array_mean_pose(ctx, K_hs, F0, lines, locations, depth, F_env=None, tol=None, max_iter=0):
    """Newton's iteration over the 6 nUnit DOFs of every array in one launch (include/raftx_array_mooring.h; Model.solveStatics
    of a farm, raft_model.py:678-885, staticsMod 0 / forcingMod 0).  ``K_hs`` [nA,nUnit,6,6], ``F0`` [nA,nUnit,6], ``lines``
    [nA,nRow,16] array rows (raft_amd.mooring.array_lines), ``locations`` [nUnit,2] or [nA,nUnit,2] (x_location, y_location) or
    full reference poses [nA,nUnit,6], ``F_env`` [nA,nUnit,6] or None."""
    K_hs = np.asarray(K_hs, dtype=float)
    nA, nU = K_hs.shape[:2]
    loc = np.asarray(locations, dtype=float)
    if loc.shape[-1] == 2:
        x_ref = np.zeros((nA, nU, 6))
        x_ref[..., :2] = np.broadcast_to(loc, (nA, nU, 2))
    else:
        x_ref = np.broadcast_to(loc, (nA, nU, 6))
    return ArrayMeanPose(ctx.array_mean_pose(K_hs, F0, np.ascontiguousarray(x_ref), depth, lines, F_env=F_env, tol=tol, max_iter=max_iter))


MODAL_FLAG_NAMES = {1: "small diagonal", 2: "eigenvalue <= 0", 4: "complex eigenvalues", 8: "singular mass matrix",
                    16: "QR iteration not converged"}


class ArrayModes:
    """Result of ``array_modes``: fn [nA,n] (Hz) and periods [nA,n] (s) in DOF order (n = 6 nUnit, unit-major), modes [nA,n,n]
    (column j: the unit-norm mode of fn[j]), C [nA,n,n] (the stiffness the modes belong to: blockdiag(K_hs) + the array
    mooring stiffness at the pose), flags [nA] (the eigen solver's), moor_flags [nA] (the lines').  An array with a mooring
    flag, or an eigen flag other than "small diagonal", is NaN."""

    def __init__(self, res):
        self.fn, self.modes, self.C = res["fn"], res["modes"], res["C"]
        self.flags, self.moor_flags = res["flags"], res["moor_flags"]

    @property
    def periods(self):
        return 1.0 / self.fn

    @property
    def ok(self):
        """[nA] bool: no line was flagged and the eigen analysis returned numbers."""
        return (self.moor_flags == 0) & ((self.flags & ~1) == 0)

    def describe_flags(self, a):
        names = dict(FLAG_NAMES)
        names[mooring.FLAG_GROUNDED] = "line on or below the seabed"
        return ([name for bit, name in names.items() if int(self.moor_flags[a]) & bit] +
                [name for bit, name in MODAL_FLAG_NAMES.items() if int(self.flags[a]) & bit])


def array_modes(ctx, M_unit, K_hs, lines, pose, depth, dC=None):
    """Natural frequencies and modes of every moored array over all 6 nUnit DOFs at the given poses, composed on the device
    (include/raftx_array_modal.h; Model.solveEigen of a farm, raft_model.py:436-547).  ``M_unit`` [nA,nUnit,6,6] (structure +
    added mass per unit), ``K_hs`` [nA,nUnit,6,6] (each unit's own stiffness), ``lines`` [nA,nRow,16] array rows
    (raft_amd.mooring.array_lines), ``pose`` [nA,nUnit,6] (``array_mean_pose(...).pose`` when it is not known), ``dC``
    [nA,n,n] or None: further stiffness over all DOFs."""
    return ArrayModes(ctx.array_modal_moored(M_unit, K_hs, lines, pose, depth, dC=dC))
