/* raftx_statics.h -- the mean equilibrium pose of rigid 6-DOF designs with mooring lines of their own (libraftx_hip.so only).
 *
 * Replaces, per unit, the solve of Model.solveStatics (raft_model.py:550-963) for staticsMod == 0 and forcingMod == 0:
 *     Y(x) = F0 + F_env - K_hs (x - x_ref) + F_moor(x) = 0
 * by Newton's iteration x <- x + (K_hs + C_moor(x))^-1 Y(x) from x = x_ref, with F_moor and the exact C_moor of
 * include/raftx_mooring.h (the same line types; every line solved from a cold start at every iterate) and the reference's
 * safeguards (raft_model.py:824-861, :667), per step:
 *     a zero diagonal entry of K takes the mean of the diagonal;
 *     dX = K^-1 Y by LU with partial pivoting; while dX.Y < 0 the diagonal grows by 10 % and the solve is repeated, at
 *     most ten times;
 *     dX is scaled by ONE factor so that no component exceeds 30 m (surge, sway), 5 m (heave), 0.1 rad (rotations).
 * The iteration has converged when that step's translations are <= tol[0] and its rotations <= tol[1]; the step is still
 * taken.  The reference stops at 0.05 m / 0.005 rad after a damped walk (dsolve2); here the default is the root to 1e-9 m /
 * 1e-10 rad.  The rotations of the pose are (roll, pitch, yaw) as everywhere in raftx.h; the Newton step adds the
 * rotation-vector increment to them, as the reference does.
 *
 * Not covered: staticsMod / forcingMod 1 (hydrostatics and loads re-evaluated at the pose), arrays with shared lines,
 * flexible units, and feeding the pose into a sweep crossing -- the pose is returned to the caller.
 */
#ifndef RAFTX_STATICS_H
#define RAFTX_STATICS_H

#include "raftx_mooring.h"

/* flags [nDesign]: the RAFTX_MOOR_* bits of the iterate that raised them (raftx_mooring.h: 1, 2, 4, 8), and */
#define RAFTX_STATICS_POSE_CAP   16   /* max_iter steps were taken and the last one was not within tol */
#define RAFTX_STATICS_SINGULAR   32   /* a zero or non-finite pivot, or a non-finite step */

#ifdef __cplusplus
extern "C" {
#endif

/* One launch for the whole iteration of the whole batch.
 *   lines   [nDesign,nLine,RAFTX_ML_N], or NULL: the records of the installed mooring program (raftx_mooring_program) fed
 *           params [nDesign,nParam] -- what raftx_mooring_expand writes; nLine must be the program's.  params is read only then.
 *   depth   > 0
 *   K_hs    [nDesign,6,6]  C_struc + C_hydro (+ C_elast)
 *   F0      [nDesign,6]    W_struc + W_hydro + f0_additional
 *   F_env   [nDesign,6] or NULL (zero): thrust, D_hydro (raftx_current_loads), mean drift
 *   x_ref   [nDesign,6] or NULL (zero): the start pose and the origin of the hydrostatic reaction
 *   tol     {m, rad} or NULL: 1e-9, 1e-10.   max_iter <= 0: 40.
 * Outputs, each of which may be NULL except flags: pose [nDesign,6]; C_moor [nDesign,6,6], F_moor [nDesign,6],
 * T [nDesign,2 nLine], J [nDesign,2 nLine,6] and the residual F_res = Y [nDesign,6] evaluated once more at the returned
 * pose -- C_moor, F_moor, T and J are bit for bit what raftx_mooring_lines gives there; iterations [nDesign], the steps
 * taken; flags [nDesign].  A flagged design's outputs are NaN, and only its own; iterations stays the count.  A design's
 * bits depend on its own inputs only.
 * Errors, before any launch: nLine < 1, nDesign < 0, NULL K_hs, F0 or flags, a depth that is not positive and finite, a
 * tolerance that is negative or not finite, a line with CB != 0, lines == NULL without a mooring program, with another nLine, or without params. */
int raftx_mean_pose(raftx_ctx *ctx, int nDesign, int nLine, const double *lines, const double *params, double depth,
                    const double *K_hs, const double *F0, const double *F_env, const double *x_ref, const double tol[2],
                    int max_iter, double *pose, double *C_moor, double *F_moor, double *T, double *J, double *F_res,
                    int32_t *iterations, int32_t *flags);

#ifdef __cplusplus
}
#endif

#endif /* RAFTX_STATICS_H */
