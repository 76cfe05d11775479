/* raftx_array_mooring.h -- the quasi-static mooring system of an ARRAY of rigid 6-DOF units: the lines of every unit and
 * SHARED lines that run from one unit to another (libraftx_hip.so only).
 *
 * Replaces what the reference does with the array-level MoorPy system of a farm (raft_model.py:655-885 for staticsMod ==
 * forcingMod == 0): ms.getCoupledStiffnessA, getForces, getTensions and the tension Jacobian over all 6 nUnit DOFs, and the
 * Newton iteration of Model.solveStatics over them.  C has the layout of Cc of raftx_solve_system[_resident]
 * ([6 nUnit, 6 nUnit], unit-major) and can be passed on as it is.
 *
 * A row is the RAFTX_ML_N record of raftx_mooring.h with two more fields:
 *     11 (RAFTX_ML_UNIT_B)   index 0 .. nUnit-1 of the unit that carries end B; fields 3-5 are in that unit's body frame
 *     12 (RAFTX_ML_UNIT_A)   0: end A is an anchor, fields 0-2 global (the meaning of raftx_mooring.h)
 *                            k >= 1: end A sits on unit k-1 and fields 0-2 are body-frame coordinates relative to that
 *                            unit's reference point -- a SHARED row
 * An anchored row may be a single line, the head row of a composite line or of a bridle, exactly as in raftx_mooring.h;
 * continuation and leg rows inherit the head row's unit (their fields 11-12 must repeat the head row's 11 and be 0).
 * A shared row is ONE suspended elastic catenary: its fields 9, 10, 13, 14, 15 are zero and its two units differ.  It is solved
 * for (HF, VF) at end B; VA = VF - wL at end A may be negative (the line sags below its lower end), ZF = z_B - z_A may have
 * either sign and may be exactly 0, and the ends are never exchanged: no output jumps as ZF crosses 0.  With u the horizontal
 * direction from A to B the force on unit B is (-HF u, -VF) at its arm and the force on unit A (+HF u, +VA) at its arm; with
 * K3 the 3 x 3 stiffness of the relative end motion the four unit blocks are [[K3, -K3], [-K3, K3]], each carried to the
 * reference points with its own arms, the arm-turning term of an end on that unit's diagonal block only.  J of both ends has
 * columns for both units.  A shared line resting on the seabed is not covered.
 *
 * Flags (int32 per array; a flagged array's outputs are NaN, and only its own): the bits of raftx_mooring.h and
 * raftx_statics.h.  For a shared row: BAD_LINE a non-finite field or pose, or L, EA or w <= 0; VERTICAL the horizontal distance
 * of the ends <= 1e-9 L; NO_CONVERGENCE the cap of the line iteration; GROUNDED the lowest point of the line more than
 * 1e-6 depth below the seabed.  A shared row never raises SLACK: between two suspended ends a catenary exists for every length
 * above the chord (a shared line is normally LONGER than XF + |ZF|: 1490 m over 1484 m hang 120 m deep), and the profile that
 * the bit stands for on an anchored line -- all of it lying on the seabed -- is what GROUNDED reports here.
 */
#ifndef RAFTX_ARRAY_MOORING_H
#define RAFTX_ARRAY_MOORING_H

#include "raftx_statics.h"

#define RAFTX_ML_UNIT_B 11
#define RAFTX_ML_UNIT_A 12
#define RAFTX_ARRAY_MAX_UNIT 6         /* 36 DOFs: above that the reference leaves the dense-solve path (raft_model.py:833) */

#ifdef __cplusplus
extern "C" {
#endif

/* Stateless.  lines [nArray,nLine,RAFTX_ML_N], pose [nArray,nUnit,6] (global; m, rad; required), depth > 0.  Outputs, each of
 * which may be NULL except flags, with n = 6 nUnit: C [nArray,n,n], F [nArray,n], T [nArray,2 nLine] (ends A of all rows, then
 * ends B: the order of getTensions), J [nArray,2 nLine,n], line_out [nArray,nLine,8] (as raftx_mooring_lines; a shared row:
 * HF, VF, HF, VA, 0, iterations, 0, 0), flags [nArray].  The sums run in row order without atomics: an array's bits depend on
 * its own rows and poses only.  With nUnit == 1 and no shared row the outputs are those of raftx_mooring_lines, bit for bit.
 * Errors, before any launch: the record errors of raftx_mooring_lines; nUnit outside 1 .. RAFTX_ARRAY_MAX_UNIT; a unit index
 * that is out of range or not an integer; unit A equal to unit B; a shared row with a continuation mark, a leg mark, a joint
 * weight or CB, or followed by a continuation or leg row; a continuation or leg row whose unit fields differ from its head
 * row's; NULL lines, pose or flags; a bad depth. */
int raftx_array_mooring_lines(raftx_ctx *ctx, int nArray, int nUnit, int nLine, const double *lines, const double *pose,
                              double depth, double *C, double *F, double *T, double *J, double *line_out, int32_t *flags);

/* The mean pose of every array in one launch: Newton's iteration on
 *     Y_i(x) = F0_i + F_env_i - K_hs_i (x_i - x_ref_i) + F_i(x) = 0   for the units i,      K = diag(K_hs_i) + C(x)
 * from x = x_ref with the safeguards of raftx_mean_pose applied to the whole 6 nUnit vector: a zero diagonal entry takes the
 * mean over all 6 nUnit diagonal entries; while dX.Y < 0 the whole diagonal grows by 10 %, at most ten times; ONE scale factor
 * against the caps (30, 30, 5 m, 0.1, 0.1, 0.1 rad) repeated per unit; converged when every unit's translations are <= tol[0]
 * and its rotations <= tol[1] (the step is still taken).
 *   K_hs [nArray,nUnit,6,6], F0 [nArray,nUnit,6], F_env [nArray,nUnit,6] or NULL (zero), x_ref [nArray,nUnit,6] (required: the
 *   units' locations), tol {m, rad} or NULL: 1e-9, 1e-10; max_iter <= 0: 40.
 * Outputs, each of which may be NULL except flags: pose [nArray,nUnit,6]; C, F, T, J as above and the residual F_res
 * [nArray,6 nUnit] evaluated once more at the returned pose -- C, F, T, J are bit for bit what raftx_array_mooring_lines gives
 * there; iterations [nArray]; flags [nArray] (also RAFTX_STATICS_POSE_CAP, RAFTX_STATICS_SINGULAR).  A flagged array's outputs
 * are NaN, and only its own; iterations stays the count.
 * Errors, before any launch: those of raftx_array_mooring_lines; NULL K_hs, F0, x_ref or flags; a bad tolerance. */
int raftx_array_mean_pose(raftx_ctx *ctx, int nArray, int nUnit, int nLine, const double *lines, double depth,
                          const double *K_hs, const double *F0, const double *F_env, const double *x_ref, const double tol[2],
                          int max_iter, double *pose, double *C, double *F, double *T, double *J, double *F_res,
                          int32_t *iterations, int32_t *flags);

#ifdef __cplusplus
}
#endif

#endif /* RAFTX_ARRAY_MOORING_H */
