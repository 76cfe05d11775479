/* raftx_statics_nl.h -- the mean equilibrium pose with hydrostatics at every iterate: Model.solveStatics for staticsMod == 1
 * (raft_model.py:705-712, :797-800), forcingMod == 0 (libraftx_hip.so only).  raftx_statics.h includes this file at its end: include
 * raftx_statics.h, whose flags, line records, step and safeguards these entries share.
 */
#ifndef RAFTX_STATICS_NL_H
#define RAFTX_STATICS_NL_H

#include "raftx_mooring.h"

#ifdef __cplusplus
extern "C" {
#endif

/* staticsMod == 1: hydrostatics at every iterate.  One launch for the whole iteration of the whole batch, from the
 * descriptors themselves (the member, station and cap rows of raftx_build_designs); no resident state is read or left.
 *     Y(x) = W_struc(x) + W_hydro(x) + W_pm(x) + F_extra - C_extra (x - x_ref) + F_env + F_moor(x)
 *     K(x) = C_struc(x) + C_hydro(x) + C_pm(x) + C_extra + C_moor(x)
 * W_struc, W_hydro, C_struc, C_hydro are what raftx_build_designs(pose = x) leaves for raftx_fetch_statics, bit for bit.
 * The step, its safeguards, the convergence rule, the tolerances, the lines and the flags are those of raftx_mean_pose.
 *   memberOff [nDesign+1], members, stationOff [nMember+1], stations, capOff [nMember+1] or NULL, caps: as
 *           raftx_build_designs takes them (memberOff[0] may be an offset into the arrays)
 *   rho, g  positive and finite
 *   drho    [nDesign] or NULL: the ballast-density correction of a trim made at x_ref (props[RAFTX_SP_DRHO] of a build with
 *           RAFTX_TRIM_BALLAST): zero-density ballast sections lose their fill, the others gain drho.  The trim is not
 *           solved again at an iterate (adjustBallastDensity precedes solveStatics).
 *   lines   [nDesign,nLine,RAFTX_ML_N]; depth > 0
 *   pm      [nX,nPM,4] point masses (mass, x, y, z: the position about the PRP in the unit's frame) -- the RNA, pointInertias.
 *           A point mass is a node that carries weight only.  With R_p the platform rotation at x, a = R_p r, f = (0, 0, -m g):
 *               W_pm += (f, a x f)
 *               C_pm[3+i,3+j] -= (dA_j x f)_i,  dA_j = r + (theta + e_j) x a - a,  theta = x[3:6]
 *           and C_pm is symmetrised: the member -> platform reduction of a node force.  At theta = 0 this is
 *           C[3,3] = C[4,4] = -m g r_z (getWeightOfPointMass) and C[3,5] = C[5,3] = m g r_x / 2, C[4,5] = C[5,4] = m g r_y / 2.
 *   C_extra [nX,6,6], F_extra [nX,6]: constant terms (C_elast, f0_additional); nX = 0: no pm / C_extra / F_extra, 1: shared,
 *           nDesign: one set each; with nX > 0 C_extra and F_extra may each be NULL, and pm when nPM == 0
 *   F_env, x_ref, tol, max_iter: as raftx_mean_pose
 * Outputs as raftx_mean_pose, and K_hs [nDesign,6,6] = C_struc + C_hydro (+ C_pm) (+ C_extra), F0 [nDesign,6] = W_struc +
 * W_hydro (+ W_pm) (+ F_extra), summed in this order; with the mooring outputs and F_res they are evaluated once more at
 * the returned pose.  Each may be NULL except flags.  Flags: those of raftx_mean_pose; RAFTX_STATICS_SINGULAR also for a pose
 * that is not finite (a NaN x_ref: the member pass never sees it); RAFTX_STATICS_BAD_MEMBER for a member with fewer than two
 * stations, dlsMax <= 0, no length or a cap layout the reference refuses.  A flagged design is NaN, alone; a design's bits
 * depend on its own inputs only.
 * Errors, before any launch: those of raftx_mean_pose; NULL or non-monotone offsets, NULL rows; nX not 0, 1 or nDesign;
 * nPM < 0, or pm == NULL with nX > 0 and nPM > 0; rho or g not positive and finite; lines == NULL. */
int raftx_mean_pose_nonlinear(raftx_ctx *ctx, int nDesign, const int64_t *memberOff, const double *members,
                              const int64_t *stationOff, const double *stations, const int64_t *capOff, const double *caps,
                              double rho, double g, const double *drho, int nLine, const double *lines, double depth, int nPM,
                              int nX, const double *pm, const double *C_extra, const double *F_extra, const double *F_env,
                              const double *x_ref, const double tol[2], int max_iter, double *pose, double *K_hs, double *F0,
                              double *C_moor, double *F_moor, double *T, double *J, double *F_res, int32_t *iterations,
                              int32_t *flags);
/* ... for the variants params [nDesign,nParam] of the installed variant program (raftx_variant_program): the rows are
 * evaluated where they are read, the bits of the form above fed raftx_expand_variants' rows.  lines == NULL: the records of
 * the installed mooring program at the same params.  Errors also: no variant program; lines == NULL without a mooring program
 * or with another nLine. */
int raftx_mean_pose_nonlinear_variants(raftx_ctx *ctx, int nDesign, const double *params, double rho, double g,
                                       const double *drho, int nLine, const double *lines, double depth, int nPM, int nX,
                                       const double *pm, const double *C_extra, const double *F_extra, const double *F_env,
                                       const double *x_ref, const double tol[2], int max_iter, double *pose, double *K_hs,
                                       double *F0, double *C_moor, double *F_moor, double *T, double *J, double *F_res,
                                       int32_t *iterations, int32_t *flags);


#ifdef __cplusplus
}
#endif

#endif /* RAFTX_STATICS_NL_H */
