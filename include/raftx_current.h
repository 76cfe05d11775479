/* raftx_current.h -- mean current loads of rigid 6-DOF designs (libraftx_hip.so only).
 *
 * Replaces, per design, what raft_fowt.py:1961-1985 (FOWT.calcCurrentLoads) computes from
 * raft_member.py:1793-1897 (Member.calcCurrentLoads) of every member: the mean Morison drag of a sheared current
 *     v(z) = speed * ((depth - |z|) / (depth + Zref))^shearExp          raft_member.py:1846
 * on every wet strip, summed to six loads about the reduced-DOF reference point (raft_member.py:1896 and the T.T of
 * raft_fowt.py:1983).  Model.solveStatics adds the result to F_env_constant (raft_model.py:621, 735).
 *
 * Everything the sum needs is in the strip records of raftx.h: RAFTX_F_X (z), RAFTX_F_AX (the folded arm),
 * q / p1 / p2, RAFTX_F_CIRC and RAFTX_F_DQ / DP1 / DP2 / DEND = sqrt(8/pi) rho/2 a Cd with the areas of
 * raft_member.py:1867-1869, 1886-1889 (= :2070-2072, 2105-2108).  The rotor tables are not part of it (the underwater
 * rotor's current path, CCBlade, is not covered); Zref is the caller's (the submerged-rotor rule of
 * raft_fowt.py:1971-1974).
 *
 * A design without wet strips gives zeros.  A strip below the seabed gives a negative base and, as in the reference, NaN
 * -- in that design only.  The bits of D[d,c,:] depend on the design's strips alone: not on the batch, the block cut of
 * a crossing or the entry used.
 *
 * These prototypes are kept out of raftx.h on purpose: that header is the contract both the device library and the CPU
 * oracle implement, and the oracle has no current-load sweep.
 */
#ifndef RAFTX_CURRENT_H
#define RAFTX_CURRENT_H

#include "raftx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* On the design set resident from the last raftx_upload_designs / raftx_build_designs (raft_fowt.py:1976-1983 for every
 * design and current at once).  speed [nCur] m/s, heading_deg [nCur] degrees from global x (raft_member.py:1848),
 * Zref [nDesign] or NULL (= 0), D [nDesign,nCur,6] out.  Errors: no design set; nCur <= 0; a non-finite argument;
 * depth + Zref <= 0. */
int raftx_current_loads(raftx_ctx *ctx, int nCur, const double *speed, const double *heading_deg, const double *Zref,
                        double depth, double shearExp, double *D);

/* On a PREPARED, not yet launched sweep slot (raftx_sweep_prepare / raftx_sweep_prepare_variants), as raftx_sweep_modal:
 * raftx_sweep_launch enqueues the current-load kernel of every block of that crossing behind the block's statistics
 * kernel, where the block's strip tables are still resident; the results land in a page-locked area and
 * raftx_sweep_wait fills D [nDesign,nCur,6] of the crossing (the caller's array must stay alive until the wait; the
 * inputs are copied).  The depth is the crossing's.  An error on an idle or launched slot; raftx_sweep_cancel drops the
 * request and leaves D untouched.
 * Under RAFTX_FUSED_GEN=1 the fused kernel builds its tables itself and leaves none in device memory: a crossing with
 * current loads generates the tables of all its blocks with k_geom_design, as crossings with MacCamy-Fuchs rows do. */
int raftx_sweep_current(raftx_ctx *ctx, int slot, int nCur, const double *speed, const double *heading_deg,
                        const double *Zref, double shearExp, double *D);

#ifdef __cplusplus
}
#endif

#endif /* RAFTX_CURRENT_H */
