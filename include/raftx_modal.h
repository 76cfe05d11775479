/* raftx_modal.h -- batched eigen analysis of rigid 6-DOF systems (libraftx_hip.so only).
 *
 * Replaces, per system, what raft_fowt.py:1627-1729 (FOWT.getStiffness + FOWT.solveEigen) and
 * raft_model.py:436-547 (Model.solveEigen, one unit, no array mooring system) compute:
 *     A = solve(M_tot, C_tot)            LU with partial pivoting (numpy.linalg.solve)
 *     eigenvalues / vectors of A         power-of-two balancing, Householder Hessenberg reduction,
 *                                        Francis double-shift QR with eigenvector back-substitution
 *                                        (the dgeev / EISPACK hqr2 class), balancing undone
 *     fn = sqrt(lambda)/2/pi [Hz] and the mode columns in the reference's DOF order (rows 5 .. 0, each
 *     claims the unclaimed column of largest |v|, first index on ties; the list reversed).
 *
 * Modes have unit 2-norm, as LAPACK returns them.  Their sign is fixed so that the component of largest
 * magnitude (first on ties) is positive: LAPACK's sign is arbitrary, the device's is deterministic.  This is
 * the only intended difference from the reference's `modes`.
 *
 * The reference raises or returns complex values where these entries set flags (int32 per system).  Under
 * every flag except RAFTX_MODAL_SMALL_DIAG the system's fn and modes are NaN.
 *
 * These prototypes are kept out of raftx.h on purpose: that header is the contract both the device library
 * and the CPU oracle implement, and the oracle has no eigen solver.
 */
#ifndef RAFTX_MODAL_H
#define RAFTX_MODAL_H

#include "raftx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RAFTX_MODAL_SMALL_DIAG     1   /* a diagonal of M_tot or C_tot below 1 (raft_fowt.py:1667-1675 raises) */
#define RAFTX_MODAL_NONPOSITIVE    2   /* an eigenvalue <= 0 (raft_fowt.py:1682-1683 raises) */
#define RAFTX_MODAL_COMPLEX        4   /* a complex-conjugate eigenvalue pair */
#define RAFTX_MODAL_SINGULAR_M     8   /* an exactly zero pivot in the LU of M_tot (numpy raises LinAlgError) */
#define RAFTX_MODAL_NO_CONVERGENCE 16  /* the QR iteration did not converge in 30*6 steps */

/* Stateless: n systems, M / C [n,6,6] row-major in, fn [n,6] (Hz), modes [n,6,6] (column j = mode of fn[j]),
 * flags [n] out. */
int raftx_modal_batch(raftx_ctx *ctx, int n, const double *M, const double *C, double *fn, double *modes,
                      int32_t *flags);

/* On the design set resident from the last raftx_upload_designs / raftx_build_designs: M0 + dM, C0 + dC after
 * the statics add-up.  dM / dC: [nDesign,6,6] or NULL (the terms the eigen problem has and the dynamics' M0 / C0
 * may not: A_BEM[:,:,0], yawstiff).  props: [nDesign,RAFTX_SP_N] or NULL, the record of raftx_fetch_statics
 * (raftx_build_designs only). */
int raftx_modal_resident(raftx_ctx *ctx, const double *dM, const double *dC, double *fn, double *modes,
                         int32_t *flags, double *props);

/* On a PREPARED, not yet launched sweep slot (raftx_sweep_prepare / raftx_sweep_prepare_variants): the modal
 * kernel of every block of that crossing is enqueued by raftx_sweep_launch behind whatever writes the summed
 * M0 / C0 of the block, and raftx_sweep_wait fills the outputs ([nDesign,...] of the crossing; dM / dC / props as
 * above; the caller's arrays must stay alive until the wait).  An error on an idle or launched slot. */
int raftx_sweep_modal(raftx_ctx *ctx, int slot, const double *dM, const double *dC, double *fn, double *modes,
                      int32_t *flags, double *props);

#ifdef __cplusplus
}
#endif

#endif /* RAFTX_MODAL_H */
