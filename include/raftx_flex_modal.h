/* raftx_flex_modal.h -- eigen analysis of units with FLEXIBLE members: n reduced DOFs per system, any n from 6 to
 * RAFTX_FLEX_MODAL_MAX_N (libraftx_hip.so only).
 *
 * Replaces what FOWT.solveEigen and Model.solveEigen do for a unit with nDOF != 6 (raft_fowt.py:1705-1714,
 * raft_model.py:518-527): eig(solve(M_tot, C_tot)), sorted ascending by eigenvalue, with no DOF claim.  The method, the
 * flags, the unit 2-norm modes and their sign convention are those of raftx_modal.h (SMALL_DIAG looks at all n diagonals, the
 * QR step cap is 30 n); an ascending stable order, ties by the QR's column index, takes the place of the DOF claim.
 * At n = 6, 12 .. 36 the results are those of raftx_array_modal_batch put in ascending order, bit for bit.
 * A system's bits do not depend on its place in the batch, on the batch size, on its neighbours or on the grid.
 *
 * Kept out of raftx.h as raftx_modal.h and raftx_array_modal.h are: the CPU oracle has no eigen solver.
 */
#ifndef RAFTX_FLEX_MODAL_H
#define RAFTX_FLEX_MODAL_H

#include "raftx_modal.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RAFTX_FLEX_MODAL_MAX_N 256

/* M, C [nSys,n,n] row-major, already summed; 6 <= n <= RAFTX_FLEX_MODAL_MAX_N.
 * fn [nSys,n] (Hz), ascending.  modes [nSys,n,nModes]: the modes of the nModes lowest frequencies as columns,
 * 0 <= nModes <= n; modes may be NULL only when nModes == 0.  Neither the bits of fn nor those of a returned column depend
 * on nModes.  flags [nSys]: RAFTX_MODAL_*; SMALL_DIAG alone leaves finite results, any other bit makes that system's fn and
 * modes NaN, and only its own.
 * The environment variable RAFTX_FLEX_MODAL_GRID, read per call, overrides the number of workgroups (each walks the systems
 * with a grid stride); the results do not depend on it.
 * Errors, before any launch: n or nModes out of range, a negative nSys, a NULL array.  nSys == 0 succeeds. */
int raftx_flex_modal_batch(raftx_ctx *ctx, int nSys, int n, int nModes, const double *M, const double *C, double *fn,
                           double *modes, int32_t *flags);

#ifdef __cplusplus
}
#endif

#endif /* RAFTX_FLEX_MODAL_H */
