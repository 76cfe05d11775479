/* raftx_array_modal.h -- eigen analysis of moored ARRAYS of rigid 6-DOF units over all n = 6 nUnit DOFs (libraftx_hip.so only).
 *
 * Replaces what Model.solveEigen does for a farm (raft_model.py:436-547): the block-diagonal unit matrices plus the array
 * mooring system's coupled stiffness (ms.getCoupledStiffnessA(lines_only=True)) over all 6 nFOWT DOFs, numpy.linalg.solve and
 * numpy.linalg.eig, and the DOF claim over rows n-1 .. 0.  The method, the flags, the unit 2-norm modes and their sign
 * convention are those of raftx_modal.h; SMALL_DIAG looks at all n diagonals and the QR step cap is 30 n.  With nUnit == 1 the
 * results are those of raftx_modal_batch, bit for bit.  A system's bits do not depend on its place in the batch, on the batch
 * size or on the other systems.  Flexible units (nDOF != 6) are not covered
 * here: a single unit with flexible members is raftx_flex_modal.h.
 *
 * Kept out of raftx.h as raftx_modal.h and raftx_array_mooring.h are: the CPU oracle has no eigen solver.
 */
#ifndef RAFTX_ARRAY_MODAL_H
#define RAFTX_ARRAY_MODAL_H

#include "raftx_modal.h"
#include "raftx_array_mooring.h"

#ifdef __cplusplus
extern "C" {
#endif

/* n = 6 nUnit, nUnit in 1 .. RAFTX_ARRAY_MAX_UNIT.  M, C [nArray,n,n] row-major (unit-major DOFs, the layout of Cc of
 * raftx_solve_system); fn [nArray,n] (Hz), modes [nArray,n,n] (column j = mode of fn[j]), flags [nArray]: RAFTX_MODAL_*.
 * Errors, before any launch: nUnit out of range, a negative nArray, a NULL array. */
int raftx_array_modal_batch(raftx_ctx *ctx, int nArray, int nUnit, const double *M, const double *C, double *fn,
                            double *modes, int32_t *flags);

/* The same on the moored array, with no host round trip in between:
 *   C_tot = blockdiag(K_unit) + C_moor(lines, pose)   the array stiffness of raftx_array_mooring_lines, bit for bit
 *   M_tot = blockdiag(M_unit)
 * M_unit, K_unit [nArray,nUnit,6,6]; dC [nArray,n,n] or NULL is added last.  lines, pose and depth as in
 * raftx_array_mooring_lines, with its errors.  C_out [nArray,n,n] or NULL receives C_tot.
 * moor_flags [nArray]: the RAFTX_MOOR_* bits.  An array with any of them set is NaN and carries flags = 0.
 * The pose is taken, not solved for: run raftx_array_mean_pose first when it is not known.
 * Errors, before any launch: those of raftx_array_mooring_lines; NULL M_unit, K_unit, fn, modes, flags or moor_flags. */
int raftx_array_modal_moored(raftx_ctx *ctx, int nArray, int nUnit, int nLine, const double *lines, const double *pose,
                             double depth, const double *M_unit, const double *K_unit, const double *dC, double *fn,
                             double *modes, double *C_out, int32_t *flags, int32_t *moor_flags);

#ifdef __cplusplus
}
#endif

#endif /* RAFTX_ARRAY_MODAL_H */
