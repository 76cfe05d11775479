/* raftx_launch.h -- diagnostics of the fused fixed point's launch form (libraftx_hip.so only).
 *
 * raftx_last_solve_kernel (raftx.h) says which specialisation the last solve launched; this entry says in which form it
 * went out: as the persistent form, whose workgroups claim pair after pair of the batch, or as one workgroup per pair --
 * and with what grid.  Tests that shrink the persistent grid (RAFTX_KP_GRID) or switch the form off (RAFTX_PERSIST=0)
 * prove with it that the setting was honoured.
 *
 * The prototype is kept out of raftx.h on purpose: that header is the contract both the device library and the CPU oracle
 * implement, and the oracle has no launches.
 */
#ifndef RAFTX_LAUNCH_H
#define RAFTX_LAUNCH_H

#include "raftx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The last fused launch on this ctx (the last block of a sweep crossing included): persistent 1 when it went out as the
 * persistent form, 0 for one workgroup per pair, for launches per LDS class and for launches in slabs; grid: the workgroups
 * of that one grid (0 where there were several); pairs: the pairs of the batch.  Returns -1 before the first solve. */
int raftx_last_solve_launch(raftx_ctx *ctx, int *persistent, int *grid, int *pairs);

#ifdef __cplusplus
}
#endif

#endif /* RAFTX_LAUNCH_H */
