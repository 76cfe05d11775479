/* raftx_channels.h -- linear output channels of a sweep crossing (libraftx_hip.so only).
 *
 * A crossing keeps no responses resident, so raftx_channel_stats_poly cannot be asked afterwards; this entry makes the
 * crossing itself return the standard deviations of the channels an optimisation steers on, 8 B per (design, sea state,
 * channel) instead of the responses.  It serves, per (design, sea state), what FOWT.saveTurbineOutputs reports as a
 * standard deviation for a rigid unit beside the six motions:
 *     raft_fowt.py:2422-2444   nacelle accelerations AxRNA / AyRNA / AzRNA     rows T[:3,:] of the hub node on (i w)^2
 *     raft_fowt.py:2500-2537   tower-base fore-aft bending moment Mbase        weight, inertial reaction, aero through Gw
 *     raft_fowt.py:2356-2373   quasi-static mooring tensions Tmoor             rows of the tension Jacobian
 * and so what omdao_raft.py:870-876 aggregates (stats_AxRNA_max, stats_Mbase_max, stats_pitch_max = mean + 3 sigma).
 *
 * Channel definition, as raftx_channel_stats_poly (raftx.h):
 *     y_c(ih,w) = sum_j (L[.,c,0,j] + i w L[.,c,1,j] - w^2 L[.,c,2,j] + Gw[.,c,j,w]) Xi[d,case,ih,j,w]
 *     chan_std[d,case,c] = sqrt(0.5 sum_{ih,w} |y_c|^2)
 * Standard deviations only: the spectra (nw doubles per channel and pair) are not returned by a crossing; a caller who
 * needs them solves resident and calls raftx_channel_stats_poly.
 *
 * The bits of chan_std[d,case,:] depend on that pair's responses, its rows and (nw, nHead, nChan) alone: not on the block
 * cut of the crossing, the slot, the other designs of the batch or the other requests that ride along.  A pair whose
 * responses are not finite (flag 2) gives non-finite values in its own entries only.
 *
 * The prototype is kept out of raftx.h on purpose: that header is the contract both the device library and the CPU oracle
 * implement, and the oracle has no streamed crossing with channels.
 */
#ifndef RAFTX_CHANNELS_H
#define RAFTX_CHANNELS_H

#include "raftx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RAFTX_SWEEP_CHAN_MAX 64

/* On a PREPARED, not yet launched sweep slot (raftx_sweep_prepare / raftx_sweep_prepare_variants), as raftx_sweep_modal and
 * raftx_sweep_current: raftx_sweep_launch enqueues the channel kernel of every block of that crossing behind the block's
 * statistics kernel; the results land in a page-locked area and raftx_sweep_wait fills chan_std [nDesign,nCase,nChan].
 * L [nL,nChan,3,6] with nL = 1 (rows shared by all designs) or nDesign; Gw [nG,nChan,6,nw] with nG = 0 (NULL), 1 or
 * nDesign.  L, Gw and chan_std must stay alive until the batch has been waited for or cancelled.
 * Errors: an idle or a launched slot; nChan outside 1 .. RAFTX_SWEEP_CHAN_MAX; nL not 1 or nDesign; nG not 0, 1 or
 * nDesign; nG > 0 without Gw; L or chan_std NULL.  A second request on a slot replaces the first; raftx_sweep_cancel and
 * a new raftx_sweep_prepare drop the request and leave chan_std untouched. */
int raftx_sweep_channels(raftx_ctx *ctx, int slot, int nChan, int nL, const double *L, int nG, const raftx_c128 *Gw,
                         double *chan_std);

#ifdef __cplusplus
}
#endif

#endif /* RAFTX_CHANNELS_H */
