// raftx_channels.h -- standard deviations of linear output channels of a sweep crossing's responses (included by
// raftx_hip.hip; entry point in include/raftx_channels.h).
//
// Per (design d, sea state) pair p of a block and channel c, the definition of raftx_channel_stats_poly:
//   coef[c,j,w] = L[d,c,0,j] + i w L[d,c,1,j] - w^2 L[d,c,2,j] (+ Gw[d,c,j,w])
//   y_c(ih,w)   = sum_j coef[c,j,w] Xi[p,ih,j,w]
//   sd[p,c]     = sqrt(0.5 sum_{ih,w} |y_c|^2)
// with the arithmetic of k_channel_stats_poly per term (the same forward-error bound holds, tests/stats_reference.py).
//
// Work decomposition: one workgroup per pair, 64 / 128 / 256 threads chosen by nw as for k_motion_stats, the lanes over
// the bins (the contiguous axis).  The channels are taken in tiles of CH_TILE: per bin and heading a lane loads the six
// complex responses once (16 B per lane, coalesced) and keeps them in registers while it loops over the channels of the
// tile, one accumulator per channel -- the pair's responses are read once per tile, where k_channel_stats_poly reads
// them once per channel.  The 18 row coefficients of a channel are uniform over the workgroup and reach the lanes as
// scalar loads; Gw is per lane, coalesced along the bins.  A lane's sums are folded by a fixed xor butterfly per wave,
// the waves' sums through one LDS slot per (wave, channel) added in wave order: no atomics, and the bits of sd[p,:]
// depend on the pair's responses, its rows and (nw, nHead, nChan) alone.
#pragma once

#define CH_TILE 8

struct ChannelArgs {
    int nCase, nHead, nw, nChan;
    size_t strideL, strideG;             // elements from one design's rows to the next (0: shared rows)
};

// w [nw]; Xi [npair,nHead,6,nw] responses of the block; L rows of the block's first design [.,nChan,3,6]; Gw [.,nChan,6,nw]
// (HAS_G) or null; sd [npair,nChan].  The pointers are kernel arguments of their own: as members of A they would not be
// known not to alias sd, and the rows would come through vector loads.
// HAS_G: the rows carry a Gw term (a template argument: the form without it holds no Gw addresses in registers; the form
// with it keeps the tile's 48 Gw loads of a bin in flight at once -- many registers, two waves per SIMD)
template <bool HAS_G>
__global__ void __launch_bounds__(256) k_sweep_channels(ChannelArgs A, const double *__restrict__ w, const cplx *__restrict__ Xi,
                                                        const double *__restrict__ L, const cplx *__restrict__ Gw,
                                                        double *__restrict__ sd) {
    __shared__ double part[4][CH_TILE];
    const size_t p = blockIdx.x, d = p / A.nCase;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = A.nw;
    const double *Ld = L + d * A.strideL;
    const cplx *Gd = HAS_G ? Gw + d * A.strideG : nullptr;
    const cplx *Xp = Xi + p * A.nHead * 6 * nw;
    for (int c0 = 0; c0 < A.nChan; c0 += CH_TILE) {           // workgroup-uniform
        const int nc = min(CH_TILE, A.nChan - c0);
        double acc[CH_TILE];
#pragma unroll
        for (int t = 0; t < CH_TILE; t++) acc[t] = 0.0;
        for (int i = threadIdx.x; i < nw; i += blockDim.x) {
            const double wi = w[i], w2 = wi * wi;
            for (int ih = 0; ih < A.nHead; ih++) {
                const cplx *x = Xp + ((size_t)ih * 6) * nw + i;
                double2 xj[6];
#pragma unroll
                for (int j = 0; j < 6; j++) xj[j] = *reinterpret_cast<const double2 *>(x + (size_t)j * nw);
#pragma unroll
                for (int t = 0; t < CH_TILE; t++) {
                    if (t >= nc) break;                       // a ragged last tile (uniform)
                    const double *row = Ld + (size_t)(c0 + t) * 18;
                    const cplx *g = HAS_G ? Gd + ((size_t)(c0 + t) * 6) * nw + i : nullptr;
                    double yr = 0.0, yi = 0.0;
#pragma unroll
                    for (int j = 0; j < 6; j++) {
                        double cr = row[j] - w2 * row[12 + j], ci = wi * row[6 + j];     // L0 + (i w) L1 + (i w)^2 L2
                        if (HAS_G) {
                            const double2 gj = *reinterpret_cast<const double2 *>(g + (size_t)j * nw);
                            cr += gj.x;
                            ci += gj.y;
                        }
                        yr += cr * xj[j].x - ci * xj[j].y;
                        yi += cr * xj[j].y + ci * xj[j].x;
                    }
                    acc[t] += yr * yr + yi * yi;
                }
            }
        }
#pragma unroll
        for (int t = 0; t < CH_TILE; t++) {
            double a = acc[t];
            for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
            if (lane == 0) part[wv][t] = a;
        }
        __syncthreads();
        if ((int)threadIdx.x < nc) {
            double a = 0.0;
            for (int q = 0; q < (int)(blockDim.x >> 6); q++) a += part[q][threadIdx.x];
            sd[p * A.nChan + c0 + threadIdx.x] = sqrt(0.5 * a);
        }
        __syncthreads();                                      // the slots are reused by the next tile
    }
}
