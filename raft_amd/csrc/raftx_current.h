// raftx_current.h -- mean drag of a sheared current on the wet strips of every design (included by raftx_hip.hip;
// entry points in include/raftx_current.h).
//
// Per design d, current c and strip (raft_member.py:1843-1896, summed as raft_fowt.py:1976-1983 does):
//   z < 0                           only a wet strip contributes (:1843; the tables hold wet strips only)
//   prof = ((depth - |z|) / (depth + Zref[d]))^shearExp               the library pow: 0 at the seabed, NaN below it (:1846)
//   vcur = speed[c] prof (cos, sin, 0)(heading[c])                    cos / sin come from the host (:1848)
//   vq = (vcur.q) q, vp = vcur - vq, vp1 = (vcur.p1) p1, vp2 = (vcur.p2) p2                       (:1859-1862)
//   n1 = n2 = |vp| (circular) or |vp1|, |vp2| (rectangular)                                        (:1874-1879)
//   D = cq |vq| vq + cp1 n1 vp1 + cp2 n2 vp2 + cEnd |vq| vq          c* = DS_DQ.. / sqrt(8/pi) = rho/2 a Cd (:1872-1894)
//   D_hydro[d,c,0:3] += D, D_hydro[d,c,3:6] += arm x D               the arm about the reduced-DOF point (:1896, T.T of
//                                                                    raft_fowt.py:1983 folded into DS_A)
//
// Work decomposition: one wave per (design, tile of CUR_TILE currents), CUR_WAVES waves per workgroup; the lanes stride
// over the design's strips, each lane reads a strip's record and evaluates its pow once and then loops over the currents
// of the tile with the six sums of every current in registers.  A crossing's usual one to four currents are one tile: one
// wave per design.  The sums of the 64 lanes are folded by a fixed xor butterfly: no atomics, no LDS, and the bits of
// D_hydro[d,c,:] depend on the design's strips alone -- not on the grid, the tile, the block cut or the launch form.
#pragma once

#define CUR_TILE 4
#define CUR_WAVES 4
#define CUR_SQRT_8_OVER_PI 1.5957691216057308      // sqrt(8/pi), as numpy rounds it (raft_amd/strips.py c_drag)

struct CurrentArgs {
    int nDesign, nCur;
    const int64_t *__restrict__ off;     // [nDesign+1]
    const double *__restrict__ ds;       // device strip records
    const int *__restrict__ dsi;
    const double *__restrict__ par;      // [3,nCur]: speed | cos(heading) | sin(heading)
    const double *__restrict__ Zref;     // [nDesign] or null (0)
    double depth, shearExp;
    double *__restrict__ D;              // [nDesign,nCur,6]
};

__global__ void __launch_bounds__(64 * CUR_WAVES) k_current_loads(CurrentArgs A) {
    const int lane = threadIdx.x & 63;
    const int nTile = (A.nCur + CUR_TILE - 1) / CUR_TILE;
    const long long wv = (long long)blockIdx.x * CUR_WAVES + (threadIdx.x >> 6);
    if (wv >= (long long)A.nDesign * nTile) return;              // wave-uniform
    const int d = (int)(wv / nTile), c0 = (int)(wv % nTile) * CUR_TILE;
    const double hz = A.depth + (A.Zref ? A.Zref[d] : 0.0);
    double sp[CUR_TILE], ch[CUR_TILE], sh[CUR_TILE], acc[CUR_TILE][6];
#pragma unroll
    for (int t = 0; t < CUR_TILE; t++) {
        const int c = min(c0 + t, A.nCur - 1);                   // a tile's tail repeats the last current (never stored)
        sp[t] = A.par[c];
        ch[t] = A.par[A.nCur + c];
        sh[t] = A.par[2 * A.nCur + c];
#pragma unroll
        for (int j = 0; j < 6; j++) acc[t][j] = 0.0;
    }
    const int64_t s0 = A.off[d], s1 = A.off[d + 1];
    for (int64_t s = s0 + lane; s < s1; s += 64) {
        const double *rec = A.ds + (size_t)s * DS_N;
        const double z = rec[DS_X + 2];
        if (!(z < 0.0)) continue;
        const bool circ = (A.dsi[s] & DSI_CIRC) != 0;
        const double ax = rec[DS_A], ay = rec[DS_A + 1], az = rec[DS_A + 2];
        const double q[3] = {rec[DS_Q], rec[DS_Q + 1], rec[DS_Q + 2]};
        const double p1[3] = {rec[DS_P1], rec[DS_P1 + 1], rec[DS_P1 + 2]};
        const double p2[3] = {rec[DS_P2], rec[DS_P2 + 1], rec[DS_P2 + 2]};
        const double cq = rec[DS_DQ] / CUR_SQRT_8_OVER_PI, cp1 = rec[DS_DQ + 1] / CUR_SQRT_8_OVER_PI,
                     cp2 = rec[DS_DQ + 2] / CUR_SQRT_8_OVER_PI, cEnd = rec[DS_DQ + 3] / CUR_SQRT_8_OVER_PI;
        const double prof = pow((A.depth - fabs(z)) / hz, A.shearExp);
#pragma unroll
        for (int t = 0; t < CUR_TILE; t++) {
            const double v = sp[t] * prof;
            const double vc[3] = {v * ch[t], v * sh[t], 0.0};
            const double dq = vc[0] * q[0] + vc[1] * q[1], d1 = vc[0] * p1[0] + vc[1] * p1[1], d2 = vc[0] * p2[0] + vc[1] * p2[1];
            double vq[3], vp[3], v1[3], v2[3];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                vq[j] = dq * q[j];
                vp[j] = vc[j] - vq[j];
                v1[j] = d1 * p1[j];
                v2[j] = d2 * p2[j];
            }
            const double nq = sqrt(vq[0] * vq[0] + vq[1] * vq[1] + vq[2] * vq[2]);
            const double np = sqrt(vp[0] * vp[0] + vp[1] * vp[1] + vp[2] * vp[2]);
            const double n1 = circ ? np : sqrt(v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2]);
            const double n2 = circ ? np : sqrt(v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2]);
            double D[3];
#pragma unroll
            for (int j = 0; j < 3; j++) D[j] = ((cq * nq * vq[j] + cp1 * n1 * v1[j]) + cp2 * n2 * v2[j]) + cEnd * nq * vq[j];   // :1894
            acc[t][0] += D[0];
            acc[t][1] += D[1];
            acc[t][2] += D[2];
            acc[t][3] += ay * D[2] - az * D[1];
            acc[t][4] += az * D[0] - ax * D[2];
            acc[t][5] += ax * D[1] - ay * D[0];
        }
    }
#pragma unroll
    for (int t = 0; t < CUR_TILE; t++)
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double a = acc[t][j];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) a += __shfl_xor(a, m, 64);
            acc[t][j] = a;
        }
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < CUR_TILE; t++)
            if (c0 + t < A.nCur) {
                double *o = A.D + ((size_t)d * A.nCur + (c0 + t)) * 6;
#pragma unroll
                for (int j = 0; j < 6; j++) o[j] = acc[t][j];
            }
    }
}

// grid of a launch over nDesign designs and nCur currents (0 designs: no launch)
static inline unsigned current_grid(int nDesign, int nCur) {
    const long long waves = (long long)nDesign * ((nCur + CUR_TILE - 1) / CUR_TILE);
    return (unsigned)((waves + CUR_WAVES - 1) / CUR_WAVES);
}
