// raftx_hip.hip -- MI355X (gfx950 / CDNA4) implementation of include/raftx.h.
//
// Hot path of WISDEM/RAFT: Morison strip sweep + stochastic drag linearisation
// fixed point + per-frequency 6x6 complex solve (raft/raft_model.py:994-1236,
// raft/raft_fowt.py:1732-1957, raft/raft_member.py:1899-2152), written
// directly for CDNA4: fp64 VALU, wave64, one workgroup per (design, sea state),
// NB frequency bins per lane.
//
// Mapping:
//   * frequency is the contiguous axis of every reference array, so lane <-> w
//     makes every global load/store of a [6,nw] / [6,6,nw] slab coalesced;
//   * strip records (256 B each) are wave-uniform: the kernels read them with
//     scalar loads (constant cache -> SGPRs) and use them as the scalar operand
//     of v_fma_f64, amortised over the NB bins a lane owns;
//   * the only cross-frequency couplings -- the per-strip vRMS sums
//     (raft_member.py:2084-2090, helpers.py:684) and the convergence test
//     (raft_model.py:1104) -- go through per-wave LDS transposition tiles
//     inside one workgroup; nothing crosses workgroups or devices;
//   * the 6x6 complex impedance is factorised per lane in registers with
//     LAPACK-style partial pivoting (pivot on |re|+|im|, as izamax).
//
// No fallback paths: every entry point either runs on the GPU or fails.

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>        // types only: the library is dlopen'ed on the first raftx_comm_* call
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <map>
#include <functional>
#include <limits>
#include <mutex>
#include <type_traits>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/raftx.h"
#include "../../include/raftx_modal.h"
#include "../../include/raftx_current.h"
#include "../../include/raftx_channels.h"
#include "../../include/raftx_qtfgen.h"
#include "../../include/raftx_mooring.h"
#include "../../include/raftx_statics.h"
#include "../../include/raftx_array_mooring.h"
#include "../../include/raftx_array_modal.h"
#include "../../include/raftx_flex_modal.h"
#include "../../include/raftx_launch.h"

// roctx ranges around the phases of the host side: named spans for `rocprofv3 --marker-trace`.
// librocprofiler-sdk-roctx is bound at run time on first use; without it (or outside a profiler) the ranges cost a branch.
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        if (getenv("RAFTX_NO_ROCTX")) return;
        for (const char *n : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
            if (void *h = dlopen(n, RTLD_NOW | RTLD_LOCAL)) {
                push = reinterpret_cast<int (*)(const char *)>(dlsym(h, "roctxRangePushA"));
                pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
                if (push && pop) return;
                push = nullptr;
                pop = nullptr;
            }
        }
    }
};
static Roctx &roctx() {
    static Roctx r;
    return r;
}
struct RangeScope {
    bool on;
    explicit RangeScope(const char *name) : on(roctx().push != nullptr) {
        if (on) roctx().push(name);
    }
    ~RangeScope() {
        if (on) roctx().pop();
    }
};

#include "raftx_kernels.h"
#include "raftx_qtf.h"
#include "raftx_geom.h"
#include "raftx_fusedgen.h"
#include "raftx_dense.h"
#include "raftx_flex.h"
#include "raftx_modal.h"
#include "raftx_current.h"
#include "raftx_channels.h"
#include "raftx_qtfgen.h"
#include "raftx_mooring.h"
#include "raftx_statics.h"
#include "raftx_array_mooring.h"
#include "raftx_array_modal.h"
#include "raftx_flex_modal.h"

// Coupled array solve (raft_model.py:1164-1236): Xi = Z_sys^-1 F for every (system, bin).  One wavefront per
// (system, bin), NBIN (1, 2 or 4: what fits LDS) consecutive bins per workgroup so that the loads of one matrix entry
// for the bins of a workgroup are one contiguous segment of the [.., nw] slabs.  The augmented matrix [Z_sys | F] of a
// wave lives in LDS; Gaussian elimination with partial pivoting (pivot on |re| + |im|, first largest, as izamax):
// pivot search as a wave reduction, multipliers with a lane per row, the rank-1 update with the lanes over the
// (row, column) entries, back substitution column by column with a lane per (row, right-hand side).  A wave's LDS
// traffic needs no s_barrier (wave_lds_fence).
template <bool RESIDENT>
__global__ void __launch_bounds__(256) k_solve_system(int nSys, int nUnit, int nRhs, int nw, int nCase,
                                                      const double *__restrict__ w, const cplx *__restrict__ Zblk,
                                                      const double *__restrict__ Mc, const double *__restrict__ Bc,
                                                      const double *__restrict__ Cc, const cplx *__restrict__ F,
                                                      cplx *__restrict__ Xi) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int n = 6 * nUnit, ld = n + nRhs, nel = n * ld;
    const int nbin = blockDim.x >> 6, ngrp = (nw + nbin - 1) / nbin;
    const int s = blockIdx.x / ngrp, iw0 = (blockIdx.x % ngrp) * nbin;
    cplx *Aall = reinterpret_cast<cplx *>(smem);           // [nbin][n][ld]
    // host layout: Zblk [nSys,nUnit,36,nw], F [nSys,nRhs,n,nw], coupling per system.
    // resident layout (results of k_solve_dynamics): unit u of system (g, c) is pair (g*nUnit+u)*nCase + c;
    // Z [pair,36,nw], F_wave [pair,nRhs,6,nw], coupling per group g.
    const int g = RESIDENT ? s / nCase : s, ic = RESIDENT ? s % nCase : 0;
    for (int t = threadIdx.x; t < nel * nbin; t += blockDim.x) {
        const int e = t / nbin, b = t % nbin;
        const int iw = min(iw0 + b, nw - 1);
        const double ww = w[iw];
        const int r = e / ld, c = e % ld;
        cplx v = {0.0, 0.0};
        if (c < n) {
            if (r / 6 == c / 6) {
                const size_t pair = RESIDENT ? ((size_t)g * nUnit + r / 6) * nCase + ic : (size_t)s * nUnit + r / 6;
                v = Zblk[((pair * 6 + r % 6) * 6 + c % 6) * nw + iw];
            }
            size_t o = (size_t)g * n * n + (size_t)r * n + c;
            double m = Mc ? Mc[o] : 0.0, bb = Bc ? Bc[o] : 0.0, kk = Cc ? Cc[o] : 0.0;
            if (Mc || Bc || Cc) {
                v.re += -(ww * ww) * m + kk;
                v.im += ww * bb;
            }
        } else if (RESIDENT) {
            const size_t pair = ((size_t)g * nUnit + r / 6) * nCase + ic;
            v = F[((pair * nRhs + (c - n)) * 6 + r % 6) * nw + iw];
        } else {
            v = F[(((size_t)s * nRhs + (c - n)) * n + r) * nw + iw];
        }
        Aall[(size_t)b * nel + e] = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    cplx *A = Aall + (size_t)wv * nel;
    for (int k = 0; k < n; k++) {
        // pivot row: first row of the largest |re| + |im| in column k
        double best = -1.0;
        int p = n;
        for (int r = k + lane; r < n; r += 64) {
            const double v = fabs(A[r * ld + k].re) + fabs(A[r * ld + k].im);
            if (v > best) {
                best = v;
                p = r;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) argmax_step(best, p, off);
        if (p >= n) p = k;                                    // a column of NaNs: no row compares larger
        if (p != k)
            for (int c = lane; c < ld; c += 64) {
                const cplx t = A[k * ld + c];
                A[k * ld + c] = A[p * ld + c];
                A[p * ld + c] = t;
            }
        wave_lds_fence();
        const cplx pv = A[k * ld + k];
        const double dd = pv.re * pv.re + pv.im * pv.im;
        const cplx inv = {pv.re / dd, -pv.im / dd};
        for (int r = k + 1 + lane; r < n; r += 64) A[r * ld + k] = cmul(A[r * ld + k], inv);
        wave_lds_fence();
        // rank-1 update: the lanes as an 8 x 8 grid over (row, column), strided by 8 -- no division in the loop
        for (int r = k + 1 + (lane >> 3); r < n; r += 8) {
            const cplx l = A[r * ld + k];
            for (int c = k + 1 + (lane & 7); c < ld; c += 8) A[r * ld + c] = csub(A[r * ld + c], cmul(l, A[k * ld + c]));
        }
        wave_lds_fence();
    }
    // back substitution, column by column: x_k = b_k / u_kk, then b_r -= u_rk x_k for the rows above
    for (int k = n - 1; k >= 0; k--) {
        const cplx pv = A[k * ld + k];
        const double dd = pv.re * pv.re + pv.im * pv.im;
        for (int j = lane; j < nRhs; j += 64) {
            const cplx sum = A[k * ld + n + j];
            A[k * ld + n + j] = cplx{(sum.re * pv.re + sum.im * pv.im) / dd, (sum.im * pv.re - sum.re * pv.im) / dd};
        }
        wave_lds_fence();
        if (nRhs == 1) {
            const cplx xk = A[k * ld + n];
            for (int r = lane; r < k; r += 64) A[r * ld + n] = csub(A[r * ld + n], cmul(A[r * ld + k], xk));
        } else {
            for (int e = lane; e < k * nRhs; e += 64) {
                const int r = e / nRhs, j = e % nRhs;
                A[r * ld + n + j] = csub(A[r * ld + n + j], cmul(A[r * ld + k], A[k * ld + n + j]));
            }
        }
        wave_lds_fence();
    }
    __syncthreads();
    // responses out: the bins of the workgroup side by side
    for (int t = threadIdx.x; t < n * nRhs * nbin; t += blockDim.x) {
        const int e = t / nbin, b = t % nbin;
        const int k = e % n, j = e / n;
        if (iw0 + b < nw) Xi[(((size_t)s * nRhs + j) * n + k) * nw + iw0 + b] = Aall[(size_t)b * nel + k * ld + n + j];
    }
}
// Register-resident variant for arrays of 2 .. 5 units (n = 12 .. 30 rows): a LANE PER ROW, two systems per wavefront (lanes
// 0-31 and 32-63), the whole row -- n complex entries plus up to four right-hand sides -- in the lane's registers.  The
// elimination is unrolled over the column k, so every register index is static; partial pivoting is implicit (the pivot
// row stays where it is and is marked done: the same pivot rows, multipliers and updates as zgetrf's interchanges,
// raft_model.py:1191), the pivot search is a two-phase 32-bit DPP argmax within the half-wave, the pivot row reaches the other
// rows through a row buffer in LDS (its owner lane stores it, everyone reads it back as a broadcast).  ~3.7 k VALU
// instructions per PAIR of systems against ~10 k per system of the LDS-resident kernel above (whose update loop spends its
// time on index arithmetic, and whose assembly through LDS is a chain of dependent loads).  What bounds it -- the LDS itself:
// a published pivot-row entry costs 8 LDS-array cycles whatever the store's width or active lanes (ds_write_b128 is eight
// 8-lane groups; 4 x b32 is four times two 32-lane groups) plus 4 to read it back, ~2 100 LDS cycles per system on the ONE
// LDS of a CU = 37 ms per 10^7 systems before anything else; 24 of the 60 ms go with the stores compiled out
// (profiles/r05_lu_store_experiment.json); a software-pipelined publication measured 16 % slower.  Round 6 built the
// variant with TWO LANES PER ROW (half the registers, four waves per SIMD instead of two, both owner lanes storing in one
// instruction): bit-identical and NOT faster (61.0 against 60.2 ms, profiles/r06_experiments/lu_two_lanes_per_row.txt) --
// more waves cannot help a kernel bound by LDS-array cycles per system, and the one-lane form already shares every store
// between its two systems.  Removed again.  What would cut the published volume is a blocked factorisation whose trailing
// update runs on the matrix pipe (v_mfma_f64_16x16x4), at the price of the pivots' bit-identity: DESIGN.md 3.3.
#define SYSROWS_MAXRHS 4
// ASM (resident form only): the units' 6 x 6 impedance blocks are ASSEMBLED here, Z = -w^2 M0 + i w (B0 + B_drag) + C0 with the
// unit kernel's own expression (assemble_and_solve: fma(-w^2, M, C), w * (B0 + Bd) -- the same bits), from 36 x 4 doubles
// per unit instead of 36 x nw complex per pair: the fixed points then need not export Z at all (a farm sweep of 200 000
// pairs writes and re-reads 23 GB of it) and run as the LEAN kernel with the excitation export (KF_OUTF).
template <int NU, int NR, bool RESIDENT, bool ASM = false>          // NR: right-hand sides compiled in (nRhs <= NR; the rest are zero columns)
// amdgpu_waves_per_eu(2, 2): the waves per SIMD the register allocation aims at
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) k_solve_system_rows(int nSys, int nRhs, int nw, int nCase, const double *__restrict__ w,
                                                          const cplx *__restrict__ Zblk, const double *__restrict__ Mc,
                                                          const double *__restrict__ Bc, const double *__restrict__ Cc,
                                                          const cplx *__restrict__ F, cplx *__restrict__ Xi,
                                                          const double *__restrict__ uM = nullptr, const double *__restrict__ uB = nullptr,
                                                          const double *__restrict__ uC = nullptr, const double *__restrict__ uBd = nullptr) {
    constexpr int N = 6 * NU;
    const int ngrp = (nw + 1) / 2;                       // two bins (systems) per wavefront: lanes 0-31 and 32-63
    const int s = blockIdx.x / ngrp, lane = threadIdx.x, half = lane >> 5, r = lane & 31, hbase = lane & 32;
    const int iwr = (blockIdx.x % ngrp) * 2 + half;
    const bool live = iwr < nw;
    const int iw = live ? iwr : nw - 1;
    const bool row = r < N;
    const int rr = row ? r : 0;
    const int g = RESIDENT ? s / nCase : s, ic = RESIDENT ? s % nCase : 0;
    // The lane's row of [Z_sys | F] (raft_model.py:1164-1191), straight into registers: the unit's own 6 x 6 block from the
    // per-unit impedances, the coupling terms from the group's matrices (rows are contiguous), everything else zero.  All
    // loads are independent: one exposed round trip.
    cplx a[N], bR[NR];
    const double ww = w[iw];
    const int u = rr / 6, q = rr % 6;
    const size_t pair = RESIDENT ? ((size_t)g * NU + u) * nCase + ic : (size_t)s * NU + u;
    cplx zb[6];
    if constexpr (ASM) {
        const size_t dsg = ((size_t)g * NU + u) * 36 + q * 6, pr = pair * 36 + q * 6;
        const double w2 = ww * ww;
#pragma unroll
        for (int c = 0; c < 6; c++) {
            const double Bq = uB[dsg + c] + uBd[pr + c];
            zb[c] = {fma(-w2, uM[dsg + c], uC[dsg + c]), ww * Bq};
        }
    } else {
#pragma unroll
        for (int c = 0; c < 6; c++) zb[c] = Zblk[((pair * 6 + q) * 6 + c) * nw + iw];
    }
#pragma unroll
    for (int j = 0; j < NR; j++)
        bR[j] = j < nRhs ? (RESIDENT ? F[((pair * nRhs + j) * 6 + q) * nw + iw] : F[(((size_t)s * nRhs + j) * N + rr) * nw + iw])
                         : cplx{0.0, 0.0};
    const size_t o = (size_t)g * N * N + (size_t)rr * N;
#pragma unroll
    for (int c = 0; c < N; c++) {
        const double m = Mc ? Mc[o + c] : 0.0, bb = Bc ? Bc[o + c] : 0.0, kk = Cc ? Cc[o + c] : 0.0;
        a[c] = {fma(-(ww * ww), m, kk), ww * bb};
    }
#pragma unroll
    for (int c = 0; c < N; c++) {                        // the diagonal block of the lane's unit (u is per lane: selects)
        const int cu = c / 6;
        const cplx z = zb[c % 6];
        a[c].re += cu == u ? z.re : 0.0;
        a[c].im += cu == u ? z.im : 0.0;
    }
    // the pivot row of a step travels through a row buffer in LDS: written by the one lane of each half that owns it, read
    // back by all (same address within a half: a broadcast read)
    __shared__ __attribute__((aligned(16))) double rowbuf_[2 * 2 * (N + NR)];
    cplx *rowbuf = reinterpret_cast<cplx *>(rowbuf_) + half * (N + NR);
    bool todo = row;                                     // this row has not been a pivot row yet
    int mystep = N;                                      // elimination step at which it was
    const unsigned rkey = 31u - (unsigned)r;             // ties go to the lower row (izamax takes the first largest)
#pragma unroll
    for (int k = 0; k < N; k++) {
        // pivot: the row of the largest |re| + |im| in column k among the rows still to do.  Magnitude and row travel as ONE
        // key -- the row index replaces the five lowest mantissa bits (a choice between candidates equal to 7e-15 is
        // arbitrary anyway) -- so that the argmax is a max: four row_shr steps inside the 16-lane rows, one row_bcast
        // across the two rows of a half, all DPP (no LDS round trips).
        double best = todo ? fabs(a[k].re) + fabs(a[k].im) : -1.0;
        if (todo && !(best >= 0.0)) best = 0.0;          // NaN: comparable, so that a pivot is always found
        // The (magnitude, row) key is compared in two 32-bit phases -- `v_max_f64` takes no DPP operand (round 4's form cost
        // seven VALU instructions per reduction step: two copies, two DPP moves, a canonicalising max, the max), while
        // `v_max_u32` with a zero-filling row_shr is ONE: first the high words (+1, so that 0 means "no candidate": rows
        // that are done), then the low words -- five lowest mantissa bits replaced by the row -- of the lanes that tie on
        // the high word.  Lexicographic (hi, lo) on non-negative doubles is the order of the doubles: the same pivots as
        // before, bit for bit.  The two 16-lane rows of a half meet in scalar registers (readlane + s_max).
        const unsigned khi = todo ? (unsigned)__double2hiint(best) + 1u : 0u;
        const unsigned klo = ((unsigned)__double2loint(best) & ~31u) | rkey;
#define ROW_UMAX_(x)                                                                                   \
        x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, true));           \
        x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, true));           \
        x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, true));           \
        x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, true));
        unsigned mh = khi;
        ROW_UMAX_(mh)                                    // row_shr:1,2,4,8 -> lane 15 of each 16-lane row
        const unsigned h0 = max((unsigned)__builtin_amdgcn_readlane((int)mh, 15), (unsigned)__builtin_amdgcn_readlane((int)mh, 31));
        const unsigned h1 = max((unsigned)__builtin_amdgcn_readlane((int)mh, 47), (unsigned)__builtin_amdgcn_readlane((int)mh, 63));
        unsigned ml = (todo && khi == (half ? h1 : h0)) ? klo : 0u;
        ROW_UMAX_(ml)
#undef ROW_UMAX_
        const unsigned l0 = max((unsigned)__builtin_amdgcn_readlane((int)ml, 15), (unsigned)__builtin_amdgcn_readlane((int)ml, 31));
        const unsigned l1 = max((unsigned)__builtin_amdgcn_readlane((int)ml, 47), (unsigned)__builtin_amdgcn_readlane((int)ml, 63));
        const int p = 31 - (int)((half ? l1 : l0) & 31u);
        const bool mine = todo && r == p;
        const bool upd = todo && r != p;
        if (mine) {
#pragma unroll
            for (int c = k; c < N; c++) rowbuf[c] = a[c];
#pragma unroll
            for (int j = 0; j < NR; j++)
                rowbuf[N + j] = bR[j];
        }
        wave_lds_fence();
        const cplx pv = rowbuf[k];
        // 1 / |pivot|^2: v_rcp_f64 + two Newton steps (5 instructions; the IEEE division sequence is ~15).  A zero pivot still
        // ends in NaN.
        const double pp = pv.re * pv.re + pv.im * pv.im;
        double dinv = __builtin_amdgcn_rcp(pp);
        dinv = fma(fma(-pp, dinv, 1.0), dinv, dinv);
        dinv = fma(fma(-pp, dinv, 1.0), dinv, dinv);
        const cplx inv = {pv.re * dinv, -pv.im * dinv};
        // rows that are done (or beyond the system) take a zero multiplier: the update itself stays straight-line code
        const cplx lk = cmul(a[k], inv);
        const cplx l = {upd ? lk.re : 0.0, upd ? lk.im : 0.0};
#pragma unroll
        for (int c = k + 1; c < N; c++) {
            const cplx u = rowbuf[c];
            a[c] = cfnma(a[c], l, u);                     // four FMAs (as a difference of a product: six instructions)
        }
#pragma unroll
        for (int j = 0; j < NR; j++)
        {
            const cplx u = rowbuf[N + j];
            bR[j] = cfnma(bR[j], l, u);
        }
        if (mine) {
            todo = false;
            mystep = k;
            a[k] = inv;                                  // the reciprocal pivot, for the back substitution
        }
        wave_lds_fence();                                // the buffer is rewritten in the next step
    }
    // back substitution in pivot order: x_k from the row that was the pivot of step k, then out of the rows of earlier steps
#pragma unroll
    for (int k = N - 1; k >= 0; k--) {
        if (mystep == k) {
#pragma unroll
            for (int j = 0; j < NR; j++) {
                bR[j] = cmul(bR[j], a[k]);
                rowbuf[N + j] = bR[j];
            }
        }
        wave_lds_fence();
        const cplx f = {mystep < k ? a[k].re : 0.0, mystep < k ? a[k].im : 0.0};
#pragma unroll
        for (int j = 0; j < NR; j++)
        {
            const cplx xk = rowbuf[N + j];
            bR[j] = cfnma(bR[j], f, xk);
        }
        wave_lds_fence();
    }
    // responses out: unknown k sits in the row that was the pivot of step k
    if (row && live && mystep < N) {
#pragma unroll
        for (int j = 0; j < NR; j++)
            if (j < nRhs) Xi[(((size_t)s * nRhs + j) * N + mystep) * nw + iw] = bR[j];
    }
}
static bool solve_system_rows_ok(int nUnit, int nRhs) {
    return nUnit >= 2 && nUnit <= 5 && nRhs >= 1 && nRhs <= SYSROWS_MAXRHS;
}
// launches the register-resident kernel; returns false if this shape has none
template <bool RESIDENT, bool ASM = false>
static bool launch_solve_system_rows(hipStream_t st, int nSys, int nUnit, int nRhs, int nw, int nCase, const double *w, const cplx *Z,
                                     const double *Mc, const double *Bc, const double *Cc, const cplx *F, cplx *X,
                                     const double *uM = nullptr, const double *uB = nullptr, const double *uC = nullptr,
                                     const double *uBd = nullptr) {
    if (!solve_system_rows_ok(nUnit, nRhs)) return false;
    const dim3 grid((unsigned)((size_t)nSys * ((nw + 1) / 2)));
    const int nr = nRhs == 1 ? 1 : (nRhs == 2 ? 2 : 4);
#define ROWS_CASE(NU_, NR_)                                                                                             \
    if (nUnit == NU_ && nr == NR_) {                                                                                    \
        hipLaunchKernelGGL((k_solve_system_rows<NU_, NR_, RESIDENT, ASM>), grid, dim3(64), 0, st, nSys, nRhs, nw, nCase, w, Z, Mc, Bc, Cc, F, X, \
                           uM, uB, uC, uBd);                                                                           \
        return true;                                                                                                    \
    }
    ROWS_CASE(2, 1) ROWS_CASE(2, 2) ROWS_CASE(2, 4) ROWS_CASE(3, 1) ROWS_CASE(3, 2) ROWS_CASE(3, 4)
    ROWS_CASE(4, 1) ROWS_CASE(4, 2) ROWS_CASE(4, 4) ROWS_CASE(5, 1) ROWS_CASE(5, 2) ROWS_CASE(5, 4)
#undef ROWS_CASE
    return false;
}

// The same assembly as a kernel of its own, for the shapes the register-resident solver does not take (more than five
// units / four right-hand sides): Z [pair,36,nw] into a scratch slab, then the LDS-resident solver as before.
__global__ void __launch_bounds__(256) k_assemble_unit_z(int npair, int nCase, int nw, const double *__restrict__ w,
                                                         const double *__restrict__ uM, const double *__restrict__ uB,
                                                         const double *__restrict__ uC, const double *__restrict__ uBd,
                                                         cplx *__restrict__ Z) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)npair * 36 * nw) return;
    const int iw = (int)(t % nw), e = (int)((t / nw) % 36);
    const size_t pair = t / ((size_t)36 * nw), d = pair / nCase;
    const double ww = w[iw], Bq = uB[d * 36 + e] + uBd[pair * 36 + e];
    Z[t] = {fma(-(ww * ww), uM[d * 36 + e], uC[d * 36 + e]), ww * Bq};
}

// bins per workgroup and dynamic LDS of k_solve_system
static int solve_system_shape(int n, int nRhs, size_t *lds) {
    const size_t per = sizeof(cplx) * (size_t)n * (n + nRhs);
    const int nbin = per * 4 <= 64 * 1024 ? 4 : (per * 2 <= 64 * 1024 ? 2 : 1);
    *lds = per * nbin;
    return nbin;
}

// Motion statistics of the resident responses (raft_fowt.py:2310-2357; helpers.py:678-700): one
// workgroup per (design, case), lanes stride the frequency axis (coalesced 16 B/lane reads of the
// Xi slab: a pure HBM stream, 19.2 KB in -> 48 B out per pair at C3).
__global__ void __launch_bounds__(256) k_motion_stats(int npair, int nHead, int nw, double inv_dw,
                                                      const cplx *__restrict__ Xi, double *__restrict__ sd,
                                                      double *__restrict__ psd,
                                                      const int *__restrict__ niter = nullptr, const int *__restrict__ flags = nullptr,
                                                      int *__restrict__ ints_out = nullptr) {
    __shared__ double part[4][6];
    const int p = blockIdx.x;
    if (p >= npair) return;
    const double r2d = 180.0 / 3.14159265358979323846;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < nw; i += blockDim.x) {
#pragma unroll
        for (int j = 0; j < 6; j++) {
            const double scale = j >= 3 ? r2d : 1.0;
            double a2 = 0.0;
            for (int ih = 0; ih < nHead; ih++) {
                const cplx x = Xi[(((size_t)p * nHead + ih) * 6 + j) * nw + i];
                const double xr = x.re * scale, xi = x.im * scale;
                a2 += xr * xr + xi * xi;
            }
            acc[j] += a2;
            if (psd) psd[((size_t)p * 6 + j) * nw + i] = 0.5 * a2 * inv_dw;
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double a = acc[j];
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        if (lane == 0) part[wv][j] = a;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        double a = 0.0;
        for (int q = 0; q < (int)(blockDim.x >> 6); q++) a += part[q][threadIdx.x];
        sd[(size_t)p * 6 + threadIdx.x] = sqrt(0.5 * a);
    }
    if (ints_out && threadIdx.x == 6) {                   // sweep crossings: iteration count and flags of the pair ride along
        ints_out[p] = niter[p];                           // (out[0..n) = niter, out[n..2n) = flags, page-locked host memory)
        ints_out[npair + p] = flags[p];
    }
}

// Statistics of linear output channels y_c = w^p sum_j L[c,j] Xi_j (hub accelerations, tension Jacobian rows ...):
// one workgroup per (design, case); the Xi slab is streamed once per channel (L2-resident after the first).
__global__ void __launch_bounds__(256) k_channel_stats(int nCase, int nHead, int nw, int nChan, double inv_dw,
                                                       const double *__restrict__ w, const cplx *__restrict__ Xi,
                                                       const double *__restrict__ L, const int *__restrict__ pw,
                                                       double *__restrict__ sd, double *__restrict__ psd) {
    __shared__ double part[4];
    const int p = blockIdx.x, d = p / nCase;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int ch = 0; ch < nChan; ch++) {
        const double *row = L + ((size_t)d * nChan + ch) * 6;
        const double l0 = row[0], l1 = row[1], l2 = row[2], l3 = row[3], l4 = row[4], l5 = row[5];
        const int pe = pw[ch];
        double acc = 0.0;
        for (int i = threadIdx.x; i < nw; i += blockDim.x) {
            double ws = 1.0;
            for (int e = 0; e < pe; e++) ws *= w[i];
            double a2 = 0.0;
            for (int ih = 0; ih < nHead; ih++) {
                const cplx *x = Xi + (((size_t)p * nHead + ih) * 6) * nw + i;
                const cplx x0 = x[0], x1 = x[(size_t)nw], x2 = x[(size_t)2 * nw], x3 = x[(size_t)3 * nw], x4 = x[(size_t)4 * nw],
                           x5 = x[(size_t)5 * nw];
                const double yr = ws * (l0 * x0.re + l1 * x1.re + l2 * x2.re + l3 * x3.re + l4 * x4.re + l5 * x5.re);
                const double yi = ws * (l0 * x0.im + l1 * x1.im + l2 * x2.im + l3 * x3.im + l4 * x4.im + l5 * x5.im);
                a2 += yr * yr + yi * yi;
            }
            acc += a2;
            if (psd) psd[((size_t)p * nChan + ch) * nw + i] = 0.5 * a2 * inv_dw;
        }
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        __syncthreads();
        if (lane == 0) part[wv] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            double a = 0.0;
            for (int q = 0; q < (int)(blockDim.x >> 6); q++) a += part[q];
            sd[(size_t)p * nChan + ch] = sqrt(0.5 * a);
        }
    }
}

// BEM excitation with heading interpolation (raft_fowt.py:1796-1849): one workgroup per (pair, heading), lanes over w
__global__ void __launch_bounds__(256) k_bem_excitation(DevTables T, int nHB, const double *__restrict__ heads,
                                                        const cplx *__restrict__ X, const double *__restrict__ hadj,
                                                        const double *__restrict__ xy, const cplx *__restrict__ Fadd,
                                                        cplx *__restrict__ F) {
    const int ih = blockIdx.x % T.nHead, p = blockIdx.x / T.nHead;
    const int d = p / T.nCase, ic = p % T.nCase;
    const double beta = T.beta[(size_t)ic * T.nHead + ih];
    double bdeg = fmod(beta * (180.0 / M_PI) - (hadj ? hadj[d] : 0.0), 360.0);        // Python's % : result in [0, 360)
    if (bdeg < 0.0) bdeg += 360.0;
    int i1 = nHB - 1, i2 = 0;
    double f2;
    if (bdeg <= heads[0]) {
        const double hlast = heads[nHB - 1] - 360.0;
        f2 = (bdeg - hlast) / (heads[0] - hlast);
    } else if (bdeg >= heads[nHB - 1]) {
        const double hfirst = heads[0] + 360.0;
        f2 = (bdeg - heads[nHB - 1]) / (hfirst - heads[nHB - 1]);
    } else {
        f2 = 0.0;
        for (int i = 0; i < nHB - 1; i++)
            if (heads[i + 1] > bdeg) {
                i1 = i;
                i2 = i + 1;
                f2 = (bdeg - heads[i]) / (heads[i + 1] - heads[i]);
                break;
            }
    }
    const double f1 = 1.0 - f2, sb = sin(beta), cb = cos(beta);
    const double xr = xy ? xy[2 * d] : 0.0, yr = xy ? xy[2 * d + 1] : 0.0;
    const cplx *X1 = X + ((size_t)d * nHB + i1) * 6 * T.nw, *X2 = X + ((size_t)d * nHB + i2) * 6 * T.nw;
    const size_t base = ((size_t)p * T.nHead + ih) * 6 * T.nw;
    for (int i = threadIdx.x; i < T.nw; i += blockDim.x) {
        cplx xp[6];
#pragma unroll
        for (int j = 0; j < 6; j++) {
            const cplx a = X1[(size_t)j * T.nw + i], b = X2[(size_t)j * T.nw + i];
            xp[j] = {a.re * f1 + b.re * f2, a.im * f1 + b.im * f2};
        }
        cplx g[6];
        g[0] = {xp[0].re * cb - xp[1].re * sb, xp[0].im * cb - xp[1].im * sb};
        g[1] = {xp[0].re * sb + xp[1].re * cb, xp[0].im * sb + xp[1].im * cb};
        g[2] = xp[2];
        g[3] = {xp[3].re * cb - xp[4].re * sb, xp[3].im * cb - xp[4].im * sb};
        g[4] = {xp[3].re * sb + xp[4].re * cb, xp[3].im * sb + xp[4].im * cb};
        g[5] = xp[5];
        double ps, pc;
        sincos(-(T.k[i] * (xr * cos(beta) + yr * sin(beta))), &ps, &pc);
        const double z = T.zeta[((size_t)ic * T.nHead + ih) * T.nw + i];
#pragma unroll
        for (int j = 0; j < 6; j++) {
            const double gr = g[j].re * z, gi = g[j].im * z;
            cplx o = {gr * pc - gi * ps, gr * ps + gi * pc};
            if (Fadd) {
                const cplx a = Fadd[base + (size_t)j * T.nw + i];
                o.re += a.re;
                o.im += a.im;
            }
            F[base + (size_t)j * T.nw + i] = o;
        }
    }
}

// y_c = sum_p (i w)^p sum_j L[c,p,j] Xi_j + sum_j Gw[c,j,w] Xi_j  (tower-base moment: weight p=0, inertial reaction
// p=2, complex aero reaction through Gw; raft_fowt.py:2500-2537)
__global__ void __launch_bounds__(256) k_channel_stats_poly(int nCase, int nHead, int nw, int nChan, double inv_dw,
                                                            const double *__restrict__ w, const cplx *__restrict__ Xi,
                                                            const double *__restrict__ L, const cplx *__restrict__ Gw,
                                                            double *__restrict__ sd, double *__restrict__ psd) {
    __shared__ double part[4];
    const int p = blockIdx.x, d = p / nCase;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int ch = 0; ch < nChan; ch++) {
        const double *row = L + ((size_t)d * nChan + ch) * 18;
        const cplx *g = Gw ? Gw + ((size_t)d * nChan + ch) * 6 * nw : nullptr;
        double acc = 0.0;
        for (int i = threadIdx.x; i < nw; i += blockDim.x) {
            const double wi = w[i], w2 = wi * wi;
            double a2 = 0.0;
            for (int ih = 0; ih < nHead; ih++) {
                const cplx *x = Xi + (((size_t)p * nHead + ih) * 6) * nw + i;
                double yr = 0.0, yi = 0.0;
#pragma unroll
                for (int j = 0; j < 6; j++) {
                    const cplx xj = x[(size_t)j * nw];
                    double cr = row[j] - w2 * row[12 + j], ci = wi * row[6 + j];     // L0 + (i w) L1 + (i w)^2 L2
                    if (g) {
                        const cplx gj = g[(size_t)j * nw + i];
                        cr += gj.re;
                        ci += gj.im;
                    }
                    yr += cr * xj.re - ci * xj.im;
                    yi += cr * xj.im + ci * xj.re;
                }
                a2 += yr * yr + yi * yi;
            }
            acc += a2;
            if (psd) psd[((size_t)p * nChan + ch) * nw + i] = 0.5 * a2 * inv_dw;
        }
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        __syncthreads();
        if (lane == 0) part[wv] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            double a = 0.0;
            for (int q = 0; q < (int)(blockDim.x >> 6); q++) a += part[q];
            sd[(size_t)p * nChan + ch] = sqrt(0.5 * a);
        }
    }
}

// The same for a response with any number of DOFs handed over by the caller (raftx_response_stats): one workgroup per channel,
// lanes over the bins, the DOF loop inside (coalesced reads of the [.,nw] slabs)
__global__ void __launch_bounds__(256) k_response_stats(int nDof, int nResp, int nw, double inv_dw, const double *__restrict__ w,
                                                        const cplx *__restrict__ Xi, const double *__restrict__ L,
                                                        const cplx *__restrict__ Gw, double *__restrict__ sd, double *__restrict__ psd) {
    __shared__ double part[4];
    const int ch = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const double *row = L + (size_t)ch * 3 * nDof;
    const cplx *g = Gw ? Gw + (size_t)ch * nDof * nw : nullptr;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nw; i += blockDim.x) {
        const double wi = w[i], w2 = wi * wi;
        double a2 = 0.0;
        for (int ih = 0; ih < nResp; ih++) {
            const cplx *x = Xi + ((size_t)ih * nDof) * nw + i;
            double yr = 0.0, yi = 0.0;
            for (int j = 0; j < nDof; j++) {
                const cplx xj = x[(size_t)j * nw];
                double cr = row[j] - w2 * row[2 * nDof + j], ci = wi * row[nDof + j];     // L0 + (i w) L1 + (i w)^2 L2
                if (g) {
                    const cplx gj = g[(size_t)j * nw + i];
                    cr += gj.re;
                    ci += gj.im;
                }
                yr += cr * xj.re - ci * xj.im;
                yi += cr * xj.im + ci * xj.re;
            }
            a2 += yr * yr + yi * yi;
        }
        acc += a2;
        if (psd) psd[(size_t)ch * nw + i] = 0.5 * a2 * inv_dw;
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) part[wv] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0;
        for (int q = 0; q < (int)(blockDim.x >> 6); q++) a += part[q];
        sd[ch] = sqrt(0.5 * a);
    }
}

// ------------------------------------------------------------------ host side
#define RAFTX_NSLOT RAFTX_SWEEP_SLOTS   // crossings in flight per context: one downloading its responses, one solving, one generated / queued, one uploading
#include "raftx_owned.h"
#include "raftx_landing.h"

// A raftx_build_designs in flight: phase 1 (descriptor H2D, member pass, scans, totals to the host) has been enqueued,
// phase 2 (strip tables, statics) follows once the totals are known.  The sweep crossing keeps several of them in flight.
struct BuildJob {
    GeomArgs A{};
    Bag tmp;                            // descriptor uploads and per-member scratch: back to the pool when the job retires
    int nDesign = 0, nw = 0;
    int64_t maxMem = 0, maxSta = 0;     // members / stations of the largest design (host loop of phase 1)
    size_t nStrips = 0, nRows = 0;      // totals of phase 1, read by phase 2 (wait_totals): wet strips, MacCamy-Fuchs rows,
    int maxS = 0;                       // strips of the largest design
    double *M0d = nullptr, *C0d = nullptr;
    const double *B0d = nullptr, *MBwd = nullptr;
    bool active = false;
    hipStream_t reduce_stream = nullptr; // (not owned) side stream the member -> platform reductions were launched on (evRed), or null
    // phase 2 left the tables of the designs to the fused kernel that solves them (raftx_fusedgen.h): nothing has been
    // written yet; solve_enqueue launches the generating form, or k_geom_design + k_geom_addup if it cannot
    bool gen_deferred = false;
    size_t gen_lds = 0;                  // dynamic LDS of geom_design_block for this batch
};

// One set of sea-state tables resident for the sweep crossings.  A crossing pins the set it was PREPARED with until it has
// been waited for (or cancelled), so that a later prepare with other sea states on another slot can neither free nor
// replace what an earlier batch still reads (its member pass reads k; its fused kernel everything).
struct CaseSet {
    std::vector<double> key;             // nCase, nHead, nw, depth, rho, g, w, k, zeta, beta as given by the caller
    DevTables T{};                       // only the sea-state fields are used
    Bag allocs;
    int users = 0;                       // crossings prepared or in flight on this set
    unsigned long long stamp = 0;        // last use (the idle set used longest ago is replaced)
};

// Edit program of parametric variants (raftx_variant_program): the base unit's descriptors and the affine edits, resident
// on the device; the uniform offset arrays of a batch of nDesign variants on the host (cached per batch size).
// The member pass of the program's FIXED members (no end edit, no diameter edit on a station: every design has their
// base rows unchanged), run once by k_geom_member_fixed and copied by the member pass of every job
// without per-design poses.  Keyed by what the pass reads besides the rows.  A crossing pins the record it was prepared
// with until it is retired, so that a crossing with another key writes another record (one more than there are slots).
struct FixedRecord {
    bool valid = false;
    double rho = 0, g = 0;
    int trim = 0, haveK = 0;
    double *rec = nullptr;               // [nFix,FR_N]
    int *irec = nullptr;                 // [nFix,FR_I]
    int users = 0;                       // crossings prepared or in flight on this record
    unsigned long long stamp = 0;
    Event ev;                            // the record has been written (on `stream`)
    hipStream_t stream = nullptr;        // (not owned)
};
struct VariantProg {
    int nM = 0, nSt = 0, nCap = 0, nP = 0;
    int nFix = 0;                                                        // fixed members
    int *fixDesc = nullptr, *fixIdx = nullptr;                           // [nFix,5] (FixedArgs::desc) / [nM] record of a member, or -1
    FixedRecord recs[RAFTX_NSLOT + 1];
    unsigned long long rec_clock = 0;
    bool has_caps = false;
    double *gm = nullptr, *gs = nullptr, *gc = nullptr;                  // base descriptors
    int *stMember = nullptr, *capMember = nullptr;                       // member of every station / cap row
    double *stFrac = nullptr, *fillFrac = nullptr, *capFrac = nullptr;   // positions as fractions of the member length
    double *endCoef = nullptr, *headCS = nullptr, *diaCoef = nullptr;
    int *endEdit = nullptr, *diaEdit = nullptr;
    std::vector<int64_t> hS, hC;                                         // base stationOff / capOff (host)
    Bag allocs;                                                          // blocks outside the pool (Bag::get_outside)
    int cachedN = -1;
    std::vector<int64_t> memberOff, stationOff, capOff;                  // uniform offsets of cachedN variants
};
// where a block's descriptors come from when they are not the caller's arrays
struct VariantSrc {
    const VariantProg *prog;
    const double *params;                                                // host, [nDesign of the batch, nP]
    const FixedRecord *rec = nullptr;                                    // the fixed members' record the batch's member passes copy, or null
};

// the program as the kernels see it (V.params stays the caller's)
static void variant_view(const VariantProg &P, VariantView &V) {
    V.nM = P.nM; V.nSt = P.nSt; V.nCap = P.nCap; V.nP = P.nP;
    V.gm = P.gm; V.gs = P.gs; V.gc = P.gc;
    V.stMember = P.stMember; V.capMember = P.capMember;
    V.stFrac = P.stFrac; V.fillFrac = P.fillFrac; V.capFrac = P.capFrac;
    V.endCoef = P.endCoef; V.headCS = P.headCS; V.diaCoef = P.diaCoef;
    V.endEdit = P.endEdit; V.diaEdit = P.diaEdit;
}
static void expand_args(const VariantProg &P, int n, double *gm_out, double *gs_out, double *gc_out, ExpandArgs &E) {
    variant_view(P, E);
    E.n = n;
    E.gm_out = gm_out; E.gs_out = gs_out; E.gc_out = gc_out;
}
// RAFTX_FUSED_GEN=1: sweep crossings build their tables inside the fused kernel (raftx_fusedgen.h).  Read per call -- tests
// switch it inside one process -- when a crossing is prepared (its job then materialises its rows: the generating form
// inlines the plain source of geom_design_block) and when its generation is enqueued.
static bool fused_gen_asked() {
    const char *fg = getenv("RAFTX_FUSED_GEN");
    return fg && atoi(fg);
}

// resident matrices of the dense solves (raftx_dense_resident): device pointers owned by `allocs`
struct DenseResident {
    int nSet = 0, n = 0, nw = 0, freq_mask = 0;
    double *w = nullptr, *M = nullptr, *B = nullptr, *C = nullptr;
    Bag allocs;
};
// The second-order records of the last raftx_qtf_tables_build (include/raftx_qtfgen.h), resident until the next one.
struct QtfResident {
    bool valid = false;
    int nDesign = 0;
    std::vector<int64_t> off;            // host copy of dOff: [QG_CNT_N][nDesign+1] strips | members | Kim & Yue rows | items
    int64_t *dOff = nullptr;
    double *strips = nullptr, *members = nullptr, *kay = nullptr;
    Bag allocs;
    int64_t total(int j) const { return off[(size_t)j * (nDesign + 1) + nDesign]; }
};
struct raftx_ctx;
// Offset arrays of a whole batch, resident on the device (uploaded once by the sweep crossing, shared by its blocks).
struct DevOffsets {
    const int64_t *memberOff, *stationOff, *capOff;      // device copies of the caller's arrays, absolute values
};
struct SeaStates { int nCase, nHead, nw; const double *w, *k; double depth, rho, g; const double *zeta, *beta; };   // sea states as a caller gives them (host arrays)
// Where the designs of a build come from: host arrays of the whole batch (a build takes a slice of designs out of them),
// alive until the build has been waited for.  The sweep crossing keeps the one of its batch for the blocks whose phase 1
// raftx_sweep_launch enqueues.
struct BuildSource {
    const int64_t *memberOff, *stationOff, *capOff;      // the batch's own (absolute) offsets; capOff may be null
    const double *members, *stations, *caps;             // descriptors (null with a variant program)
    const double *pose, *M0, *B0, *C0, *MBw, *Fz_moor, *k;
    double rho, g;
    int nw, add_mask;
    DevOffsets dOff{nullptr, nullptr, nullptr};          // the offsets resident for the whole batch; memberOff == nullptr: every build uploads its slice
    const double *k_dev = nullptr;                       // wave numbers already resident (the crossing's sea-state tables), or null: k is uploaded
    VariantSrc var{nullptr, nullptr};                    // prog == nullptr: the caller's descriptor arrays
};
// rows [lo, lo + n) of `per` doubles each out of a landing region; row d of such an array made NaN (an array not asked for: nothing)
static void rows_out(double *out, const double *src, size_t lo, size_t n, size_t per) {
    if (out && n * per) memcpy(out + lo * per, src, n * per * sizeof(double));
}
static void blank_row(double *a, size_t d, size_t per) {
    if (a) std::fill(a + d * per, a + (d + 1) * per, std::numeric_limits<double>::quiet_NaN());
}
// One sweep crossing in flight: everything raftx_sweep_wait needs to finish it.
struct SweepSlot {
    bool busy = false;                   // launched (phase 2 enqueued), not yet waited for
    int cset = -1;                       // the CaseSet of the parent this crossing was prepared with (pinned until retired)
    int frec = -1;                       // ... and the FixedRecord of the parent's variant program, or -1
    bool prepared = false;               // phase 1 enqueued (descriptor upload, member pass), not yet launched
    int nIter = 0;
    double tol = 0, XiStart = 0, dw = 0;
    std::vector<raftx_ctx *> blk;
    std::vector<int> bnd;
    int nCase = 0, nHead = 0, nw = 0;
    double *sd = nullptr;
    int32_t *niter = nullptr, *flags = nullptr;
    raftx_c128 *Xi = nullptr;
    int64_t *stripOffsets = nullptr;
    Bag allocs;                          // the batch's offset arrays on the device, shared by its blocks
    Event evXi;                          // download of the responses finished (sD2H)
    // phase 1 (descriptor upload + member pass) of the blocks behind the second one is enqueued by raftx_sweep_launch, one
    // block ahead of the block being launched: the caller's arrays (alive until the batch has been waited for) and the
    // batch's device offsets are kept for that
    BuildSource p1{};
    size_t next_p1 = 0;                  // first block whose phase 1 has not been enqueued yet
    std::chrono::steady_clock::time_point t0{};                           // raftx_sweep_prepare was entered
    double since() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }   // host ms
    double tl[4] = {0, 0, 0, 0};
    double span[2] = {0, 0};             // fused launches of the crossing last waited for: start / end, ms since the ctx epoch
    size_t nSlabEv = 0;
    bool slab = false;                   // this crossing's fused launches were cut into slabs (SlabPlan)
    std::vector<double> tlb;             // RAFTX_SWEEP_DEBUG: host time per block of raftx_sweep_launch (upload enqueued | totals seen | enqueued)
    // The requests of a crossing.  Each knows the caller's arrays it fills: collect() copies a block's part (designs lo .. lo + n)
    // out of the block's landing area `land`, blank() makes what the request handed out for design d NaN (collect_pose).
    struct ModalReq {                    // raftx_sweep_modal: eigen analysis of the crossing's designs
        bool on = false;
        const double *dM = nullptr, *dC = nullptr;   // device copies [nDesign,36] (in S.allocs), or null
        double *fn = nullptr, *modes = nullptr, *props = nullptr;   // the caller's outputs, filled by raftx_sweep_wait
        int32_t *flags = nullptr;
        Event evUp;                      // the copies of dM / dC have landed (sCopy)
        void collect(const double *land, size_t lo, size_t n, size_t) {
            if (!on) return;
            const landing::Modal L = landing::modal(n, RAFTX_SP_N);
            rows_out(fn, land + L.fn, lo, n, 6);
            rows_out(modes, land + L.modes, lo, n, 36);
            rows_out(props, land + L.props, lo, n, RAFTX_SP_N);
            memcpy(flags + lo, L.flags.in(land), n * sizeof(int32_t));
        }
        void blank(size_t d, size_t) {
            if (!on) return;
            blank_row(fn, d, 6);
            blank_row(modes, d, 36);
            blank_row(props, d, RAFTX_SP_N);
        }
    } modal;
    struct CurrentReq {                  // raftx_sweep_current: mean current loads of the crossing's designs
        bool on = false;
        int nCur = 0;
        double shearExp = 0;
        std::vector<double> host;        // speed | cos | sin [3,nCur] | Zref [nDesign]: the source of the copies below
        const double *par = nullptr, *Zref = nullptr;   // device copies (in S.allocs); Zref null: 0
        double *D = nullptr;             // the caller's output [nDesign,nCur,6], filled by raftx_sweep_wait
        Event evUp;                      // the copies have landed (sCopy)
        void collect(const double *land, size_t lo, size_t n, size_t) { if (on) rows_out(D, land, lo, n, (size_t)nCur * 6); }
        void blank(size_t d, size_t) { if (on) blank_row(D, d, (size_t)nCur * 6); }
    } current;
    struct ChannelsReq {                 // raftx_sweep_channels: output channels of the crossing's (design, case) pairs
        bool on = false;
        int nChan = 0, nL = 0, nG = 0;   // rows of L: 1 (shared) or nDesign; of Gw: 0 (none), 1 or nDesign
        const double *L = nullptr;       // device copies (in S.allocs) [nL,nChan,3,6]
        const cplx *Gw = nullptr;        // [nG,nChan,6,nw], or null
        double *out = nullptr;           // the caller's output [nDesign,nCase,nChan], filled by raftx_sweep_wait
        Event evUp;                      // the copies have landed (sCopy)
        void collect(const double *land, size_t lo, size_t n, size_t nCase) { if (on) rows_out(out, land, lo, n, nCase * nChan); }
        void blank(size_t d, size_t nCase) { if (on) blank_row(out, d, nCase * nChan); }
    } channels;
    struct MooringReq {                  // raftx_sweep_mooring: the mooring system of the crossing's designs
        bool on = false, add = false;
        int nLine = 0;
        const double *C = nullptr, *Lr = nullptr;   // device (in S.allocs): C_moor [nDesign,36]; J as channel rows [nDesign,2 nLine,3,6]
        Pinned<double> pin;              // landing area of the whole crossing (landing::mooring)
        double *C_out = nullptr, *F_out = nullptr, *T_out = nullptr, *Tstd_out = nullptr;   // the caller's, filled by raftx_sweep_wait
        int32_t *flags_out = nullptr;
        Event evUp;                      // the kernels have run and the landing area is filled (sCopy)
        // (a block's part is T_std; the rest is the crossing's: collect_mooring)
        void collect(const double *land, size_t lo, size_t n, size_t nCase) { if (on) rows_out(Tstd_out, land, lo, n, nCase * 2 * nLine); }
        void blank(size_t d, size_t nCase) {
            if (!on) return;
            blank_row(C_out, d, 36);
            blank_row(F_out, d, 6);
            blank_row(T_out, d, 2 * (size_t)nLine);
            blank_row(Tstd_out, d, nCase * 2 * nLine);
        }
    } mooring;
    struct PoseReq {                     // raftx_sweep_mean_pose: the crossing runs at every design's mean equilibrium pose
        bool on = false;
        int nLine = 0, nX = 0, maxIter = 0, chains = 0;       // chains: the kind of the records (check_lines)
        double tolT = 0, tolR = 0;
        // device, the whole crossing (in S.allocs): the line records; the statics-only extras [nX,36] / [nX,6] and the loads
        // [nDesign,6], each or null; what the solve reads (K_hs, F0), its scratch and what it leaves; the poses of the second pass
        const double *lines = nullptr, *Cx = nullptr, *Fx = nullptr, *Fenv = nullptr;
        double *K = nullptr, *F0 = nullptr, *lw = nullptr, *bw = nullptr, *solved = nullptr, *placed = nullptr, *Fres = nullptr;
        int *iter = nullptr, *fl = nullptr;
        Pinned<double> pin;              // landing area of the whole crossing (landing::pose)
        double *pose_out = nullptr, *Fres_out = nullptr;                     // the caller's, filled by raftx_sweep_wait
        int32_t *iter_out = nullptr, *flags_out = nullptr;
        Event evUp;                      // the inputs have landed and the program's records have been written (sCopy)
    } pose;                              // (its outputs are the whole crossing's and say why a design is flagged: collect_pose, never blanked)
    // The one place that switches the requests of a crossing off: a request left on would fire at the next raftx_sweep_wait
    // and copy into a caller's array that may be gone.
    void clear_requests() { modal.on = current.on = channels.on = mooring.on = pose.on = false; }
};

// The host state of a context.  Every resource is held by an owner (raftx_owned.h), so raftx_ctx_destroy ends in `delete c`
// and THE DECLARATION ORDER OF THE MEMBERS IS THE TEARDOWN ORDER, reversed: a member may use what is declared ahead of it
// until it is destroyed.  Hence: the streams first (destroyed last, after the events recorded and the buffers used on
// them; raftx_ctx_destroy has waited for what was enqueued), then the events, then the pool ahead of every bag -- each bag
// is back in the pool before the pool returns its blocks to the driver -- then the buffers outside the pool, the landing
// areas and the satellites that hold owners of their own.  A new resource goes behind the last thing it depends on.
struct raftx_ctx {
    int device = 0;
    char err[512] = {0};
    // ---- streams
    Stream stream;                       // every kernel that matters; borrowed from the parent in the block contexts of raftx_sweep_stats
    Stream sAux;                         // side stream of the parent ctx: the reductions of the member pass run beside its scans
    Stream sCopy, sPrep, sD2H, sGen;     // internal streams of raftx_sweep_stats (created on first use)
    Stream sSlab[2];                     // with sGen: the streams the slabs of a crossing with responses out go to (SlabPlan)
    Stream sD2Hhigh;                     // bulk download of the responses: a stream of the highest priority class, created when first needed
    // ---- events
    Event ev0, ev1;
    Event evUp, evTot, evG0, evG1, evG2, evG3, evS0, evS1, evDone;   // build phases, statistics, block finished
    Event evZ;                           // the first kernel of the member pass has run (phase 1)
    Event evMem, evRed;                  // member pass done (preparation stream) / per-design reduction done (side stream)
    Event evMoor;                        // C_moor has been added to the block's C0 (raftx_sweep_mooring, sCopy)
    Event evPose;                        // the block's designs have their mean pose (raftx_sweep_mean_pose, preparation stream)
    Event evEpoch;                       // zero of raftx_sweep_solve_span: recorded when the first crossing of the ctx is launched
    std::vector<Event> evSlab;           // completion markers of the slabs (no timing), created as needed, kept
    Event evFork, evJoin;
    // ---- the pool, then the bags that hold its blocks
    DevPool pool;
    Bag design_allocs, case_allocs, result_allocs;
    BuildJob job;
    CaseSet csets[RAFTX_NSLOT + 1];      // sea-state tables of the sweep crossings: one per crossing in flight + one being replaced
    unsigned long long cset_clock = 0;
    DenseResident dense;                 // matrices kept for raftx_solve_dense_resident
    VariantProg vprog;                   // raftx_variant_program
    QtfResident qt;                      // raftx_qtf_tables_build
    SweepSlot slots[RAFTX_NSLOT];        // crossings in flight (raftx_sweep_prepare / _launch / _wait)
    // ---- buffers outside the pool
    DevBuf<double> rXl;
    struct FlexStart {                   // raftx_flex_start: the linearisation point of the next raftx_flex_solve, one-shot
        DevBuf<cplx> x;                  // device copy
        size_t n = 0;                    // entries set (0: none)
        size_t take() { return std::exchange(n, (size_t)0); }   // the size of a pending start, which is spent with this
    } flexStart;
    DevBuf<unsigned long long> rXlSlots;
    DevBuf<unsigned> kpCtr;              // claim counters of the persistent fused launches: a ring of KP_RING sets of 8 (one per XCD slab, 128 B apart)
    DevBuf<cplx> rQtf;                   // QTFs of the last raftx_qtf_slender call, kept for raftx_qtf_force
    DevBuf<cplx> rXl0, rXlOut;           // optional restart point / exported linearisation point [npair,6,nw]: both or neither
    DevBuf<int> pairList;                // device pair lists of a launch split into LDS classes
    DevBuf<int> identList;               // 0, 1, 2, ..: the pair list of a launch cut into slabs (SlabPlan)
    DevBuf<unsigned long long> dbg;
    DevBuf<cplx> rKay;                   // Kim & Yue table of raftx_qtf_kay, consumed by the next raftx_qtf_slender call
    DevBuf<cplx> bemF;                   // resident BEM (+ added) excitation of raftx_bem_excitation [npair,nHead,6,nw]
    DevBuf<int> commFlag;                // one int in HBM: the status word the ranks agree on before an exchange step (comm_agree)
    struct {                             // raftx_mooring_program: base records and the affine edits of their end points
        int nLine = 0, nP = 0, chains = 0;   // chains: the kind of the base records (check_lines: 0, 1 continuation rows, 2 leg rows)
        DevBuf<double> base, coef;
        DevBuf<int> edit;
    } mprog;
    // ---- page-locked landing areas
    Pinned<long long> pin;               // landing area of the build totals and offsets [PIN_OFF + nDesign + 1]
    Pinned<double> pinRes;               // ... of a block's statistics (sweep crossing)
    Pinned<double> pinModal;             // ... of a block's eigen analysis (raftx_sweep_modal)
    Pinned<double> pinCur;               // ... of a block's current loads (raftx_sweep_current)
    Pinned<double> pinChan;              // ... of a block's output channels (raftx_sweep_channels) [pairs,nChan]
    Pinned<double> pinMoorT;             // ... of a block's tension statistics (raftx_sweep_mooring) [pairs,2 nLine]
    // ---- plain state
    DevTables T{};
    // resident results of the last raftx_solve_dynamics_device (device pointers owned by result_allocs)
    cplx *rXi = nullptr, *rFw = nullptr, *rZ = nullptr, *rFe = nullptr;
    double *rB = nullptr;
    int *rNi = nullptr, *rFl = nullptr;
    size_t r_npair = 0, r_nx = 0, r_nz = 0;
    int r_mask = 0;
    int r_last_mask = 0;                 // RAFTX_WANT_* outputs the LAST fused solve wrote (r_mask: what the buffers could hold)
    bool r_fe = false;
    unsigned kpNext = 0;
    int nCU = 0;                         // compute units of the device (the persistent grid is what they hold at once)
    int last_flags = -1, last_minb = 0, last_rc = 0;       // specialisation of the last fused-kernel launch (raftx_last_solve_kernel)
    int last_persist = 0, last_grid = 0, last_pairs = -1;  // its launch form: persistent?, workgroups, pairs (raftx_last_solve_launch)
    int rQtf_sets = 0, rQtf_nw2 = 0, rKay_sets = 0, rKay_nw2 = 0;
    bool have_xl0 = false, want_xlout = false;
    int maxS = 0;
    std::vector<int> hS;                 // submerged strips of every design (host copy: LDS classes of the fused kernel)
    double last_ms = 0.0;
    bool have_designs = false, have_cases = false;
    int nw_designs = 0;
    bool kay_ready = false, bem_ready = false;
    // results of the last raftx_build_designs (device pointers owned by design_allocs)
    int g_n = 0;
    size_t g_nStrips = 0, g_nRows = 0;
    double *g_abi = nullptr, *g_A = nullptr, *g_Ch = nullptr, *g_Wh = nullptr, *g_props = nullptr, *g_Ms = nullptr, *g_Cs = nullptr, *g_Ws = nullptr;
    bool last_gen_fused = false;         // the last fused launch generated its designs' tables itself (raftx_fusedgen.h)
    cplx *g_cm = nullptr;
    void *comm = nullptr;                // ncclComm_t of raftx_comm_init (RCCL), or null
    int comm_rank = 0, comm_world = 1;
    std::vector<raftx_ctx *> workers[RAFTX_NSLOT]; // block contexts of the sweep crossings (device buffers, pool, events), per slot, kept for reuse; destroyed by raftx_ctx_destroy
};

#define MAX_NW 2048
#define HIPCHK(ctx, call)                                                                              \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            snprintf((ctx)->err, sizeof((ctx)->err), "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                     __FILE__, __LINE__);                                                              \
            return -2;                                                                                 \
        }                                                                                              \
    } while (0)
#define FAIL(ctx, ...)                                        \
    do {                                                      \
        snprintf((ctx)->err, sizeof((ctx)->err), __VA_ARGS__); \
        return -1;                                            \
    } while (0)

extern "C" int raftx_version(void) { return RAFTX_VERSION; }
extern "C" int raftx_is_device(void) { return 1; }
extern "C" int raftx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

extern "C" int raftx_ctx_create(int device_id, raftx_ctx **out) {
    if (!out) return -1;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return -3;   // no GPU: fail loudly, no fallback
    if (device_id < 0 || device_id >= ndev) return -4;
    if (hipSetDevice(device_id) != hipSuccess) return -5;
    raftx_ctx *c = new raftx_ctx();
    c->device = device_id;
    // the ctx stream -- the fused fixed points, table generation, statistics -- is of the default priority class (a high one
    // lost: profiles/MEASUREMENT_HISTORY.md, "Closed scheduling experiments of the crossing")
    bool ok = c->stream.ensure(hipStreamNonBlocking) == hipSuccess;
    for (Event *e : {&c->evZ, &c->ev0, &c->ev1, &c->evUp, &c->evTot, &c->evG0, &c->evG1, &c->evG2, &c->evG3, &c->evS0,
                     &c->evS1, &c->evDone, &c->evMem, &c->evRed})
        ok = ok && e->ensure() == hipSuccess;
    if (!ok) {
        delete c;                                     // releases what was created
        return -6;
    }
    *out = c;
    return 0;
}

// The variant program of a ctx, its fixed members' records and their events; the mooring program.  Both by move
// assignment of a fresh value: the owners inside (Bag, Event, DevBuf) release what they hold before they take the new one.
static void variant_release(raftx_ctx *c) { c->vprog = VariantProg(); }
static void mooring_program_release(raftx_ctx *c) { c->mprog = {}; }

// Only the ordered steps: everything the ctx holds is released by its owners, in the reverse of the declaration order of
// raftx_ctx (see there).
extern "C" void raftx_ctx_destroy(raftx_ctx *c) {
    if (!c) return;
#ifdef GEOM_PHASE_TIMING
    if (c->stream.owned) {
        unsigned long long ph[10] = {0};
        (void)hipDeviceSynchronize();
        if (hipMemcpyFromSymbol(ph, HIP_SYMBOL(geom_phase_cycles), sizeof(ph)) == hipSuccess && ph[0]) {
            unsigned long long tot = 0;
            for (int i = 0; i < 7; i++) tot += ph[i];
            fprintf(stderr, "[k_geom_design phases, %% of wave time] counts %.1f | generate %.1f | abi out %.1f | runs %.1f | ds out %.1f | g-vectors %.1f | morison+matrices %.1f\n",
                    100.0 * ph[0] / tot, 100.0 * ph[1] / tot, 100.0 * ph[2] / tot, 100.0 * ph[3] / tot, 100.0 * ph[4] / tot,
                    100.0 * ph[5] / tot, 100.0 * ph[6] / tot);
        }
    }
#endif
    (void)raftx_comm_destroy(c);
    if (c->stream.owned) {                            // a crossing prepared and never launched still has work on sCopy / sPrep
        (void)hipSetDevice(c->device);
        (void)hipDeviceSynchronize();
    }
    for (int sl = 0; sl < RAFTX_NSLOT; sl++) {
        for (raftx_ctx *w : c->workers[sl]) raftx_ctx_destroy(w);
        c->workers[sl].clear();
    }
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    delete c;
}

extern "C" int raftx_host_alloc(raftx_ctx *c, size_t bytes, void **out) {
    if (!c || !out) return -1;
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return 0;
}
extern "C" int raftx_host_free(raftx_ctx *c, void *ptr) {
    if (!c) return -1;
    if (ptr) HIPCHK(c, hipHostFree(ptr));
    return 0;
}

// Where the GPU sits on the host: PCI address and NUMA node (sysfs), for placing the feeding thread and its page-locked
// buffers on the socket the GPU hangs off.  No ctx: callers ask before they create one.
extern "C" int raftx_device_locality(int device, char *pci_bus_id, int len, int *numa_node) {
    if (numa_node) *numa_node = -1;
    char id[64] = {0};
    if (hipDeviceGetPCIBusId(id, (int)sizeof(id), device) != hipSuccess) return -2;
    if (pci_bus_id && len > 0) snprintf(pci_bus_id, (size_t)len, "%s", id);
    for (char *p = id; *p; p++) *p = (char)tolower(*p);
    char path[160];
    snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", id);
    if (FILE *f = fopen(path, "r")) {
        int node = -1;
        if (fscanf(f, "%d", &node) == 1 && numa_node) *numa_node = node;
        fclose(f);
    }
    return 0;
}

extern "C" const char *raftx_last_error(raftx_ctx *c) { return c ? c->err : "null ctx"; }
extern "C" double raftx_last_kernel_ms(raftx_ctx *c) { return c ? c->last_ms : 0.0; }

// ---- device memory owned by a bag: a block of the ctx pool for n elements, remembered in `bag` (design_allocs, a job's
// tmp, a slot's allocs, ..), which goes back to the pool as a whole (Bag::release).  A zero count still gives a valid,
// never-read block.
template <typename Tp>
static int pool_alloc(raftx_ctx *c, Bag &bag, size_t n, Tp **out) {
    HIPCHK(c, bag.get(c->pool, n, out));
    return 0;
}
// ... filled from host memory by a copy enqueued on `st`.  An absent or empty host array takes no block and gives a NULL
// device pointer: the kernels test the optional tables for it.
template <typename Tp, typename Dp>
static int upload_on(raftx_ctx *c, hipStream_t st, Bag &bag, const Tp *host, size_t n, Dp *dev) {
    *dev = nullptr;
    if (!host || n == 0) return 0;
    Tp *p = nullptr;
    if (pool_alloc(c, bag, n, &p)) return -2;
    HIPCHK(c, hipMemcpyAsync(p, host, n * sizeof(Tp), hipMemcpyHostToDevice, st));
    *dev = p;
    return 0;
}
template <typename Tp, typename Dp>
static int upload(raftx_ctx *c, Bag &bag, const Tp *host, size_t n, Dp *dev) { return upload_on(c, c->stream, bag, host, n, dev); }

extern "C" int raftx_upload_designs(raftx_ctx *c, int nDesign, const int64_t *stripOffsets, const double *strips,
                                    int nStripFields, const double *M0, const double *B0, const double *C0, int nw,
                                    const double *MBw, const int64_t *cmOffsets, const raftx_c128 *CmMCF) {
    RangeScope range_("raftx_upload_designs: run detection + H2D");
    if (!c) return -1;
    if (nStripFields != NF) FAIL(c, "nStripFields=%d, expected %d", nStripFields, NF);
    if (nDesign < 0 || !stripOffsets || !M0 || !B0 || !C0) FAIL(c, "upload_designs: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->design_allocs.release();
    c->have_designs = false;
    c->bem_ready = false;
    int maxS = 0;
    c->hS.assign((size_t)nDesign, 0);
    for (int d = 0; d < nDesign; d++) {
        int64_t S = stripOffsets[d + 1] - stripOffsets[d];
        if (S < 0) FAIL(c, "strip offsets not monotone at design %d", d);
        if (S > maxS) maxS = (int)S;
        c->hS[(size_t)d] = (int)S;
    }
    // Device strip table.  Straight runs of equally spaced strips (members) are detected here,
    // from the absolute positions alone, so that the kernels can advance the wave kinematics
    // along a run with rotors instead of re-evaluating sincos/exp per strip.  The optional
    // RAFTX_F_STEP / RAFTX_F_UNIT hints of the ABI record are not trusted (nor needed).
    std::vector<double> dsv((size_t)stripOffsets[nDesign] * DS_N, 0.0);
    std::vector<int> dsf((size_t)stripOffsets[nDesign], 0);
    for (int d = 0; d < nDesign; d++)
        derive_design_tables(strips, stripOffsets[d], stripOffsets[d + 1], dsv.data(), dsf.data());
    DevTables &T = c->T;
    T.nDesign = nDesign;
    int rc = 0;
    rc |= upload(c, c->design_allocs, stripOffsets, (size_t)nDesign + 1, &T.off);
    rc |= upload(c, c->design_allocs, dsv.data(), dsv.size(), &T.ds);
    rc |= upload(c, c->design_allocs, dsf.data(), dsf.size(), &T.dsi);
    rc |= upload(c, c->design_allocs, M0, (size_t)nDesign * 36, &T.M0);
    rc |= upload(c, c->design_allocs, B0, (size_t)nDesign * 36, &T.B0);
    rc |= upload(c, c->design_allocs, C0, (size_t)nDesign * 36, &T.C0);
    rc |= upload(c, c->design_allocs, MBw, MBw ? (size_t)nDesign * 72 * nw : 0, &T.MBw);
    T.cmoff = nullptr;
    T.cm = nullptr;
    if (cmOffsets && CmMCF) {
        rc |= upload(c, c->design_allocs, cmOffsets, (size_t)nDesign + 1, &T.cmoff);
        rc |= upload(c, c->design_allocs, reinterpret_cast<const cplx *>(CmMCF), (size_t)cmOffsets[nDesign] * 2 * nw,
                     &T.cm);
    }
    if (rc) return -2;
    HIPCHK(c, hipStreamSynchronize(c->stream));   // host buffers may be released after return
    c->maxS = maxS;
    c->nw_designs = nw;
    c->have_designs = true;
    c->g_n = 0;
    return 0;
}

// ---- geometry -> strip tables + statics on the device (raftx_geom.h): raftx_build_designs in two phases, so that the
// sweep crossing can keep several design blocks in flight.
// Phase 1 enqueues the descriptor H2D on sCopy and, behind it on sPrep, the member pass and the scans; the totals
// (wet strips, MacCamy-Fuchs rows, strips of the largest design, error flags) and the design offsets land in page-locked
// memory and evTot marks them.  Nothing here waits for the device.  The layout of that landing area (raftx_ctx::pin =
// GeomArgs::hostOut) in long longs, as k_geom_scan_t stores it through A.hostOut (raftx_geom.h):
constexpr size_t PIN_TOT = 0;                // [0..2] wet strips, MacCamy-Fuchs rows, strips of the largest design
constexpr size_t PIN_ERR = 3;                // [3..4] the four error flags of GeomArgs::err, as ints
constexpr size_t PIN_OFF = 8;                // [8 .. 8 + nDesign] strip offsets of the designs
// The check of a design source's arrays, made once by the entry point that takes them.  Callers and tests read the texts:
// `bad` is the entry point's own ("build_designs: bad arguments" | "sweep_stats: bad design arguments"), `who` its prefix.
static int check_source(raftx_ctx *c, const BuildSource &B, int nDesign, const char *who, const char *bad) {
    const bool var = B.var.prog != nullptr;
    if (nDesign < 0 || !B.memberOff || (!B.members && !var) || !B.stationOff || (!B.stations && !var) || !B.M0 || !B.B0 || !B.C0)
        FAIL(c, "%s: %s", who, bad);
    if (!var && (B.capOff == nullptr) != (B.caps == nullptr)) FAIL(c, "%s: capOff and caps must be given together", who);
    return 0;
}
static void launch_scan(hipStream_t st, const GeomArgs &A) {
    hipLaunchKernelGGL(k_geom_scan_t<1024>, dim3(1), dim3(1024), 0, st, A);
}
// Designs [lo, lo + nDesign) of a source: their members [m0, m1), stations [s0, s1) and caps [c0, c1) in the batch's arrays.
struct Slice { int lo; int64_t m0, m1, s0, s1, c0, c1; };
static int slice_of(raftx_ctx *c, const BuildSource &B, int lo, int nDesign, Slice &L) {
    if (lo < 0 || nDesign < 0) FAIL(c, "build_designs: bad arguments");
    const int64_t m0 = B.memberOff[lo], m1 = B.memberOff[lo + nDesign];
    if (m1 < m0 || m0 < 0) FAIL(c, "build_designs: member offsets not monotone");
    const int64_t s0 = B.stationOff[m0], s1 = B.stationOff[m1];
    if (s1 < s0 || s0 < 0) FAIL(c, "build_designs: station offsets not monotone");
    const int64_t c0 = B.capOff ? B.capOff[m0] : 0, c1 = B.capOff ? B.capOff[m1] : 0;
    if (c1 < c0 || c0 < 0) FAIL(c, "build_designs: cap offsets not monotone");
    L = {lo, m0, m1, s0, s1, c0, c1};
    return 0;
}
// The slice's descriptors into device memory, copied on sCopy.  Offsets: the slice of the batch's resident arrays, or
// uploaded here.  Members, stations and caps: the slice of the caller's arrays, or with a variant program only the
// parameters -- the job then keeps no rows and its kernels evaluate them on read (A.prog), or, where the tables may be left
// to the generating fused form, E says what k_geom_expand writes the rows from (E.gm_out != null).  The per-design matrices
// stay with the tables (design_allocs); the rest goes back to the pool when the job retires.
static int upload_descriptors(raftx_ctx *c, hipStream_t sCopy, const BuildSource &B, const Slice &L, ExpandArgs &E) {
    BuildJob &J = c->job;
    GeomArgs &A = J.A;
    Bag &tmp = J.tmp, &keep = c->design_allocs;
    const size_t lo = (size_t)L.lo, nDesign = (size_t)A.nDesign, nMember = (size_t)A.nMember, nw = (size_t)B.nw;
    const size_t nSta = (size_t)(L.s1 - L.s0), nCap = (size_t)(L.c1 - L.c0);
    int rc = 0;
    if (B.dOff.memberOff) {
        A.memberOff = B.dOff.memberOff + lo;
        A.stationOff = B.dOff.stationOff + L.m0;
        A.capOff = B.capOff ? B.dOff.capOff + L.m0 : nullptr;
    } else {
        rc |= upload_on(c, sCopy, tmp, B.memberOff + lo, nDesign + 1, &A.memberOff);
        rc |= upload_on(c, sCopy, tmp, B.stationOff + L.m0, nMember + 1, &A.stationOff);
        if (B.capOff) rc |= upload_on(c, sCopy, tmp, B.capOff + L.m0, nMember + 1, &A.capOff);
    }
    memset(&E, 0, sizeof(E));
    if (const VariantProg *P = B.var.prog) {
        // variants of one base unit: only their parameters cross the bus (nP doubles per design).  No row is written: the
        // member pass, the ballast trim and the generation evaluate a row from the base row where they load it ...
        if (nMember != nDesign * P->nM || nSta != nDesign * P->nSt || nCap != nDesign * P->nCap)
            FAIL(c, "build_designs: offsets do not describe %d variants of the program's base unit", A.nDesign);
        const double *params = nullptr;
        if (nDesign * P->nP) rc |= upload_on(c, sCopy, tmp, B.var.params + lo * P->nP, nDesign * P->nP, &params);
        else rc |= pool_alloc(c, tmp, 1, &params);                  // no parameter: a valid, never-read address (it marks A.prog)
        if (fused_gen_asked()) {
            // ... unless the generating fused form may take the tables: the rows in HBM, written by k_geom_expand on sPrep ahead of
            // the member pass
            double *gm = nullptr, *gs = nullptr, *gc = nullptr;
            if (pool_alloc(c, tmp, nMember * RAFTX_GM_N, &gm) || pool_alloc(c, tmp, nSta * RAFTX_GS_N, &gs) ||
                pool_alloc(c, tmp, nCap * RAFTX_GC_N, &gc))
                return -2;
            E.params = params;
            expand_args(*P, A.nDesign, gm, gs, gc, E);
            A.gm = gm; A.gs = gs; A.caps = B.capOff ? gc : nullptr;
        } else {
            variant_view(*P, A.prog);
            A.prog.params = params;
        }
    } else {
        rc |= upload_on(c, sCopy, tmp, B.members + (size_t)L.m0 * RAFTX_GM_N, nMember * RAFTX_GM_N, &A.gm);
        rc |= upload_on(c, sCopy, tmp, B.stations + (size_t)L.s0 * RAFTX_GS_N, nSta * RAFTX_GS_N, &A.gs);
    }
    rc |= upload_on(c, sCopy, tmp, B.pose ? B.pose + lo * 6 : nullptr, nDesign * 6, &A.pose);
    if (B.capOff && !B.var.prog) {
        if (nCap) rc |= upload_on(c, sCopy, tmp, B.caps + (size_t)L.c0 * RAFTX_GC_N, nCap * RAFTX_GC_N, &A.caps);
        else rc |= pool_alloc(c, tmp, RAFTX_GC_N, &A.caps);        // no caps in this slice: a valid, never-read address
    }
    if (B.k_dev) A.k = B.k_dev;                   // wave numbers already resident (the sweep crossing's sea-state tables)
    else rc |= upload_on(c, sCopy, keep, B.k, nw, &A.k);
    rc |= upload_on(c, sCopy, keep, B.M0 + lo * 36, nDesign * 36, &J.M0d);
    rc |= upload_on(c, sCopy, keep, B.C0 + lo * 36, nDesign * 36, &J.C0d);
    rc |= upload_on(c, sCopy, keep, B.B0 + lo * 36, nDesign * 36, &J.B0d);
    rc |= upload_on(c, sCopy, keep, B.MBw ? B.MBw + lo * 72 * nw : nullptr, nDesign * 72 * nw, &J.MBwd);
    if (B.Fz_moor) rc |= upload_on(c, sCopy, tmp, B.Fz_moor + lo, nDesign, &A.Fz);
    if (rc) return -2;
    A.M0 = J.M0d; A.C0 = J.C0d;
    return 0;
}
// device-side scratch of the member pass and the scans (on a pooled block a memset on sPrep is ordered before the kernels
// that use it); kept with the tables: the offsets the scans leave and the per-design results of the reductions
static int alloc_member_scratch(raftx_ctx *c) {
    GeomArgs &A = c->job.A;
    Bag &tmp = c->job.tmp, &keep = c->design_allocs;
    const size_t nDesign = (size_t)A.nDesign, nMember = (size_t)A.nMember;
    if (pool_alloc(c, tmp, nMember, &A.cnt) || pool_alloc(c, tmp, nMember, &A.cntm) || pool_alloc(c, tmp, nMember * MP_N, &A.mpose) ||
        pool_alloc(c, tmp, nMember * MH_N, &A.mhyd) || pool_alloc(c, tmp, nMember * MI_N, &A.minert) || pool_alloc(c, tmp, 4, &A.err) ||
        pool_alloc(c, tmp, nMember, &A.mdesign_w) || pool_alloc(c, tmp, nDesign, &A.drho) || pool_alloc(c, tmp, 5, &A.tot) ||
        pool_alloc(c, keep, nDesign + 1, &A.off) || pool_alloc(c, keep, nDesign + 1, &A.cmoff) || pool_alloc(c, keep, nDesign * 36, &A.Ch) ||
        pool_alloc(c, keep, nDesign * 6, &A.Wh) || pool_alloc(c, keep, nDesign * 36, &A.Ms) || pool_alloc(c, keep, nDesign * 36, &A.Cs) ||
        pool_alloc(c, keep, nDesign * 6, &A.Ws) || pool_alloc(c, keep, nDesign * RAFTX_SP_N, &A.props))
        return -2;
    A.mdesign = A.mdesign_w;
    return 0;
}
// the member offsets of every design, checked here (the kernels walk them): monotone, inside the slice; and the
// largest design's members / stations (they size the LDS of k_geom_design)
static int design_bounds(raftx_ctx *c, const BuildSource &B, const Slice &L) {
    BuildJob &J = c->job;
    J.maxMem = J.maxSta = 0;
    for (int d = 0; d < J.nDesign; d++) {
        const int64_t a = B.memberOff[L.lo + d], b = B.memberOff[L.lo + d + 1];
        if (b < a || a < L.m0 || b > L.m1) FAIL(c, "member offsets not monotone at design %d", L.lo + d);
        if (B.stationOff[b] < B.stationOff[a]) FAIL(c, "build_designs: station offsets not monotone");
        J.maxMem = std::max(J.maxMem, b - a);
        J.maxSta = std::max(J.maxSta, B.stationOff[b] - B.stationOff[a]);
    }
    return 0;
}
static int enqueue_member_pass(raftx_ctx *c, hipStream_t sPrep) {
    BuildJob &J = c->job;
    GeomArgs &A = J.A;
    const int64_t nDesign = J.nDesign, nMember = A.nMember;
    hipLaunchKernelGGL(k_geom_zero, dim3((unsigned)(nDesign / 256 + 1)), dim3(256), 0, sPrep, A);
    HIPCHK(c, hipEventRecord(c->evZ, sPrep));
    HIPCHK(c, hipEventRecord(c->evG2, sPrep));
    A.mgrid = 0;
    if (nMember > 0) {
        // member kernels on a (member position, design) grid when that wastes few threads: wavefronts of like members
        A.mgrid = (nDesign >= 64 && J.maxMem * nDesign <= nMember + nMember / 4) ? (int)J.maxMem : 0;
        const int64_t nThread = A.mgrid > 0 ? (int64_t)A.mgrid * nDesign : nMember;
        hipLaunchKernelGGL(k_geom_member, dim3((unsigned)((nThread + 127) / 128)), dim3(128), 0, sPrep, A);
        if (A.add_mask & RAFTX_TRIM_BALLAST) {            // heave trim: density correction, then the inertia again
            hipLaunchKernelGGL(k_geom_trim, dim3((unsigned)(nDesign / 128 + 1)), dim3(128), 0, sPrep, A);
            hipLaunchKernelGGL(k_geom_reinertia, dim3((unsigned)((nThread + 127) / 128)), dim3(128), 0, sPrep, A);
        }
    }
    return 0;
}
// The member pass of an enqueued job once more, at the poses A.pose now points to (raftx_sweep_mean_pose): the same grid, the
// counts and totals cleared, no ballast trim -- the density correction is the first pass's, taken at the reference pose.
static int enqueue_member_repass(raftx_ctx *c, hipStream_t sPrep) {
    BuildJob &J = c->job;
    GeomArgs &A = J.A;
    const int64_t nDesign = J.nDesign, nMember = A.nMember;
    hipLaunchKernelGGL(k_geom_rezero, dim3((unsigned)(nDesign / 256 + 1)), dim3(256), 0, sPrep, A);
    if (nMember > 0) {
        const int64_t nThread = A.mgrid > 0 ? (int64_t)A.mgrid * nDesign : nMember;
        hipLaunchKernelGGL(k_geom_member, dim3((unsigned)((nThread + 127) / 128)), dim3(128), 0, sPrep, A);
        if (A.add_mask & RAFTX_TRIM_BALLAST)
            hipLaunchKernelGGL(k_geom_reinertia, dim3((unsigned)((nThread + 127) / 128)), dim3(128), 0, sPrep, A);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}
// The scans (totals, error flags and design offsets reach the host through their own stores into page-locked memory,
// A.hostOut: a D2H copy of them would queue on the DMA engine behind a bulk download of the previous batch) and the member
// -> platform reductions, which need the member pass only.  A crossing's block (a preparation stream apart from its ctx
// stream) runs the reductions on a side stream beside the scans, off the stream the fused kernel waits on (phase 2
// orders the design kernel behind them) -- and the scan and its markers first: streams share hardware queues, and a
// reduction submitted ahead of the scan on the same queue would sit on the path to the totals (the host waits for them
// before it can size and launch the generation).
static int enqueue_scan_reduce(raftx_ctx *c, hipStream_t sPrep) {
    BuildJob &J = c->job;
    const bool side = J.nDesign > 0 && sPrep != c->stream;
    auto scan = [&]() -> int {
        if (J.nDesign > 0) launch_scan(sPrep, J.A);
        HIPCHK(c, hipEventRecord(c->evG3, sPrep));
        HIPCHK(c, hipEventRecord(c->evTot, sPrep));
        return 0;
    };
    J.reduce_stream = nullptr;
    hipStream_t sRed = sPrep;
    if (side) {
        HIPCHK(c, hipEventRecord(c->evMem, sPrep));
        if (scan()) return -2;
        HIPCHK(c, c->sAux.ensure(hipStreamNonBlocking));
        sRed = c->sAux;
        HIPCHK(c, hipStreamWaitEvent(sRed, c->evMem, 0));
    }
    if (J.nDesign > 0) hipLaunchKernelGGL(k_geom_reduce, dim3((unsigned)(((size_t)J.nDesign * 3 + 63) / 64)), dim3(64), 0, sRed, J.A);
    if (!side) return scan();
    HIPCHK(c, hipEventRecord(c->evRed, sRed));
    J.reduce_stream = sRed;
    return 0;
}
// Designs [lo, lo + nDesign) of the source, which its entry point has checked (check_source).
static int build_phase1(raftx_ctx *c, hipStream_t sCopy, hipStream_t sPrep, const BuildSource &B, int lo, int nDesign) {
    RangeScope range_("build phase 1: descriptor H2D, member pass, scans (enqueue)");
    BuildJob &J = c->job;
    Slice L;
    if (int rc = slice_of(c, B, lo, nDesign, L)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    c->design_allocs.release();               // callers guarantee that nothing in flight reads the previous tables
    J.tmp.release();
    c->have_designs = false; c->bem_ready = false; c->g_n = 0;
    HIPCHK(c, c->pin.reserve(PIN_OFF + (size_t)nDesign + 1));
    GeomArgs &A = J.A;
    memset(&A, 0, sizeof(A));
    A.nDesign = nDesign; A.nMember = L.m1 - L.m0;
    A.rho = B.rho; A.g = B.g; A.nw = B.nw; A.add_mask = B.add_mask;
    A.mbase = L.m0; A.sbase = L.s0; A.cbase = L.c0;
    A.hostOut = c->pin.p;
    memset(c->pin.p, 0, (PIN_OFF + 1) * sizeof(long long));
    J.nDesign = nDesign; J.nw = B.nw;
    ExpandArgs E;
    if (int rc = upload_descriptors(c, sCopy, B, L, E)) return rc;
    HIPCHK(c, hipEventRecord(c->evUp, sCopy));
    HIPCHK(c, hipStreamWaitEvent(sPrep, c->evUp, 0));
    if (B.var.prog && nDesign > 0) {
        // a job that materialises its rows (upload_descriptors): the expansion on the preparation stream, ahead of the member
        // pass -- its stores land inside the running fused kernel of the batch before (a high-priority stream of its own gained
        // nothing: profiles/MEASUREMENT_HISTORY.md, "Closed scheduling experiments of the crossing")
        if (E.gm_out) launch_expand(E, sPrep);
        if (const FixedRecord *R = B.var.rec) {
            // the fixed members' pass ran once for the program: this job's member pass copies it
            if (R->stream != sPrep) HIPCHK(c, hipStreamWaitEvent(sPrep, R->ev, 0));
            A.fixRec = R->rec; A.fixInt = R->irec; A.fixIdx = B.var.prog->fixIdx; A.fixNM = B.var.prog->nM;
        }
    }
    if (int rc = alloc_member_scratch(c)) return rc;
    if (int rc = design_bounds(c, B, L)) return rc;
    if (int rc = enqueue_member_pass(c, sPrep)) return rc;
    if (int rc = enqueue_scan_reduce(c, sPrep)) return rc;
    J.active = true;
    return 0;
}

// Phase 2: waits (host) for the totals of phase 1, sizes the strip tables, and enqueues strip generation, the MacCamy-
// Fuchs table and the per-design reduction on the ctx stream, ordered behind phase 1 by evTot.  Does not wait for them.
// sGen: the stream the generation kernels go to (null: the ctx stream).  The sweep crossing gives the preparation stream
// for every block but the first, so that a block's tables are generated WHILE the fused kernel of the block before it
// runs (they fill the CUs its last residency round leaves idle); the ctx stream is ordered behind them by evG1.
// kind: 0 = a raftx_build_designs call (tables + ABI copy of the strip records), or bits:
constexpr int GEN_CROSSING = 1;      // a block of a sweep crossing (no ABI copy)
constexpr int GEN_MAY_DEFER = 2;     // ... whose tables may be left to the fused kernel (RAFTX_FUSED_GEN=1)
constexpr int GEN_PIPELINED = 4;     // ... with other crossings in flight (its member pass ran a step ago: the generation adds the design matrices up itself)
static void launch_design(raftx_ctx *c, hipStream_t st) {
    hipLaunchKernelGGL(k_geom_design, dim3((unsigned)c->job.nDesign), dim3(GD_T), c->job.gen_lds, st, c->job.A);
}
// the totals and error flags of phase 1, from the landing area, into the job; the strip offsets to the caller
static int wait_totals(raftx_ctx *c, int64_t *stripOffsets) {
    BuildJob &J = c->job;
    for (;;) {                                        // spin: the blocking wait costs ~0.2 ms of wake-up latency per block
        const hipError_t q = hipEventQuery(c->evTot);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) HIPCHK(c, q);
    }
    HIPCHK(c, hipGetLastError());
    const int *bad = reinterpret_cast<const int *>(c->pin.p + PIN_ERR);
    if (bad[3] > 0) FAIL(c, "member %d: needs 2..%d stations, dlsMax > 0 and length > 0", bad[3] - 1, GEOM_MAX_STATIONS);
    if (bad[3] < 0) FAIL(c, "build_designs: member %d is MacCamy-Fuchs but no wave numbers were given", -bad[3] - 1);
    if (bad[0]) FAIL(c, "member %d: cap/bulkhead layout not supported (the reference raises here too)", bad[0] - 1);
    if (bad[1]) FAIL(c, "design %d: ballast trim needs some ballast volume", bad[1] - 1);
    J.nStrips = (size_t)c->pin.p[PIN_TOT]; J.nRows = (size_t)c->pin.p[PIN_TOT + 1]; J.maxS = (int)c->pin.p[PIN_TOT + 2];
    const long long *off = c->pin.p + PIN_OFF;
    if (stripOffsets) memcpy(stripOffsets, off, ((size_t)J.nDesign + 1) * sizeof(int64_t));
    c->hS.resize((size_t)J.nDesign);
    for (int d = 0; d < J.nDesign; d++) c->hS[(size_t)d] = (int)(off[d + 1] - off[d]);
    return 0;
}
static int enqueue_generation(raftx_ctx *c, hipStream_t sGen, int kind) {
    BuildJob &J = c->job;
    GeomArgs &A = J.A;
    const int nDesign = J.nDesign, nw = J.nw;
    const size_t nRows = J.nRows;
    // RAFTX_FUSED_GEN=1: sweep crossings build their tables inside the fused kernel (raftx_fusedgen.h).  Measured and NOT
    // the default (profiles/r06_experiments/fused_generation_ab.txt): bit-identical, the gap between two fused kernels
    // shrinks from 0.30 to 0.09 ms, but the kernel grows by 0.50 ms -- the ~50 us of dependent loads per design are not
    // hidden by the seven other waves of the CU (each is bound by its own dependency chains, not by issue slots).
    // A job that keeps no rows (A.prog: prepared without the variable) takes the k_geom_design route: the generating form
    // inlines the plain source.
    const bool defer = (kind & GEN_MAY_DEFER) && fused_gen_asked() && !A.prog.params && nDesign > 0 && nRows == 0;
    J.gen_deferred = false;
    const size_t gd_lds = geom_design_lds(J.maxS, (int)J.maxSta, (int)J.maxMem);
    if (gd_lds > 160 * 1024)
        FAIL(c, "build_designs: designs of up to %d submerged strips, %d stations and %d members need %zu B of LDS in k_geom_design, 160 KiB available",
             J.maxS, (int)J.maxSta, (int)J.maxMem, gd_lds);
    if (gd_lds > 64 * 1024)
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_geom_design), hipFuncAttributeMaxDynamicSharedMemorySize, (int)gd_lds));
    J.gen_lds = gd_lds;
    if (!sGen || defer) sGen = c->stream;
    HIPCHK(c, hipStreamWaitEvent(sGen, c->evTot, 0));
    HIPCHK(c, hipEventRecord(c->evG0, sGen));
    if (defer) {
        // the ctx stream (where the fused kernel goes) behind everything the generation reads: scans, reductions
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->evTot, 0));
        if (J.reduce_stream) HIPCHK(c, hipStreamWaitEvent(c->stream, c->evRed, 0));
        J.gen_deferred = true;
    } else if (nDesign > 0) {
        // A sweep crossing in flight behind others (its member pass and reductions ran a step ago): the generation adds its
        // design's matrices up itself -- one kernel and one launch gap less on the path between two fused kernels (same
        // additions in the same order: bit-identical).  RAFTX_ADDUP_KERNEL=1 keeps k_geom_addup.
        static const bool addup_kernel = getenv("RAFTX_ADDUP_KERNEL") && atoi(getenv("RAFTX_ADDUP_KERNEL"));
        A.addup_in_design = ((kind & GEN_PIPELINED) && !addup_kernel && nRows == 0 && !A.abi) ? 1 : 0;
        if (A.addup_in_design && J.reduce_stream) HIPCHK(c, hipStreamWaitEvent(sGen, c->evRed, 0));
        launch_design(c, sGen);
        if (!A.addup_in_design) {
            // the reductions of phase 1 (side stream) are not waited for until their results are added up: streams share
            // hardware queues, and a reduction that ended up behind the scan would otherwise hold the generation back
            if (J.reduce_stream) HIPCHK(c, hipStreamWaitEvent(sGen, c->evRed, 0));
            hipLaunchKernelGGL(k_geom_addup, dim3((unsigned)(((size_t)nDesign * 36 + 255) / 256)), dim3(256), 0, sGen, A);
        }
    }
    if (nRows > 0)                                        // after k_geom_design: it leaves (R, Ca) of the MacCamy-Fuchs strips
        hipLaunchKernelGGL(k_geom_mcf, dim3((unsigned)nRows, (unsigned)((nw + 63) / 64)), dim3(64), 0, sGen, A, (int64_t)nRows);
    HIPCHK(c, hipEventRecord(c->evG1, sGen));
    if (sGen != c->stream) HIPCHK(c, hipStreamWaitEvent(c->stream, c->evG1, 0));
    return 0;
}
// the finished job's tables become the designs of the ctx: what the solves (c->T) and the fetch calls (c->g_*) read
static void publish_tables(raftx_ctx *c) {
    const BuildJob &J = c->job;
    const GeomArgs &A = J.A;
    DevTables &T = c->T;
    T.nDesign = J.nDesign; T.off = A.off; T.ds = A.ds; T.dsi = A.dsi;
    T.M0 = J.M0d; T.C0 = J.C0d; T.B0 = J.B0d; T.MBw = J.MBwd;
    T.cmoff = J.nRows ? A.cmoff : nullptr; T.cm = J.nRows ? A.cm : nullptr;
    c->maxS = J.maxS; c->nw_designs = J.nw; c->have_designs = true;
    c->g_n = J.nDesign; c->g_nStrips = J.nStrips; c->g_nRows = J.nRows;
    c->g_abi = A.abi; c->g_cm = A.cm;
    c->g_A = A.A; c->g_Ch = A.Ch; c->g_Wh = A.Wh; c->g_props = A.props;
    c->g_Ms = A.Ms; c->g_Cs = A.Cs; c->g_Ws = A.Ws;
}
static int build_phase2(raftx_ctx *c, int64_t *stripOffsets, hipStream_t sGen = nullptr, int kind = 0) {
    RangeScope range_("build phase 2: wait for totals, strip tables + statics (enqueue)");
    BuildJob &J = c->job;
    GeomArgs &A = J.A;
    if (!J.active) FAIL(c, "build_designs: phase 2 without phase 1");
    if (int rc = wait_totals(c, stripOffsets)) return rc;
    // the ABI copy of the strip records (raftx_fetch_strips) is for raftx_build_designs; a sweep crossing never
    // fetches it: 137 MB of stores per 10 000 designs less between two fused kernels (k_geom_design checks the pointer)
    Bag &keep = c->design_allocs;
    A.abi = nullptr;
    if ((!kind && pool_alloc(c, keep, J.nStrips * NF, &A.abi)) || pool_alloc(c, keep, J.nStrips * DS_N, &A.ds) ||
        pool_alloc(c, keep, J.nStrips, &A.dsi) || pool_alloc(c, keep, J.nRows * 3, &A.mcfaux) ||
        pool_alloc(c, keep, J.nRows * 2 * (size_t)J.nw, &A.cm) || pool_alloc(c, keep, (size_t)J.nDesign * 36, &A.A))
        return -2;
    if (int rc = enqueue_generation(c, sGen, kind)) return rc;
    publish_tables(c);
    return 0;
}
// a build that will not be finished, or has been (the caller has drained the device): its scratch back to the pool
static void build_abandon(raftx_ctx *c) {
    c->job.tmp.release();
    c->job.active = false;
}
// kernel time of a finished build (both phases), and its scratch back to the pool
static int build_retire(raftx_ctx *c, double *ms_out) {
    float a = 0.f, b = 0.f;
    if (c->job.active) {
        HIPCHK(c, hipEventElapsedTime(&a, c->evG2, c->evG3));
        HIPCHK(c, hipEventElapsedTime(&b, c->evG0, c->evG1));
    }
    if (ms_out) *ms_out = (double)a + (double)b;
    build_abandon(c);
    return 0;
}

extern "C" int raftx_build_designs(raftx_ctx *c, int nDesign, const int64_t *memberOff, const double *members,
                                   const int64_t *stationOff, const double *stations, const int64_t *capOff,
                                   const double *caps, const double *pose, double rho, double g, int nw, const double *k,
                                   int add_mask, const double *M0, const double *B0, const double *C0, const double *MBw,
                                   const double *Fz_moor, int64_t *stripOffsets) {
    if (!c) return -1;
    if (!stripOffsets) FAIL(c, "build_designs: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const BuildSource src{memberOff, stationOff, capOff, members, stations, caps, pose, M0, B0, C0, MBw, Fz_moor, k, rho, g, nw, add_mask};
    int rc = check_source(c, src, nDesign, "build_designs", "bad arguments");
    if (!rc && (nw < 1 || nw > MAX_NW)) {             // (not FAIL: the cleanup below has to follow)
        snprintf(c->err, sizeof(c->err), "build_designs: nw=%d outside 1..%d", nw, MAX_NW);
        rc = -1;
    }
    if (!rc) rc = build_phase1(c, c->stream, c->stream, src, 0, nDesign);
    if (!rc) rc = build_phase2(c, stripOffsets);
    const hipError_t e = hipStreamSynchronize(c->stream);     // host buffers may be released after return
    if (rc) {
        build_abandon(c);
        c->have_designs = false;
        return rc;
    }
    HIPCHK(c, e);
    HIPCHK(c, hipGetLastError());
    double ms = 0.0;
    if (build_retire(c, &ms)) return -2;
    c->last_ms = ms;                                 // the kernels; allocations and descriptor H2D are outside
    return 0;
}

extern "C" int raftx_fetch_strips(raftx_ctx *c, double *strips, raftx_c128 *cm) {
    if (!c) return -1;
    if (!c->g_n || !c->have_designs) FAIL(c, "fetch_strips: no raftx_build_designs call on this ctx");
    HIPCHK(c, hipSetDevice(c->device));
    if (strips && c->g_nStrips && !c->g_abi)
        FAIL(c, "fetch_strips: the tables of this batch were generated by a sweep crossing, which keeps no ABI copy of the strip records");
    if (strips && c->g_nStrips)
        HIPCHK(c, hipMemcpyAsync(strips, c->g_abi, c->g_nStrips * NF * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (cm && c->g_nRows)
        HIPCHK(c, hipMemcpyAsync(cm, c->g_cm, c->g_nRows * 2 * (size_t)c->nw_designs * sizeof(cplx), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int raftx_fetch_statics(raftx_ctx *c, double *A_morison, double *C_hydro, double *W_hydro, double *M_struc,
                                   double *C_struc, double *W_struc, double *props) {
    if (!c) return -1;
    if (!c->g_n || !c->have_designs) FAIL(c, "fetch_statics: no raftx_build_designs call on this ctx");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->g_n;
    if (A_morison) HIPCHK(c, hipMemcpyAsync(A_morison, c->g_A, n * 36 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (C_hydro) HIPCHK(c, hipMemcpyAsync(C_hydro, c->g_Ch, n * 36 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (W_hydro) HIPCHK(c, hipMemcpyAsync(W_hydro, c->g_Wh, n * 6 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (props) HIPCHK(c, hipMemcpyAsync(props, c->g_props, n * RAFTX_SP_N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (M_struc) HIPCHK(c, hipMemcpyAsync(M_struc, c->g_Ms, n * 36 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (C_struc) HIPCHK(c, hipMemcpyAsync(C_struc, c->g_Cs, n * 36 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (W_struc) HIPCHK(c, hipMemcpyAsync(W_struc, c->g_Ws, n * 6 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// The sea-state tables of one set of cases into device memory of ctx `c` (allocations into `bag`, fields into `T`), copied
// on `st`, which has drained when this returns (the depth constants are host temporaries).
static int upload_case_tables(raftx_ctx *c, hipStream_t st, Bag &bag, DevTables &T, const SeaStates &sea) {
    const int nCase = sea.nCase, nHead = sea.nHead, nw = sea.nw;
    const double *k = sea.k, depth = sea.depth;
    // per-bin depth constants, computed once on the host in full libm precision.  The kernels derive
    // the depth regime (k == 0 / deep / finite) from k themselves, with the same rule.
    std::vector<double> csh(nw), cch(nw);
    for (int i = 0; i < nw; i++) {
        double kh = k[i] * depth;
        if (k[i] == 0.0 || kh > 89.4) {   // helpers.py:211-218: Sh = 1, Ch = Cc = 99999  /  Sh = Ch = e^{kz}, Cc = e^{kz} + e^{-k(z+2h)}
            csh[i] = cch[i] = 1.0;
        } else {                          // helpers.py:219-222 written with decaying exponentials only
            double e2kh = exp(-2.0 * kh);
            csh[i] = 1.0 / (-expm1(-2.0 * kh));
            cch[i] = 1.0 / (1.0 + e2kh);
        }
    }
    T.nCase = nCase; T.nHead = nHead; T.nw = nw;
    T.depth = depth; T.rho = sea.rho; T.g = sea.g;
    int rc = 0;
    rc |= upload_on(c, st, bag, sea.w, (size_t)nw, &T.w);
    rc |= upload_on(c, st, bag, k, (size_t)nw, &T.k);
    rc |= upload_on(c, st, bag, csh.data(), (size_t)nw, &T.csh);
    rc |= upload_on(c, st, bag, cch.data(), (size_t)nw, &T.cch);
    rc |= upload_on(c, st, bag, sea.zeta, (size_t)nCase * nHead * nw, &T.zeta);
    rc |= upload_on(c, st, bag, sea.beta, (size_t)nCase * nHead, &T.beta);
    const hipError_t e = hipStreamSynchronize(st);        // also on failure: csh / cch go out of scope
    if (rc) return -2;
    HIPCHK(c, e);
    return 0;
}

extern "C" int raftx_upload_cases(raftx_ctx *c, int nCase, int nHead, int nw, const double *w, const double *k,
                                  double depth, double rho, double g, const double *zeta, const double *beta) {
    RangeScope range_("raftx_upload_cases: H2D");
    if (!c) return -1;
    if (nCase < 0 || nHead < 1 || nw < 1 || !w || !k || !zeta || !beta) FAIL(c, "upload_cases: bad arguments");
    if (nw > MAX_NW) FAIL(c, "nw=%d exceeds the %d bins per workgroup supported by this build", nw, MAX_NW);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->case_allocs.release();
    c->have_cases = false;
    c->bem_ready = false;
    if (int rc = upload_case_tables(c, c->stream, c->case_allocs, c->T, SeaStates{nCase, nHead, nw, w, k, depth, rho, g, zeta, beta})) return rc;
    c->have_cases = true;
    return 0;
}

#define LDS_LIMIT (160 * 1024)

// Launch shape: NB bins per lane x threads per workgroup (one workgroup per pair).  Defaults
// (measured on MI355X, profiles/): two waves per SIMD with 2 bins per lane beat both the
// 4-bins-per-lane / 1-wave-per-SIMD and the 1-bin-per-lane shapes at nw = 200.
//   nw <=  64 : (1,  64)    one wave per pair, no s_barrier anywhere in the kernel
//   nw <= 128 : (2,  64)
//   nw <= 256 : (2, 128)
//   nw <= 512 : (2, 256)
//   larger    : (2..4, 512)
// RAFTX_SHAPE="nb,threads" overrides (tuning only; must be one of the instantiated shapes).
struct Shape {
    int nb, threads;
};
#define SHAPES(X) X(1, 64, 1) X(2, 64, 1) X(4, 64, 1) X(2, 128, MINB_2X128) X(1, 256, 2) X(2, 256, 2) X(2, 512, 1) X(3, 512, 1) X(4, 512, 1)
// (NB, MAXT, MINB) of every instantiated kernel: MAXT is the shape's threads, MINB the waves per SIMD it is compiled for
static bool shape_ok(Shape sh, int nw) {
#define X(NB_, MT_, MB_) if (sh.nb == NB_ && sh.threads == MT_) return (long)NB_ * MT_ >= nw;
    SHAPES(X)
#undef X
    return false;
}
static Shape pick_shape(int nw) {
    static const char *env = getenv("RAFTX_SHAPE");
    if (env) {
        Shape sh = {0, 0};
        if (sscanf(env, "%d,%d", &sh.nb, &sh.threads) == 2 && shape_ok(sh, nw)) return sh;
    }
    if (nw <= 64) return {1, 64};
    if (nw <= 128) return {2, 64};
    if (nw <= 256) return {2, 128};
    if (nw <= 512) return {2, 256};
    int nb = (nw + 511) / 512;
    return {nb < 2 ? 2 : nb, 512};
}

static int prep_lds(raftx_ctx *c, const void *kernel, size_t bytes) {
    if (bytes > LDS_LIMIT)
        FAIL(c, "a design has %d submerged strips / nw=%d: %zu B of LDS needed, 160 KiB available", c->maxS, c->T.nw, bytes);
    if (bytes > 64 * 1024)
        HIPCHK(c, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}
#define NO_KERNEL(c, sh) FAIL(c, "no kernel for shape %d x %d", (sh).nb, (sh).threads)

// Device buffers the ctx keeps outside the pool and regrows on demand: nothing to do while the block holds want_n
// elements (FIT_EXACT: exactly want_n, for the buffers whose count is their shape); otherwise drains what may still use the
// old block (the ctx stream, or the whole device -- the owner itself never synchronises) and lets the buffer grow; on
// failure it is empty.
enum Drain { DRAIN_STREAM, DRAIN_DEVICE };
enum Fit { FIT_AT_LEAST, FIT_EXACT };
template <typename Tp>
static int grow_device(raftx_ctx *c, DevBuf<Tp> &buf, size_t want_n, Drain drain = DRAIN_STREAM, Fit fit = FIT_AT_LEAST) {
    if (fit == FIT_EXACT ? (buf.p && buf.n == want_n) : buf.holds(want_n)) return 0;
    HIPCHK(c, drain == DRAIN_DEVICE ? hipDeviceSynchronize() : hipStreamSynchronize(c->stream));
    HIPCHK(c, buf.grow(want_n));
    return 0;
}

static int check_ready(raftx_ctx *c) {
    if (!c) return -1;
    if (!c->have_designs) FAIL(c, "no designs uploaded");
    if (!c->have_cases) FAIL(c, "no cases uploaded");
    if ((c->T.MBw || c->T.cm) && c->nw_designs != c->T.nw)
        FAIL(c, "nw mismatch between designs (%d) and cases (%d)", c->nw_designs, c->T.nw);
    return 0;
}

#define D2H(c, dst, src, bytes) HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (c)->stream))
#define H2D(c, dst, src, bytes) HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (c)->stream))

static int finish_timed(raftx_ctx *c) {
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->last_ms = ms;
    return 0;
}

// threads of a workgroup whose lanes stride the nw frequency bins of one row (the statistics and channel kernels, k_bem_excitation)
static dim3 bin_threads(int nw) { return dim3(nw > 128 ? 256 : (nw > 64 ? 128 : 64)); }

// The device scratch of one call and the call's protocol on the ctx stream (the arrays: Staging, raftx_owned.h):
//   declare tmp / in / out | upload(who) | anything untimed | begin() | the kernels | finish()
// A call that is not timed ends with download() where the others end with finish().
struct Scratch : Staging {
    raftx_ctx *c;
    explicit Scratch(raftx_ctx *c_) : Staging(c_->pool), c(c_) {}
    ~Scratch() { (void)hipStreamSynchronize(c->stream); }   // ahead of the bag's release: blocks go back to the pool only when nothing in flight uses them
    int upload(const char *who) {                    // -1: a block was refused; else the uploads declared so far, in their order
        if (failed) FAIL(c, "%s: device allocation failed", who);
        HIPCHK(c, send(c->stream));
        return 0;
    }
    int begin() {                                    // the timed window of raftx_last_kernel_ms opens
        HIPCHK(c, hipEventRecord(c->ev0, c->stream));
        return 0;
    }
    int download() {                                 // the result copies, in their order, and the caller's arrays are final
        HIPCHK(c, fetch(c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return 0;
    }
    int finish() { return finish_timed(c) ? -2 : download(); }   // ... after the window has closed and last_ms is set
};

// the instantiated kernel of a shape (nullptr: none)
typedef void (*excitation_fn)(DevTables, cplx *);
static excitation_fn excitation_kernel(Shape sh) {
#define X(NB_, MT_, MB_) if (sh.nb == NB_ && sh.threads == MT_) return k_excitation<NB_, MT_, MB_>;
    SHAPES(X)
#undef X
    return nullptr;
}
extern "C" int raftx_excitation(raftx_ctx *c, raftx_c128 *F_iner) {
    if (check_ready(c)) return -1;
    if (!F_iner) FAIL(c, "excitation: F_iner is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    const DevTables &T = c->T;
    size_t npair = (size_t)T.nDesign * T.nCase;
    size_t n = npair * T.nHead * 6 * T.nw;
    Scratch sc(c);
    cplx *dF = sc.out<cplx>(F_iner, n);
    if (int rc = sc.upload("excitation")) return rc;
    const Shape sh = pick_shape(T.nw);
    if (sc.begin()) return -2;
    if (npair) {
        excitation_fn kernel = excitation_kernel(sh);
        if (!kernel) NO_KERNEL(c, sh);
        hipLaunchKernelGGL(kernel, dim3((unsigned)(npair * T.nHead)), dim3(sh.threads), 0, c->stream, T, dF);
    }
    return sc.finish();
}

typedef void (*linearize_fn)(DevTables, const cplx *, double *, cplx *);
static linearize_fn linearize_kernel(Shape sh) {
#define X(NB_, MT_, MB_) if (sh.nb == NB_ && sh.threads == MT_) return k_linearize<NB_, MT_, MB_>;
    SHAPES(X)
#undef X
    return nullptr;
}
// one drag linearisation on device arrays (enqueued on the ctx stream between ev0 and the caller's ev1)
static int linearize_enqueue(raftx_ctx *c, const cplx *dXi, double *dB, cplx *dF, bool timed = true) {
    const DevTables &T = c->T;
    const size_t npair = (size_t)T.nDesign * T.nCase;
    const Shape sh = pick_shape(T.nw);
    const size_t lds = lds_bytes(c->maxS, 0, sh.threads / 64, stage_policy(sh.nb, sh.threads));
    linearize_fn kernel = linearize_kernel(sh);
    if (!kernel) NO_KERNEL(c, sh);
    if (prep_lds(c, reinterpret_cast<const void *>(kernel), lds)) return -1;
    if (timed) HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    if (npair) hipLaunchKernelGGL(kernel, dim3(grid_for_pairs(npair)), dim3(sh.threads), lds, c->stream, T, dXi, dB, dF);
    return 0;
}
extern "C" int raftx_linearize(raftx_ctx *c, const raftx_c128 *Xi, double *B_drag, raftx_c128 *F_drag) {
    if (check_ready(c)) return -1;
    if (!Xi) FAIL(c, "linearize: Xi is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    const DevTables &T = c->T;
    size_t npair = (size_t)T.nDesign * T.nCase;
    Scratch sc(c);
    cplx *dXi = sc.in<cplx>(Xi, npair * 6 * T.nw);
    double *dB = sc.out<double>(B_drag, npair * 36);
    cplx *dF = sc.out<cplx>(F_drag, npair * T.nHead * 6 * T.nw);
    if (int rc = sc.upload("linearize")) return rc;
    if (linearize_enqueue(c, dXi, dB, dF)) return -1;
    return sc.finish();
}

// the resident strips of one design (host copy of its offsets)
static int strip_count(raftx_ctx *c, int design, int icase, const char *what, int *S) {
    if (check_ready(c)) return -1;
    const DevTables &T = c->T;
    if (design < 0 || design >= T.nDesign || icase < 0 || icase >= T.nCase) FAIL(c, "%s: design / case outside the resident set", what);
    HIPCHK(c, hipSetDevice(c->device));
    int64_t o[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(o, T.off + design, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *S = (int)(o[1] - o[0]);
    return 0;
}
extern "C" int raftx_strip_kinematics(raftx_ctx *c, int design, int icase, raftx_c128 *u, raftx_c128 *ud, raftx_c128 *pDyn) {
    if (!c) return -1;
    int S = 0;
    if (int rc = strip_count(c, design, icase, "strip_kinematics", &S)) return rc;
    const DevTables &T = c->T;
    const size_t n = (size_t)T.nHead * S * T.nw;
    if (!n) return 0;
    Scratch sc(c);
    cplx *du = sc.out<cplx>(u, n * 3), *dud = sc.out<cplx>(ud, n * 3), *dp = sc.out<cplx>(pDyn, n);
    if (int rc = sc.upload("strip_kinematics")) return rc;
    if (sc.begin()) return -2;
    hipLaunchKernelGGL(k_strip_kinematics, dim3((unsigned)(S * T.nHead)), dim3(256), 0, c->stream, T, design, icase, du, dud, dp);
    return sc.finish();
}
extern "C" int raftx_strip_drag(raftx_ctx *c, int design, int icase, const raftx_c128 *Xi, int ih, double *Bmat,
                                raftx_c128 *F_exc_drag) {
    if (!c) return -1;
    int S = 0;
    if (int rc = strip_count(c, design, icase, "strip_drag", &S)) return rc;
    const DevTables &T = c->T;
    if (!Xi) FAIL(c, "strip_drag: Xi is NULL");
    if (ih < 0 || ih >= T.nHead) FAIL(c, "strip_drag: heading outside the resident sea state");
    if (!S) return 0;
    Scratch sc(c);
    cplx *dXi = sc.in<cplx>(Xi, (size_t)6 * T.nw);
    double *dB = sc.out<double>(Bmat, (size_t)S * 9);
    cplx *dF = sc.out<cplx>(F_exc_drag, (size_t)S * 3 * T.nw);
    if (int rc = sc.upload("strip_drag")) return rc;
    if (sc.begin()) return -2;
    hipLaunchKernelGGL(k_strip_drag, dim3((unsigned)S), dim3(256), 0, c->stream, T, design, icase, ih, dXi, dB, dF);
    return sc.finish();
}

template <typename Tp>
static Tp *dev_alloc(raftx_ctx *c, size_t n) {
    Tp *p = nullptr;
    (void)c->result_allocs.get(c->pool, n, &p);
    return p;
}

// (re)size the ctx-owned result buffers for the current designs x cases
static int ensure_results(raftx_ctx *c, int want_mask, bool need_fe) {
    const DevTables &T = c->T;
    size_t npair = (size_t)T.nDesign * T.nCase;
    size_t nx = npair * T.nHead * 6 * T.nw, nz = npair * 36 * T.nw;
    bool ok = c->rXi && c->r_npair == npair && c->r_nx == nx && c->r_nz == nz &&
              (c->r_mask & want_mask) == want_mask && (!need_fe || c->r_fe);
    if (ok) return 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->result_allocs.release();
    c->rXi = c->rFw = c->rZ = c->rFe = nullptr;
    c->rB = nullptr;
    c->rNi = c->rFl = nullptr;
    c->rXi = dev_alloc<cplx>(c, nx);
    c->rNi = dev_alloc<int>(c, npair);
    c->rFl = dev_alloc<int>(c, npair);
    if (want_mask & RAFTX_WANT_BDRAG) c->rB = dev_alloc<double>(c, npair * 36);
    if (want_mask & RAFTX_WANT_FWAVE) c->rFw = dev_alloc<cplx>(c, nx);
    if (want_mask & RAFTX_WANT_Z) c->rZ = dev_alloc<cplx>(c, nz);
    if (need_fe) c->rFe = dev_alloc<cplx>(c, nx);
    if (!c->rXi || !c->rNi || !c->rFl || ((want_mask & RAFTX_WANT_BDRAG) && !c->rB) ||
        ((want_mask & RAFTX_WANT_FWAVE) && !c->rFw) || ((want_mask & RAFTX_WANT_Z) && !c->rZ) || (need_fe && !c->rFe)) {
        c->result_allocs.release();
        c->rXi = nullptr;
        FAIL(c, "solve_dynamics: device allocation of result buffers failed");
    }
    c->r_npair = npair;
    c->r_nx = nx;
    c->r_nz = nz;
    c->r_mask = want_mask;
    c->r_fe = need_fe;
    return 0;
}

// A fused-kernel launch cut into SLABS of the pair list (a crossing that downloads its responses: slab k's download runs
// while the slabs behind it solve).  The slabs go round-robin to the streams `alts`, none to the ctx stream: pairs are
// independent, and a grid queued on another stream is handed out as soon as the grids before it are exhausted -- the
// workgroups of the next slabs fill the CUs a slab's last residency round leaves idle, so a cut costs no tail (slabs as
// consecutive launches of ONE stream each wait for the slowest pair of the slab before: +0.1-0.15 ms per cut,
// profiles/r02_crossing_splits.txt), and the ctx stream stays free for what the NEXT block needs (its table generation
// runs beside these slabs instead of behind them).  `after(p0, p1, s)` enqueues what follows the pairs [p0, p1) on the
// stream s they were launched on.  The caller joins: `slab_join` orders the ctx stream behind every stream in `alts`.
// A launch that is already split into LDS classes is not cut again: it runs on the ctx stream, one call of `after`.
struct SlabPlan {
    std::vector<size_t> bnd;                                             // 0 = bnd[0] < .. < bnd.back() = pairs of the ctx
    std::vector<hipStream_t> alts;
    size_t next = 0;                                                     // round-robin position, carried from block to block
    std::function<int(size_t, size_t, hipStream_t)> after;
};
static int slab_join(raftx_ctx *c, hipStream_t into, const std::vector<hipStream_t> &alts) {
    for (hipStream_t s : alts) {
        HIPCHK(c, hipEventRecord(c->evJoin, s));                         // a wait captures the record that precedes it: one event serves
        HIPCHK(c, hipStreamWaitEvent(into, c->evJoin, 0));
    }
    return 0;
}
__global__ void k_iota(int n, int *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = i;
}

// ---- persistent fused launches (raftx_kernels.h: raftx_kp_f<FLAGS>)
typedef void (*kp_fn)(PersistArgs);
static kp_fn kp_kernel(int flags) {
#define X(F) if (flags == F) return raftx_kp_f##F;
    RAFTX_PERSIST128(X)
#undef X
    return nullptr;
}
#define KP_RING 64
#define KP_MAX_GRID 2048                 // workgroups of a persistent grid at most (8 per CU x 256 CUs)
static int launch_persistent(raftx_ctx *c, kp_fn kernel, const DevTables &T, const SolveArgs &A, size_t npairs, int threads, size_t lds,
                             int wg_per_cu, const GeomArgs *gen = nullptr) {
    if (!c->nCU) {
        hipDeviceProp_t pr;
        HIPCHK(c, hipGetDeviceProperties(&pr, c->device));
        c->nCU = pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 256;
    }
    HIPCHK(c, c->kpCtr.zeroed_once((size_t)KP_RING * 9 * KP_CTR_STRIDE, c->stream));   // once: every launch leaves its set zeroed (kp_leave)
    if (lds > 64 * 1024)
        HIPCHK(c, hipFuncSetAttribute(gen ? reinterpret_cast<const void *>(raftx_kpg_f0) : reinterpret_cast<const void *>(kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    PersistArgs P;
    P.T = T;
    P.A = A;
    P.ctr = c->kpCtr.p + (size_t)(c->kpNext++ % KP_RING) * 9 * KP_CTR_STRIDE;   // (a set is reused KP_RING launches of this ctx later)
    P.xl_base = XL_SLOTS;
    static const int grid_env = getenv("RAFTX_KP_GRID") ? atoi(getenv("RAFTX_KP_GRID")) : 0;      // tuning: workgroups of the grid
    size_t grid = (size_t)(grid_env > 0 ? grid_env : wg_per_cu * c->nCU);
    grid = std::min<size_t>(std::min<size_t>(grid, KP_MAX_GRID), grid_for_pairs(npairs));
    c->last_persist = 1;
    c->last_grid = (int)grid;
    c->last_pairs = (int)npairs;
    if (gen) {                                            // the generating form: the workgroups build their designs' tables first
        PersistGenArgs PG;
        PG.P = P;
        PG.G = *gen;
        hipLaunchKernelGGL(raftx_kpg_f0, dim3((unsigned)grid), dim3(threads), lds, c->stream, PG);
        return 0;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(threads), lds, c->stream, P);
    return 0;
}

// ---- the fused fixed point: kernel table, launch plan, scratch that grows, launch forms
// The instantiations of k_solve_dynamics<NB, FLAGS, MAXT, MINB>: for every shape the full-featured <NB, KF_ALL, MAXT, 1>
// (trades occupancy for registers) and the lean <NB, 0, MAXT, MINB>; the 200-bin shape has a lean kernel per feature set
// of this list as well (smallest first: a call takes the first one that covers what it needs).
#define RAFTX_LEAN128(X) X(0) X(KF_FDEP) X(KF_MCF) X(KF_MULTI) X(KF_FDEP | KF_EXTRA) X(KF_FDEP | KF_MCF) X(KF_FDEP | KF_MULTI) \
    X(KF_MCF | KF_MULTI) X(KF_FDEP | KF_EXTRA | KF_MULTI) X(KF_FDEP | KF_MCF | KF_MULTI) X(KF_OUTF) X(KF_OUTF | KF_MULTI)
struct SolveKernel {
    void (*fn)(DevTables, SolveArgs);
    int minb;                            // waves per SIMD it is compiled for
    kp_fn kp;                            // its persistent twin raftx_kp_f<FLAGS> (nullptr: none)
};
// the kernel of (shape, lean flags or KF_ALL); false: not instantiated
static bool solve_kernel(Shape sh, int flags, SolveKernel *out) {
#define ENTRY_(NB_, FL_, MT_, MB_)                                                                                      \
    {                                                                                                                   \
        *out = {k_solve_dynamics<NB_, FL_, MT_, MB_>, MB_,                                                              \
                (NB_ == 2 && MT_ == 128 && MB_ == MINB_2X128) ? kp_kernel(FL_) : nullptr};                              \
        return true;                                                                                                    \
    }
#define LEAN_(F) if (flags == (F)) ENTRY_(2, (F), 128, MINB_2X128)
#define X(NB_, MT_, MB_)                                                                                                \
    if (sh.nb == NB_ && sh.threads == MT_) {                                                                            \
        if (flags == KF_ALL) ENTRY_(NB_, KF_ALL, MT_, 1)                                                                \
        if constexpr (NB_ == 2 && MT_ == 128) { RAFTX_LEAN128(LEAN_) }                                                  \
        else if (flags == 0) ENTRY_(NB_, 0, MT_, MB_)                                                                   \
        return false;                                                                                                   \
    }
    SHAPES(X)
#undef X
#undef LEAN_
#undef ENTRY_
    return false;
}

// what one call of solve_enqueue launches with (make_plan)
struct LaunchPlan {
    Shape sh;
    int nw;
    bool xlg;                            // XiLast in a global scratch slab (raftx_kernels.h XlStore)
    bool rc_shape;                       // the shape whose spare LDS is a run-start cache (RC of k_solve_dynamics)
    int lean;                            // flags of the lean specialisation that runs; -1: the full-featured kernel
    SolveKernel k;                       // k.kp is null unless a launch of the whole batch goes out in the persistent form
    int wg_per_cu;                       // pairs per CU the LDS is budgeted for
    bool persist;
    // dynamic LDS of a workgroup whose largest design has S strips, with rc_n slots of run-start cache
    size_t lds(int S, int rc_n) const {
        return lds_bytes(S, xlg ? 0 : nw, sh.threads / 64, stage_policy(sh.nb, sh.threads), park_policy(sh.nb, sh.threads), rc_n,
                         rc_shape ? nw : 0);
    }
    // Workgroups a CU can hold by registers (the shape's waves per SIMD); LDS beyond what that residency needs goes to
    // the run-start cache (raftx_kernels.h Kin): as many 16-byte-per-bin slots as fit without costing a resident pair.
    int rc_slots(int S) const {
        if (!rc_shape) return 0;
        const int cap = 24;
        const size_t base = lds(S, 0);
        const size_t budget = LDS_LIMIT / (size_t)wg_per_cu - (persist ? KP_STASH * sizeof(double) : 0);
        if (budget <= base) return 0;
        return (int)std::min<size_t>((size_t)cap, (budget - base) / (16 * (size_t)xl_row(nw)));
    }
};
static int make_plan(raftx_ctx *c, SolveArgs *A, LaunchPlan *lp) {
    const DevTables &T = c->T;
    // the lean specialisation (no optional inputs / outputs) is the sweep path
    int need = (T.MBw ? KF_FDEP : 0) | (A->Z ? KF_OUTZ : 0) | (A->F_wave ? KF_OUTF : 0) | (A->F_extra ? KF_EXTRA : 0) |
               (T.cm ? KF_MCF : 0) | (T.nHead > 1 ? KF_MULTI : 0);
    if (c->have_xl0 || c->want_xlout) need |= KF_XLIO;
    const Shape sh = lp->sh = pick_shape(T.nw);
    lp->nw = T.nw;
    lp->xlg = xl_global(sh.nb, sh.threads);
    lp->rc_shape = sh.threads == 128 && sh.nb == 2;
    // Which specialisation runs.  The 200-bin shape has lean kernels (two waves per SIMD, no Z / F_wave / restart I/O)
    // for the feature sets a sweep meets -- several headings, MacCamy-Fuchs columns, frequency-dependent M / B (turbine
    // aerodynamics, potential-flow coefficients), a resident extra excitation (BEM, second-order) -- and takes the
    // smallest one that covers what this call needs; everything else (the drop-in's optional outputs) is the
    // full-featured kernel at one wave per SIMD.
    int lean = -1;
    if (lp->rc_shape) {
#define X(F) if (lean < 0 && (need & ~(F)) == 0) lean = (F);
        RAFTX_LEAN128(X)
#undef X
    } else if (need == 0) {
        lean = 0;
    }
    static const char *force_all = getenv("RAFTX_FORCE_ALL");           // tuning / tests: always the full-featured kernel
    if (force_all && atoi(force_all)) lean = -1;
    lp->lean = lean;
    if (!solve_kernel(sh, lean >= 0 ? lean : KF_ALL, &lp->k)) NO_KERNEL(c, sh);
    c->last_flags = lean >= 0 ? lean : KF_ALL;
    c->last_minb = lp->k.minb;
    lp->wg_per_cu = std::max(1, lp->k.minb * 4 / (sh.threads / 64));
    // the persistent form (raftx_kernels.h k_solve_dynamics_p / raftx_kp_f*): lean 200-bin launches of one LDS class that
    // are not cut into slabs; RAFTX_PERSIST=0 keeps the one-workgroup-per-pair launches (A/B, tuning)
    static const bool persist_env = !(getenv("RAFTX_PERSIST") && !atoi(getenv("RAFTX_PERSIST")));
    lp->persist = persist_env && lp->rc_shape && lean >= 0 && lp->xlg;
    if (!lp->persist) lp->k.kp = nullptr;
    A->rc_n = c->last_rc = lp->rc_slots(c->maxS);
    return 0;
}

// XiLast scratch of the shapes of xl_global(): a slot per RUNNING workgroup (xl_slot_acquire), not per pair; the slot
// bits are cleared once -- every workgroup returns its slot
static int ensure_xl_scratch(raftx_ctx *c, const LaunchPlan &lp) {
    if (!lp.xlg) return 0;
    const size_t xl_regions = XL_SLOTS + KP_MAX_GRID;      // the slot pool + one region per workgroup of a persistent grid
    const size_t want = xl_regions * 12 * (size_t)lp.nw;
    // (the whole device: fused kernels of the other streams may hold slots of the old slab)
    if (grow_device(c, c->rXl, want, DRAIN_DEVICE)) return -2;
    HIPCHK(c, c->rXlSlots.zeroed_once((size_t)XL_POOLS * XL_POOL_WORDS, c->stream));   // ahead of this ctx's launches, in stream order
    return 0;
}
// the restart point and the exported linearisation point, [npair,6,nw] each: both or neither
static int ensure_xlio(raftx_ctx *c, size_t nxl) {
    int rc = grow_device(c, c->rXl0, nxl, DRAIN_STREAM, FIT_EXACT);   // (their count is the batch shape: a smaller nxl replaces them too)
    if (!rc) rc = grow_device(c, c->rXlOut, nxl, DRAIN_STREAM, FIT_EXACT);
    if (rc) {
        c->rXl0.release();
        c->rXlOut.release();
    }
    return rc;
}

// LDS classes: the workgroups of a launch all get the LDS of its largest design, and the number of pairs a CU holds
// (4 at C3) falls with it -- one 140-strip candidate would cost a whole 10 k-design sweep a quarter of its
// residency.  Designs are therefore grouped by how many of their pairs fit a CU, one launch per group (largest
// residency first), through a pair list; a batch of one class (the usual case) is one launch without a list.
struct LdsClasses {
    struct Class {
        size_t npairs;                   // consecutive in pairList, in the order of `cls`
        int S;                           // strips of its largest design
    };
    std::vector<Class> cls;              // in launch order; empty: the batch is of one class
    std::vector<int> pairs;              // host copy of pairList (what its upload reads)
};
static int lds_classes(raftx_ctx *c, const LaunchPlan &lp, LdsClasses *out) {
    const DevTables &T = c->T;
    if ((int)c->hS.size() != T.nDesign) return 0;
    auto fit = [&](int S_) { return std::min(lp.wg_per_cu, (int)(LDS_LIMIT / lp.lds(S_, 0))); };   // pairs a CU holds
    std::vector<int> k_of((size_t)T.nDesign);
    bool mixed = false;
    for (int d = 0; d < T.nDesign; d++) mixed |= (k_of[(size_t)d] = fit(c->hS[(size_t)d])) != k_of[0];
    if (!mixed) return 0;
    if (grow_device(c, c->pairList, c->r_npair)) return -2;
    out->pairs.reserve((size_t)T.nDesign * T.nCase);       // (no reallocation under the uploads)
    for (int kk = fit(0); kk >= 0; kk--) {
        LdsClasses::Class k = {0, 0};
        const size_t at = out->pairs.size();
        for (int d = 0; d < T.nDesign; d++) {
            if (k_of[(size_t)d] != kk) continue;
            for (int ic = 0; ic < T.nCase; ic++) out->pairs.push_back(d * T.nCase + ic);
            k.S = std::max(k.S, c->hS[(size_t)d]);
        }
        if (!(k.npairs = out->pairs.size() - at)) continue;
        H2D(c, c->pairList.p + at, out->pairs.data() + at, k.npairs * sizeof(int));
        out->cls.push_back(k);
    }
    return 0;
}
// what a launch in slabs needs: the identity pair list and the fork / join events
static int ensure_slab_list(raftx_ctx *c) {
    if (!c->identList.holds(c->r_npair)) {
        if (grow_device(c, c->identList, c->r_npair)) return -2;
        hipLaunchKernelGGL(k_iota, dim3((unsigned)((c->r_npair + 255) / 256)), dim3(256), 0, c->stream, (int)c->r_npair, c->identList.p);
    }
    HIPCHK(c, c->evFork.ensure(hipEventDisableTiming));
    HIPCHK(c, c->evJoin.ensure(hipEventDisableTiming));
    return 0;
}
// A generation deferred to this launch (build_phase2): the generating form of the plain persistent kernel builds every
// design's tables in the workgroup that solves it -- if this launch is one (`whole`: one grid, and every design claimed
// exactly once); otherwise the generation kernels go first, here.  True: the launch has to generate.
static bool resolve_generation(raftx_ctx *c, const LaunchPlan &lp, bool whole) {
    BuildJob &J = c->job;
    const DevTables &T = c->T;
    if (!J.gen_deferred) return false;
    J.gen_deferred = false;
    const bool fused = whole && lp.k.kp && lp.lean == 0 && T.nCase == 1 && c->r_npair == (size_t)T.nDesign && c->r_npair > 0 &&
                       J.nDesign == T.nDesign && J.gen_lds + KP_STASH * sizeof(double) <= LDS_LIMIT / (size_t)lp.wg_per_cu;
    if (!fused) {
        J.A.addup_in_design = 0;
        launch_design(c, c->stream);
        hipLaunchKernelGGL(k_geom_addup, dim3((unsigned)(((size_t)J.nDesign * 36 + 255) / 256)), dim3(256), 0, c->stream, J.A);
    }
    return fused;
}

// the three forms of the launch: every pair in one grid on the ctx stream (persistent where the kernel has a twin) ...
static int launch_whole(raftx_ctx *c, const LaunchPlan &lp, const SolveArgs &A, size_t lds, bool gen_fused) {
    if (!c->r_npair) return 0;
    c->last_grid = (int)grid_for_pairs(c->r_npair);       // (launch_persistent records its own)
    if (lp.k.kp)
        return launch_persistent(c, lp.k.kp, c->T, A, c->r_npair, lp.sh.threads,
                                 std::max(lds, gen_fused ? c->job.gen_lds : (size_t)0) + KP_STASH * sizeof(double), lp.wg_per_cu,
                                 gen_fused ? &c->job.A : nullptr);
    hipLaunchKernelGGL(lp.k.fn, dim3(grid_for_pairs(c->r_npair)), dim3(lp.sh.threads), lds, c->stream, c->T, A);
    return 0;
}
// ... the slabs of `plan` on its side streams, each followed by plan->after (*rc_after: what that returned) ...
static int launch_slabs(raftx_ctx *c, const LaunchPlan &lp, SolveArgs A, size_t lds, SlabPlan *plan, int *rc_after) {
    HIPCHK(c, hipEventRecord(c->evFork, c->stream));       // the tables and the iota list are on the ctx stream
    for (size_t k = 0; k < plan->alts.size() && k + 1 < plan->bnd.size(); k++)
        HIPCHK(c, hipStreamWaitEvent(plan->alts[(plan->next + k) % plan->alts.size()], c->evFork, 0));
    for (size_t k = 0; k + 1 < plan->bnd.size() && !*rc_after; k++) {
        hipStream_t s = plan->alts[plan->next++ % plan->alts.size()];
        A.pairs = c->identList.p + plan->bnd[k];
        A.npairs = (int)(plan->bnd[k + 1] - plan->bnd[k]);
        hipLaunchKernelGGL(lp.k.fn, dim3(grid_for_pairs((size_t)A.npairs)), dim3(lp.sh.threads), lds, s, c->T, A);
        if (plan->after) *rc_after = plan->after(plan->bnd[k], plan->bnd[k + 1], s);
    }
    return 0;
}
// ... or one grid per LDS class on the ctx stream, each with the LDS and the cache slots of its own largest design
static void launch_classes(raftx_ctx *c, const LaunchPlan &lp, SolveArgs A, const LdsClasses &classes) {
    size_t at = 0;
    for (const LdsClasses::Class &k : classes.cls) {
        A.pairs = c->pairList.p + at;
        A.npairs = (int)k.npairs;
        at += k.npairs;
        A.rc_n = lp.rc_slots(k.S);
        hipLaunchKernelGGL(lp.k.fn, dim3(grid_for_pairs(k.npairs)), dim3(lp.sh.threads), lp.lds(k.S, A.rc_n), c->stream, c->T, A);
    }
}

// the arguments of the fused kernel that do not depend on the launch plan; sizes the result buffers, uploads F_extra
static int fill_solve_args(raftx_ctx *c, int nIter, double tol, double XiStart, const raftx_c128 *F_extra, int want_mask, SolveArgs *out) {
    if (check_ready(c)) return -1;
    if (nIter < 0) FAIL(c, "solve_dynamics: nIter < 0");
    HIPCHK(c, hipSetDevice(c->device));
    if (ensure_results(c, want_mask, F_extra != nullptr)) return -1;
    SolveArgs &A = *out;
    A.nIter = nIter + 1;
    A.tol = tol;
    A.XiStart = XiStart;
    A.F_extra = F_extra ? c->rFe : (c->bem_ready ? c->bemF.p : nullptr);
    A.Xi = c->rXi;
    A.niter = c->rNi;
    A.flags = c->rFl;
    A.B_drag = (want_mask & RAFTX_WANT_BDRAG) ? c->rB : nullptr;
    A.F_wave = (want_mask & RAFTX_WANT_FWAVE) ? c->rFw : nullptr;
    A.Z = (want_mask & RAFTX_WANT_Z) ? c->rZ : nullptr;
    c->r_last_mask = want_mask;          // buffers of a wider earlier request stay allocated (ensure_results) but are NOT rewritten
    A.pairs = nullptr;
    A.npairs = 0;
    A.Xl0 = nullptr;
    A.XlOut = nullptr;
    A.dbg = nullptr;
#ifdef RAFTX_PHASE_TIMING
    const size_t ndbg = 10 + 2 * PT_CLOCK_BUCKETS;
    HIPCHK(c, c->dbg.zeroed_once(ndbg, c->stream));
    HIPCHK(c, hipMemsetAsync(c->dbg.p, 0, ndbg * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(c->dbg.p + 8, 0xFF, sizeof(unsigned long long), c->stream));      // earliest start: a minimum
    A.dbg = c->dbg.p;
#endif
    if (F_extra && c->r_nx) H2D(c, c->rFe, F_extra, c->r_nx * sizeof(cplx));
    return 0;
}

// enqueues the fused fixed point on the ctx stream between ev0 and ev1; does not wait for it
static int solve_enqueue(raftx_ctx *c, int nIter, double tol, double XiStart, const raftx_c128 *F_extra, int want_mask,
                         SlabPlan *plan = nullptr) {
    SolveArgs A;
    if (int rc = fill_solve_args(c, nIter, tol, XiStart, F_extra, want_mask, &A)) return rc;
    LaunchPlan lp;
    if (int rc = make_plan(c, &A, &lp)) return rc;
    const size_t lds = lp.lds(c->maxS, A.rc_n);
    if (int rc = ensure_xl_scratch(c, lp)) return rc;
    A.Xl = c->rXl.p;
    A.slots = c->rXlSlots.p;
    if (c->have_xl0 || c->want_xlout) {       // restart / export of the linearisation point (the re-entry of raft_model.py:1108-1131)
        const size_t nxl = c->r_npair * 6 * (size_t)c->T.nw;
        if (c->have_xl0 && c->rXl0.n != nxl) FAIL(c, "solve_dynamics: the linearisation point was set for a different batch shape");
        if (int rc = ensure_xlio(c, nxl)) return rc;
        if (c->have_xl0) A.Xl0 = c->rXl0.p;
        A.XlOut = c->rXlOut.p;
        c->have_xl0 = false;                  // one-shot
    }
    LdsClasses classes;
    if (int rc = lds_classes(c, lp, &classes)) return rc;
    const bool slabbed = plan && classes.cls.empty() && !plan->alts.empty() && plan->bnd.size() >= 2 && plan->bnd.back() == c->r_npair;
    if (int rc = slabbed ? ensure_slab_list(c) : 0) return rc;
    const bool whole = classes.cls.empty() && !slabbed;
    const bool gen_fused = c->last_gen_fused = resolve_generation(c, lp, whole);
    c->last_persist = 0;                      // class and slabbed launches: per-pair grids, none recorded
    c->last_grid = 0;
    c->last_pairs = (int)c->r_npair;
    if (prep_lds(c, reinterpret_cast<const void *>(lp.k.fn), lds)) return -1;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    int rc_after = 0;
    if (whole && launch_whole(c, lp, A, lds, gen_fused)) return -1;
    if (slabbed && launch_slabs(c, lp, A, lds, plan, &rc_after)) return -2;
    if (!classes.cls.empty()) launch_classes(c, lp, A, classes);
    if (plan && plan->after && !slabbed) rc_after = plan->after(0, c->r_npair, c->stream);
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipGetLastError());
    if (rc_after) FAIL(c, "solve_dynamics: what follows a slab of the launch could not be enqueued");
    return 0;
}
static int finish_enqueued(raftx_ctx *c) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->last_ms = ms;
    return 0;
}
extern "C" int raftx_solve_dynamics_device(raftx_ctx *c, int nIter, double tol, double XiStart,
                                           const raftx_c128 *F_extra, int want_mask) {
    RangeScope range_("raftx_solve_dynamics_device: fused fixed point");
    const int rc = solve_enqueue(c, nIter, tol, XiStart, F_extra, want_mask);
    if (rc) return rc;
    return finish_enqueued(c);
}

extern "C" int raftx_set_linearisation_point(raftx_ctx *c, const raftx_c128 *XiLast0, int keep_last) {
    if (!c) return -1;
    if (check_ready(c)) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    c->want_xlout = keep_last != 0;
    c->have_xl0 = false;
    if (XiLast0) {
        const DevTables &T = c->T;
        const size_t nxl = (size_t)T.nDesign * T.nCase * 6 * T.nw;
        if (int rc = ensure_xlio(c, nxl)) return rc;
        if (nxl) H2D(c, c->rXl0.p, XiLast0, nxl * sizeof(cplx));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->have_xl0 = true;
    }
    return 0;
}

extern "C" int raftx_fetch_linearisation_point(raftx_ctx *c, raftx_c128 *XiLast) {
    if (!c) return -1;
    if (!c->rXlOut.p || !XiLast) FAIL(c, "fetch_linearisation_point: nothing kept (call raftx_set_linearisation_point(ctx, ., 1) first)");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->rXlOut.n) D2H(c, XiLast, c->rXlOut.p, c->rXlOut.n * sizeof(cplx));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int raftx_fetch_results(raftx_ctx *c, raftx_c128 *Xi, int32_t *niter, int32_t *flags, double *B_drag,
                                   raftx_c128 *F_wave, raftx_c128 *Z) {
    RangeScope range_("raftx_fetch_results: D2H");
    if (!c) return -1;
    if (!c->rXi) FAIL(c, "fetch_results: no resident results");
    HIPCHK(c, hipSetDevice(c->device));
    // (kept = written by the LAST solve: a buffer left over from a wider earlier request holds that request's results)
    if (B_drag && !(c->rB && (c->r_last_mask & RAFTX_WANT_BDRAG))) FAIL(c, "fetch_results: B_drag was not kept");
    if (F_wave && !(c->rFw && (c->r_last_mask & RAFTX_WANT_FWAVE))) FAIL(c, "fetch_results: F_wave was not kept");
    if (Z && !(c->rZ && (c->r_last_mask & RAFTX_WANT_Z))) FAIL(c, "fetch_results: Z was not kept");
    if (Xi && c->r_nx) D2H(c, Xi, c->rXi, c->r_nx * sizeof(cplx));
    if (niter && c->r_npair) D2H(c, niter, c->rNi, c->r_npair * sizeof(int));
    if (flags && c->r_npair) D2H(c, flags, c->rFl, c->r_npair * sizeof(int));
    if (B_drag && c->r_npair) D2H(c, B_drag, c->rB, c->r_npair * 36 * sizeof(double));
    if (F_wave && c->r_nx) D2H(c, F_wave, c->rFw, c->r_nx * sizeof(cplx));
    if (Z && c->r_nz) D2H(c, Z, c->rZ, c->r_nz * sizeof(cplx));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int raftx_solve_dynamics(raftx_ctx *c, int nIter, double tol, double XiStart, const raftx_c128 *F_extra,
                                    raftx_c128 *Xi, int32_t *niter, int32_t *flags, double *B_drag,
                                    raftx_c128 *F_wave, raftx_c128 *Z) {
    int mask = (B_drag ? RAFTX_WANT_BDRAG : 0) | (F_wave ? RAFTX_WANT_FWAVE : 0) | (Z ? RAFTX_WANT_Z : 0);
    int rc = raftx_solve_dynamics_device(c, nIter, tol, XiStart, F_extra, mask);
    if (rc) return rc;
    return raftx_fetch_results(c, Xi, niter, flags, B_drag, F_wave, Z);
}

extern "C" int raftx_bem_excitation(raftx_ctx *c, int nHeadBEM, const double *headings_deg, const raftx_c128 *X_BEM,
                                    const double *heading_adjust, const double *xy_ref, const raftx_c128 *F_add,
                                    raftx_c128 *F_out) {
    if (check_ready(c)) return -1;
    if (nHeadBEM < 1 || !headings_deg || !X_BEM) FAIL(c, "bem_excitation: bad arguments");
    for (int i = 0; i < nHeadBEM; i++)
        if (!(headings_deg[i] >= 0.0 && headings_deg[i] < 360.0) || (i && !(headings_deg[i] > headings_deg[i - 1])))
            FAIL(c, "bem_excitation: headings must be ascending in [0, 360)");
    HIPCHK(c, hipSetDevice(c->device));
    const DevTables &T = c->T;
    const size_t npair = (size_t)T.nDesign * T.nCase, nx = npair * T.nHead * 6 * T.nw;
    const size_t nX = (size_t)T.nDesign * nHeadBEM * 6 * T.nw;
    c->bem_ready = false;
    if (grow_device(c, c->bemF, nx)) return -2;
    Scratch sc(c);
    double *dH = sc.in<double>(headings_deg, nHeadBEM);
    cplx *dX = sc.in<cplx>(X_BEM, nX);
    double *dA = sc.in<double>(heading_adjust, T.nDesign), *dXY = sc.in<double>(xy_ref, (size_t)T.nDesign * 2);
    cplx *dAdd = sc.in<cplx>(F_add, nx);
    sc.out_from(F_out, c->bemF.p, nx);
    if (int rc = sc.upload("bem_excitation")) return rc;
    if (sc.begin()) return -2;
    if (nx)
        hipLaunchKernelGGL(k_bem_excitation, dim3((unsigned)(npair * T.nHead)), bin_threads(T.nw), 0, c->stream, T, nHeadBEM, dH, dX, dA,
                           dXY, dAdd, c->bemF.p);
    if (int rc = sc.finish()) return rc;
    c->bem_ready = true;
    return 0;
}

extern "C" int raftx_motion_stats(raftx_ctx *c, double dw, double *sd, double *psd) {
    if (!c) return -1;
    if (!c->rXi) FAIL(c, "motion_stats: no resident results");
    if (!sd) FAIL(c, "motion_stats: std is NULL");
    if (!(dw > 0.0)) FAIL(c, "motion_stats: dw must be positive");
    HIPCHK(c, hipSetDevice(c->device));
    const DevTables &T = c->T;
    const size_t npair = c->r_npair;
    Scratch sc(c);
    double *dS = sc.out<double>(sd, npair * 6), *dP = sc.out<double>(psd, npair * 6 * T.nw);
    if (int rc = sc.upload("motion_stats")) return rc;
    if (sc.begin()) return -2;
    if (npair)
        hipLaunchKernelGGL(k_motion_stats, dim3((unsigned)npair), bin_threads(T.nw), 0, c->stream, (int)npair, T.nHead, T.nw, 1.0 / dw,
                           c->rXi, dS, dP);
    return sc.finish();
}

extern "C" int raftx_channel_stats(raftx_ctx *c, int nChan, const double *L, const int32_t *pw, double dw, double *sd,
                                   double *psd) {
    if (!c) return -1;
    if (!c->rXi) FAIL(c, "channel_stats: no resident results");
    if (nChan < 0 || (nChan && (!L || !pw)) || !sd) FAIL(c, "channel_stats: bad arguments");
    if (!(dw > 0.0)) FAIL(c, "channel_stats: dw must be positive");
    for (int i = 0; i < nChan; i++)
        if (pw[i] < 0 || pw[i] > 4) FAIL(c, "channel_stats: pow[%d]=%d outside 0..4", i, pw[i]);
    HIPCHK(c, hipSetDevice(c->device));
    const DevTables &T = c->T;
    const size_t npair = c->r_npair;
    Scratch sc(c);
    double *dL = sc.in<double>(L, (size_t)T.nDesign * nChan * 6);
    int *dP = sc.in<int>(pw, nChan);
    double *dS = sc.out<double>(sd, npair * nChan), *dPsd = sc.out<double>(psd, npair * nChan * T.nw);
    if (int rc = sc.upload("channel_stats")) return rc;
    if (sc.begin()) return -2;
    if (npair && nChan)
        hipLaunchKernelGGL(k_channel_stats, dim3((unsigned)npair), bin_threads(T.nw), 0, c->stream, T.nCase, T.nHead, T.nw, nChan,
                           1.0 / dw, T.w, c->rXi, dL, dP, dS, dPsd);
    return sc.finish();
}

extern "C" int raftx_channel_stats_poly(raftx_ctx *c, int nChan, const double *L, const raftx_c128 *Gw, double dw, double *sd,
                                        double *psd) {
    if (!c) return -1;
    if (!c->rXi) FAIL(c, "channel_stats_poly: no resident results");
    if (nChan < 0 || (nChan && !L) || !sd) FAIL(c, "channel_stats_poly: bad arguments");
    if (!(dw > 0.0)) FAIL(c, "channel_stats_poly: dw must be positive");
    HIPCHK(c, hipSetDevice(c->device));
    const DevTables &T = c->T;
    const size_t npair = c->r_npair;
    Scratch sc(c);
    double *dL = sc.in<double>(L, (size_t)T.nDesign * nChan * 18);
    cplx *dG = sc.in<cplx>(Gw, (size_t)T.nDesign * nChan * 6 * T.nw);
    double *dS = sc.out<double>(sd, npair * nChan), *dPsd = sc.out<double>(psd, npair * nChan * T.nw);
    if (int rc = sc.upload("channel_stats_poly")) return rc;
    if (sc.begin()) return -2;
    if (npair && nChan)
        hipLaunchKernelGGL(k_channel_stats_poly, dim3((unsigned)npair), bin_threads(T.nw), 0, c->stream, T.nCase, T.nHead, T.nw, nChan,
                           1.0 / dw, T.w, c->rXi, dL, dG, dS, dPsd);
    return sc.finish();
}

extern "C" int raftx_response_stats(raftx_ctx *c, int nChan, int nDof, int nResp, int nw, const double *w, const double *L,
                                    const raftx_c128 *Gw, const raftx_c128 *Xi, double dw, double *sd, double *psd) {
    RangeScope range_("raftx_response_stats: linear channels of a caller-held response");
    if (!c) return -1;
    if (nChan < 0 || nDof < 1 || nResp < 1 || nw < 1 || !w || (nChan && !L) || !Xi || !sd) FAIL(c, "response_stats: bad arguments");
    if (!(dw > 0.0)) FAIL(c, "response_stats: dw must be positive");
    if (!nChan) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    double *dw_ = sc.in<double>(w, nw), *dL = sc.in<double>(L, (size_t)nChan * 3 * nDof);
    cplx *dG = sc.in<cplx>(Gw, (size_t)nChan * nDof * nw), *dX = sc.in<cplx>(Xi, (size_t)nResp * nDof * nw);
    double *dS = sc.out<double>(sd, nChan), *dP = sc.out<double>(psd, (size_t)nChan * nw);
    if (int rc = sc.upload("response_stats")) return rc;
    if (sc.begin()) return -2;
    hipLaunchKernelGGL(k_response_stats, dim3((unsigned)nChan), bin_threads(nw), 0, c->stream, nDof, nResp, nw, 1.0 / dw, dw_, dX, dL, dG,
                       dS, dP);
    return sc.finish();
}

// launches the LDS-resident solver, for the shapes launch_solve_system_rows has no kernel for (callers have checked that
// the shape fits: solve_system_shape gives at most 150 KiB)
template <bool RESIDENT>
static int launch_solve_system_lds(raftx_ctx *c, int nSys, int nUnit, int nRhs, int nw, int nCase, const double *w, const cplx *Z,
                                   const double *Mc, const double *Bc, const double *Cc, const cplx *F, cplx *X) {
    size_t lds = 0;
    const int nbin = solve_system_shape(6 * nUnit, nRhs, &lds);
    if (lds > 64 * 1024)
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_solve_system<RESIDENT>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_solve_system<RESIDENT>, dim3((unsigned)((size_t)nSys * ((nw + nbin - 1) / nbin))), dim3(64 * nbin), lds,
                       c->stream, nSys, nUnit, nRhs, nw, nCase, w, Z, Mc, Bc, Cc, F, X);
    return 0;
}

extern "C" int raftx_solve_system(raftx_ctx *c, int nSys, int nUnit, int nRhs, int nw, const double *w,
                                  const raftx_c128 *Zblk, const double *Mc, const double *Bc, const double *Cc,
                                  const raftx_c128 *F, raftx_c128 *Xi) {
    if (!c) return -1;
    if (nSys < 0 || nUnit < 1 || nRhs < 1 || nw < 1 || !w || !Zblk || !F || !Xi) FAIL(c, "solve_system: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const int n = 6 * nUnit;
    size_t lds = 0;
    solve_system_shape(n, nRhs, &lds);
    if (lds > 150 * 1024) FAIL(c, "solve_system: %d DOFs x %d rhs does not fit the LDS-resident solver", n, nRhs);
    Scratch sc(c);
    const size_t nf = (size_t)nSys * nRhs * n * nw, nc = (size_t)nSys * n * n;
    double *dw = sc.in<double>(w, nw);
    cplx *dZ = sc.in<cplx>(Zblk, (size_t)nSys * nUnit * 36 * nw), *dF = sc.in<cplx>(F, nf);
    double *dM = sc.in<double>(Mc, nc), *dB = sc.in<double>(Bc, nc), *dC = sc.in<double>(Cc, nc);
    cplx *dX = sc.out<cplx>(Xi, nf);
    if (int rc = sc.upload("solve_system")) return rc;
    if (sc.begin()) return -2;
    if (nSys && !launch_solve_system_rows<false>(c->stream, nSys, nUnit, nRhs, nw, 1, dw, dZ, dM, dB, dC, dF, dX))
        if (int rc = launch_solve_system_lds<false>(c, nSys, nUnit, nRhs, nw, 1, dw, dZ, dM, dB, dC, dF, dX)) return rc;
    return sc.finish();
}

// launch of the dense solves of nSys systems x nw bins on device arrays: the register-resident kernel where the augmented
// matrix fits its grid (the flexible deck: 150 + 1), the L2-workspace kernel otherwise.  Matrix set of system s: s / mdiv.
static bool dense_reg_shape(int n, int nRhs) {
    return n + nRhs <= 160;
}
// size of the L2-workspace kernel's block A, in elements: 0 where the register kernel takes the shape
static size_t dense_workspace(int nSys, int n, int nRhs, int nw) {
    return dense_reg_shape(n, nRhs) ? 0 : (size_t)nSys * nw * n * (n + nRhs);
}
struct DenseSolve {                      // one launch; optional: Badd [nSys,n,n] on top of B, active (0: system skipped), Z out
    int nSys, mdiv, n, nRhs, nw;
    const double *w, *M, *B, *C;
    int freq_mask;
    const double *Badd = nullptr;
    const int *active = nullptr;
    const cplx *F = nullptr;
    cplx *X = nullptr, *Z = nullptr, *A = nullptr;       // A: dense_workspace() elements
};
static int dense_launch(raftx_ctx *c, const DenseSolve &d) {
    const dim3 grid((unsigned)d.nw, (unsigned)d.nSys);
    if (dense_reg_shape(d.n, d.nRhs)) {
#define DENSE_REG_(RB_, CB_)                                                                                            \
        hipLaunchKernelGGL((k_solve_dense_reg2<RB_, CB_, 16>), grid, dim3(512), 0, c->stream, d.n, d.nRhs, d.nw, d.w, d.M, d.B, d.C, \
                           d.freq_mask, d.mdiv, d.Badd, d.active, d.F, d.X, d.Z)
        // entries per thread: the smallest 32 RB x 16 CB grid that holds [Z | F] (measured at 60 DOFs: 0.076 ms with 3 x 6
        // against 0.136 with 5 x 10 and 0.23 for the L2-workspace kernel)
        if (d.n + d.nRhs <= 32) DENSE_REG_(1, 2);
        else if (d.n + d.nRhs <= 64) DENSE_REG_(2, 4);
        else if (d.n + d.nRhs <= 96) DENSE_REG_(3, 6);
        else if (d.n + d.nRhs <= 128) DENSE_REG_(4, 8);
        else DENSE_REG_(5, 10);
#undef DENSE_REG_
    } else {
        hipLaunchKernelGGL(k_solve_dense, grid, dim3(256), 0, c->stream, d.n, d.nRhs, d.nw, d.w, d.M, d.B, d.C, d.freq_mask, d.mdiv, d.Badd, d.active, d.F, d.A, d.X, d.Z);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}
static int dense_check(raftx_ctx *c, const char *who, int nSys, int n, int nRhs, int nw) {
    if (nSys < 0 || n < 1 || nRhs < 1 || nw < 1) FAIL(c, "%s: bad arguments", who);
    if (n + nRhs > DENSE_MAX_LD) FAIL(c, "%s: %d DOFs + %d right-hand sides exceed %d", who, n, nRhs, DENSE_MAX_LD);
    if (nSys > 65535) FAIL(c, "%s: at most 65 535 systems per call", who);
    return 0;
}

static int solve_dense_impl(raftx_ctx *c, int nSys, int n, int nRhs, int nw, const double *w, const double *M, const double *B,
                            const double *C, int freq_mask, const raftx_c128 *F, raftx_c128 *Xi, raftx_c128 *Z) {
    if (!c) return -1;
    if (!w || !M || !B || !C || !F || !Xi) FAIL(c, "solve_dense: bad arguments");
    if (dense_check(c, "solve_dense", nSys, n, nRhs, nw)) return -1;
    if (nSys == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    const size_t nn = (size_t)n * n, nf = (size_t)nSys * nRhs * n * nw;
    DenseSolve d;
    d.nSys = nSys; d.mdiv = 1; d.n = n; d.nRhs = nRhs; d.nw = nw; d.freq_mask = freq_mask;
    d.w = sc.in<double>(w, nw); d.M = sc.in<double>(M, (size_t)nSys * nn * ((freq_mask & 1) ? nw : 1));
    d.B = sc.in<double>(B, (size_t)nSys * nn * ((freq_mask & 2) ? nw : 1)); d.C = sc.in<double>(C, (size_t)nSys * nn);
    d.F = sc.in<cplx>(F, nf); d.X = sc.out<cplx>(Xi, nf); d.Z = sc.out<cplx>(Z, (size_t)nSys * nn * nw);
    d.A = sc.tmp<cplx>(dense_workspace(nSys, n, nRhs, nw));
    if (int rc = sc.upload("solve_dense")) return rc;
    if (sc.begin()) return -2;
    if (dense_launch(c, d)) return -1;
    return sc.finish();
}
extern "C" int raftx_solve_dense(raftx_ctx *c, int n, int nRhs, int nw, const double *w, const double *M, const double *B,
                                 const double *C, int freq_mask, const raftx_c128 *F, raftx_c128 *Xi, raftx_c128 *Z) {
    return solve_dense_impl(c, 1, n, nRhs, nw, w, M, B, C, freq_mask, F, Xi, Z);
}
extern "C" int raftx_solve_dense_batch(raftx_ctx *c, int nSys, int n, int nRhs, int nw, const double *w, const double *M,
                                       const double *B, const double *C, int freq_mask, const raftx_c128 *F, raftx_c128 *Xi,
                                       raftx_c128 *Z) {
    return solve_dense_impl(c, nSys, n, nRhs, nw, w, M, B, C, freq_mask, F, Xi, Z);
}

// The matrices of a fixed point stay on the device: M, B, C of nSet units are uploaded once (raftx_dense_resident); every
// iteration then sends what CHANGES -- the drag linearisation Badd [n,n] of each (unit, sea state) and the right-hand sides --
// and gets the responses back (raftx_solve_dense_resident).  With frequency-dependent rotor matrices the flexible deck's M and
// B are 7.2 MB each: re-uploaded by every raftx_solve_dense call they were most of the call.
extern "C" int raftx_dense_resident(raftx_ctx *c, int nSet, int n, int nw, const double *w, const double *M, const double *B,
                                    const double *C, int freq_mask) {
    if (!c) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    DenseResident &R = c->dense;
    R = DenseResident();                              // (move assignment: the old matrices' bag gives its blocks back first)
    if (nSet == 0) return 0;                                              // (release)
    if (!w || !M || !B || !C) FAIL(c, "dense_resident: bad arguments");
    if (dense_check(c, "dense_resident", nSet, n, 1, nw)) return -1;
    const size_t nn = (size_t)n * n, nM = (size_t)nSet * nn * ((freq_mask & 1) ? nw : 1), nB = (size_t)nSet * nn * ((freq_mask & 2) ? nw : 1);
    if (pool_alloc(c, R.allocs, (size_t)nw, &R.w) || pool_alloc(c, R.allocs, nM, &R.M) || pool_alloc(c, R.allocs, nB, &R.B) ||
        pool_alloc(c, R.allocs, (size_t)nSet * nn, &R.C))
        return -2;
    H2D(c, R.w, w, nw * sizeof(double));
    H2D(c, R.M, M, nM * sizeof(double));
    H2D(c, R.B, B, nB * sizeof(double));
    H2D(c, R.C, C, (size_t)nSet * nn * sizeof(double));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    R.nSet = nSet; R.n = n; R.nw = nw; R.freq_mask = freq_mask;
    return 0;
}
extern "C" int raftx_solve_dense_resident(raftx_ctx *c, int nPer, const double *Badd, int nRhs, const raftx_c128 *F, raftx_c128 *Xi,
                                          raftx_c128 *Z) {
    if (!c) return -1;
    const DenseResident &R = c->dense;
    if (R.nSet < 1) FAIL(c, "solve_dense_resident: no resident matrices (raftx_dense_resident first)");
    if (nPer < 1 || !F || !Xi) FAIL(c, "solve_dense_resident: bad arguments");
    const int nSys = R.nSet * nPer, n = R.n, nw = R.nw;
    if (dense_check(c, "solve_dense_resident", nSys, n, nRhs, nw)) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    const size_t nn = (size_t)n * n, nf = (size_t)nSys * nRhs * n * nw;
    DenseSolve d;
    d.nSys = nSys; d.mdiv = nPer; d.n = n; d.nRhs = nRhs; d.nw = nw; d.freq_mask = R.freq_mask;
    d.w = R.w; d.M = R.M; d.B = R.B; d.C = R.C; d.Badd = sc.in<double>(Badd, (size_t)nSys * nn);
    d.F = sc.in<cplx>(F, nf); d.X = sc.out<cplx>(Xi, nf); d.Z = sc.out<cplx>(Z, (size_t)nSys * nn * nw);
    d.A = sc.tmp<cplx>(dense_workspace(nSys, n, nRhs, nw));
    if (int rc = sc.upload("solve_dense_resident")) return rc;
    if (sc.begin()) return -2;
    if (dense_launch(c, d)) return -1;
    return sc.finish();
}

// include/raftx.h raftx_flex_start: the next raftx_flex_solve starts from this iterate (one-shot)
extern "C" int raftx_flex_start(raftx_ctx *c, int nUnit, int n, const raftx_c128 *XiLast0) {
    if (!c) return -1;
    c->flexStart.take();
    if (!XiLast0) return 0;
    if (check_ready(c)) return -1;
    const DevTables &T = c->T;
    if (nUnit < 1 || n < 6) FAIL(c, "flex_start: bad arguments (nUnit=%d, n=%d)", nUnit, n);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t need = (size_t)nUnit * T.nCase * n * T.nw;
    if (grow_device(c, c->flexStart.x, need)) return -2;
    H2D(c, c->flexStart.x.p, XiLast0, need * sizeof(cplx));
    HIPCHK(c, hipStreamSynchronize(c->stream));           // the caller's array is free again
    c->flexStart.n = need;
    return 0;
}

// The fixed point of flexible units on the device (raftx_flex.h; include/raftx.h raftx_flex_solve): the counts of a call,
// its device arrays, and its steps in the order raftx_flex_solve takes them.
struct FlexShape {
    int nUnit, nNode, nCase, nHead, nw, n, nSys, freq_mask;
    size_t nn, nxs, npn, nM, nB, nxl, nxh;               // n^2, n nw, nodes x sea states, entries of M, of B, of one iterate, of all headings
    bool started;                                         // raftx_flex_start gave the first iterate
};
struct FlexArrays {
    double *M, *B, *C, *Tn, *W, *Bn, *Bd;
    int64_t *off;
    int *nodeUnit, *act, *ni, *fl, *count, *iter;
    cplx *Flin, *XiN, *Fn, *Fw, *Fd, *rhs, *Xnew, *Xi, *Xl, *Xh, *A, *Z;
};
static DenseSolve flex_dense(const raftx_ctx *c, const FlexShape &S, const FlexArrays &A) {   // what the two solves of the fixed point share
    DenseSolve d;
    d.nSys = S.nSys; d.mdiv = S.nCase; d.n = S.n; d.nw = S.nw; d.freq_mask = S.freq_mask;
    d.w = c->T.w; d.M = A.M; d.B = A.B; d.C = A.C; d.Badd = A.Bd; d.A = A.A;
    return d;
}
// the shape of the call against the resident tables; a pending start is taken here, whether it fits or not
static int flex_check(raftx_ctx *c, int nUnit, const int64_t *nodeOff, int n, int freq_mask, FlexShape &S) {
    const DevTables &T = c->T;
    S.nUnit = nUnit; S.nNode = T.nDesign; S.nCase = T.nCase; S.nHead = T.nHead; S.nw = T.nw; S.n = n; S.nSys = nUnit * T.nCase;
    if (nodeOff[0] != 0 || nodeOff[nUnit] != S.nNode) FAIL(c, "flex_solve: nodeOff must run from 0 to the %d resident node tables", S.nNode);
    for (int u = 0; u < nUnit; u++)
        if (nodeOff[u + 1] < nodeOff[u]) FAIL(c, "flex_solve: node offsets not monotone");
    if (dense_check(c, "flex_solve", S.nSys, n, S.nHead, S.nw)) return -1;
    if (n < 6) FAIL(c, "flex_solve: n = %d reduced DOFs", n);
    if (!S.nSys || !S.nNode) FAIL(c, "flex_solve: device allocation failed");   // (no sea states, no nodes: the wording the empty blocks always had)
    S.freq_mask = freq_mask;
    S.nn = (size_t)n * n; S.nxs = (size_t)n * S.nw; S.npn = (size_t)S.nNode * S.nCase;
    S.nM = nUnit * S.nn * ((freq_mask & 1) ? S.nw : 1); S.nB = nUnit * S.nn * ((freq_mask & 2) ? S.nw : 1);
    S.nxl = S.nSys * S.nxs; S.nxh = S.nxl * S.nHead;
    const size_t had = c->flexStart.take();
    S.started = had != 0;
    if (had && had != S.nxl) FAIL(c, "flex_solve: the linearisation point of raftx_flex_start has %zu entries, this call %zu", had, S.nxl);
    return 0;
}
static int flex_reset(raftx_ctx *c, const FlexShape &S, const FlexArrays &A) {
    HIPCHK(c, hipMemsetAsync(A.ni, 0, S.nSys * sizeof(int), c->stream));
    HIPCHK(c, hipMemsetAsync(A.fl, 0, S.nSys * sizeof(int), c->stream));
    HIPCHK(c, hipMemsetAsync(A.Bd, 0, S.nSys * S.nn * sizeof(double), c->stream));
    HIPCHK(c, hipMemsetAsync(A.Xi, 0, S.nxl * sizeof(cplx), c->stream));
    HIPCHK(c, hipMemsetAsync(A.Fd, 0, S.nxh * sizeof(cplx), c->stream));
    return 0;
}
static int flex_first_iterate(raftx_ctx *c, const FlexShape &S, const FlexArrays &A, double XiStart) {
    if (S.started)
        HIPCHK(c, hipMemcpyAsync(A.Xl, c->flexStart.x.p, S.nxl * sizeof(cplx), hipMemcpyDeviceToDevice, c->stream));
    else
        hipLaunchKernelGGL(k_flex_fill, dim3((unsigned)((S.nxl + 255) / 256)), dim3(256), 0, c->stream, S.nxl, cplx{XiStart, 0.0}, A.Xl);   // :999
    return 0;
}
// one iteration: node motions -> linearisation of every (node, sea state) -> projections with the units' T -> dense solves ->
// convergence test / relaxation -> the count of pairs still iterating to the host (the ctx's page-locked area)
static int flex_iteration(raftx_ctx *c, const FlexShape &S, const FlexArrays &A, double tol) {
    const int nt = (S.n + 15) / 16;
    const dim3 gridB((unsigned)((nt * nt + 3) / 4), (unsigned)S.nSys), gridF((unsigned)((S.nxs + 255) / 256), (unsigned)(S.nSys * S.nHead));
    hipLaunchKernelGGL(k_flex_node_motion, dim3((unsigned)S.npn), dim3(256), 0, c->stream, S.nCase, S.n, S.nw, A.nodeUnit, A.Tn, A.Xl, A.XiN);
    if (linearize_enqueue(c, A.XiN, A.Bn, A.Fn, false)) return -1;
    hipLaunchKernelGGL(k_flex_w, dim3((unsigned)S.npn), dim3(256), 0, c->stream, S.nNode, S.nCase, S.n, A.Tn, A.Bn, A.W);
    hipLaunchKernelGGL(k_flex_gemm_B, gridB, dim3(256), 0, c->stream, S.nNode, S.nCase, S.n, A.off, A.Tn, A.W, A.act, A.Bd);
    hipLaunchKernelGGL(k_flex_project_F, gridF, dim3(256), 0, c->stream, S.nCase, S.nHead, S.n, S.nw, A.off, A.Tn, A.Fn, A.Flin, A.act, A.Fw, A.Fd, A.rhs);
    DenseSolve d = flex_dense(c, S, A);
    d.nRhs = 1; d.active = A.act; d.F = A.rhs; d.X = A.Xnew;
    if (dense_launch(c, d)) return -1;
    HIPCHK(c, hipMemsetAsync(A.count, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(k_flex_converge, dim3((unsigned)S.nSys), dim3(256), 0, c->stream, S.n, S.nw, tol, A.iter, A.Xnew, A.Xi, A.Xl, A.act, A.ni, A.fl, A.count);
    hipLaunchKernelGGL(k_flex_tick, dim3(1), dim3(1), 0, c->stream, A.iter);
    HIPCHK(c, hipMemcpyAsync(c->pin.p, A.count, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    return 0;
}
// The launches of an iteration are the same every time (the iteration number lives in device memory), so they can be
// captured ONCE into a hipGraph and replayed: RAFTX_FLEX_GRAPH=1.  Measured (scripts/bench_flex.py, prof_flex_dropin.py): the
// capture + instantiation of every call costs more than the four or five replays save -- 13.5 against 13.1 ms for a batch
// of 16 units x 3 sea states, 2.5-2.9 against 2.3 ms for a single unit -- so plain launches are the default (a graph kept
// across calls of one shape would pay; not built).  The first iteration always runs plainly (it sets the kernels' LDS
// attributes, which a capture must not contain); a capture or instantiation that fails leaves plain launches.
struct FlexGraph : NoCopy {              // the handles of the captured iteration, released on every path
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    ~FlexGraph() { if (exec) (void)hipGraphExecDestroy(exec); if (graph) (void)hipGraphDestroy(graph); }
};
static int flex_iterate(raftx_ctx *c, const FlexShape &S, const FlexArrays &A, int nIter, double tol) {
    static const bool use_graph = getenv("RAFTX_FLEX_GRAPH") && atoi(getenv("RAFTX_FLEX_GRAPH"));
    const volatile int *hCount = reinterpret_cast<volatile int *>(c->pin.p);
    HIPCHK(c, hipMemsetAsync(A.iter, 0, sizeof(int), c->stream));
    FlexGraph g;
    int rc = 0;
    for (int it = 0; it <= nIter && !rc; it++) {                          // :977, 1052
        if (it == 1 && use_graph && nIter > 1 && hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            const int rcq = flex_iteration(c, S, A, tol);
            const hipError_t ee = hipStreamEndCapture(c->stream, &g.graph);
            if (rcq || ee != hipSuccess || !g.graph || hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0) != hipSuccess) g.exec = nullptr;
            (void)hipGetLastError();
        }
        if (g.exec) rc = hipGraphLaunch(g.exec, c->stream) != hipSuccess ? -2 : 0;
        else rc = flex_iteration(c, S, A, tol);
        if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = -2;
        if (!rc && *hCount == 0) break;
    }
    if (rc) FAIL(c, "flex_solve: an iteration could not be enqueued (%s)", hipGetErrorString(hipGetLastError()));
    return 0;
}
// every heading with the impedance of the pair's last iteration (:1155, 1191, 1212-1216)
static int flex_all_headings(raftx_ctx *c, const FlexShape &S, const FlexArrays &A) {
    DenseSolve d = flex_dense(c, S, A);
    d.nRhs = S.nHead; d.F = A.Fw; d.X = A.Xh; d.Z = A.Z;
    return dense_launch(c, d) ? -1 : 0;
}
extern "C" int raftx_flex_solve(raftx_ctx *c, int nUnit, const int64_t *nodeOff, int n, const double *Tn, const double *M,
                                const double *B, const double *C, int freq_mask, const raftx_c128 *F_lin, int nIter, double tol,
                                double XiStart, raftx_c128 *Xi, int32_t *niter, int32_t *flags, double *B_drag, raftx_c128 *F_drag,
                                raftx_c128 *Z) {
    RangeScope range_("raftx_flex_solve: fixed point of units with flexible members");
    if (check_ready(c)) return -1;
    if (nUnit < 1 || !nodeOff || !Tn || !M || !B || !C || !F_lin || !Xi || !niter || !flags || nIter < 0)
        FAIL(c, "flex_solve: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    FlexShape S;
    if (flex_check(c, nUnit, nodeOff, n, freq_mask, S)) return -1;
    std::vector<int> hNodeUnit((size_t)S.nNode), ones((size_t)S.nSys, 1);       // (uploaded: they live until the call returns)
    for (int u = 0; u < nUnit; u++)
        for (int64_t i = nodeOff[u]; i < nodeOff[u + 1]; i++) hNodeUnit[(size_t)i] = u;
    Scratch sc(c);
    FlexArrays A;
    A.M = sc.in<double>(M, S.nM); A.B = sc.in<double>(B, S.nB); A.C = sc.in<double>(C, nUnit * S.nn);
    A.Tn = sc.in<double>(Tn, (size_t)S.nNode * 6 * n); A.off = sc.in<int64_t>(nodeOff, (size_t)nUnit + 1);
    A.nodeUnit = sc.in<int>(hNodeUnit.data(), hNodeUnit.size()); A.Flin = sc.in<cplx>(F_lin, S.nxh); A.act = sc.in<int>(ones.data(), ones.size());
    A.W = sc.tmp<double>(S.npn * 6 * n); A.Bn = sc.tmp<double>(S.npn * 36); A.Bd = sc.tmp<double>(S.nSys * S.nn);
    A.ni = sc.tmp<int>(S.nSys); A.fl = sc.tmp<int>(S.nSys); A.count = sc.tmp<int>(1); A.iter = sc.tmp<int>(1);
    A.XiN = sc.tmp<cplx>(S.npn * 6 * S.nw); A.Fn = sc.tmp<cplx>(S.npn * S.nHead * 6 * S.nw);
    A.Fw = sc.tmp<cplx>(S.nxh); A.Fd = sc.tmp<cplx>(S.nxh); A.Xh = sc.tmp<cplx>(S.nxh);
    A.rhs = sc.tmp<cplx>(S.nxl); A.Xnew = sc.tmp<cplx>(S.nxl); A.Xi = sc.tmp<cplx>(S.nxl); A.Xl = sc.tmp<cplx>(S.nxl);
    A.A = sc.tmp<cplx>(dense_workspace(S.nSys, n, S.nHead, S.nw));               // (the one-column solve of an iteration needs no more)
    A.Z = Z ? sc.tmp<cplx>(S.nSys * S.nn * S.nw) : nullptr;
    sc.out_from(Xi, A.Xh, S.nxh); sc.out_from(niter, A.ni, (size_t)S.nSys); sc.out_from(flags, A.fl, (size_t)S.nSys);   // copied in this order
    sc.out_from(B_drag, A.Bd, S.nSys * S.nn); sc.out_from(F_drag, A.Fd, S.nxh); sc.out_from(Z, A.Z, S.nSys * S.nn * S.nw);
    if (int rc = sc.upload("flex_solve")) return rc;
    HIPCHK(c, c->pin.reserve(16));
    if (int rc = flex_reset(c, S, A)) return rc;
    if (int rc = flex_first_iterate(c, S, A, XiStart)) return rc;
    if (sc.begin()) return -2;                                                  // the span of the whole fixed point
    if (int rc = flex_iterate(c, S, A, nIter, tol)) return rc;
    if (int rc = flex_all_headings(c, S, A)) return rc;
    return sc.finish();
}

extern "C" int raftx_solve_system_resident(raftx_ctx *c, int nUnit, const double *Mc, const double *Bc, const double *Cc,
                                           raftx_c128 *Xi) {
    if (!c) return -1;
    const DevTables &T = c->T;
    // what the coupled solve is fed from: the exported impedances (RAFTX_WANT_Z), or -- no Z kept -- the units' constant
    // matrices + the exported B_drag (RAFTX_WANT_BDRAG), assembled on the fly; frequency-dependent M(w), B(w) need the export
    // -- decided on what the LAST solve wrote, not on which buffers exist: a same-shape solve that asked for less keeps the
    // wider buffers of the call before it, with that call's contents
    const int lm = c->r_last_mask;
    const bool haveZ = c->rZ && (lm & RAFTX_WANT_Z), haveF = c->rFw && (lm & RAFTX_WANT_FWAVE);
    const bool assemble = c->rXi && !haveZ && c->rB && (lm & RAFTX_WANT_BDRAG) && haveF && !T.MBw;
    if (!c->rXi || !haveF || (!haveZ && !assemble))
        FAIL(c, "solve_system_resident: needs resident F_wave and either Z or (constant matrices) B_drag "
                "(raftx_solve_dynamics_device with RAFTX_WANT_FWAVE | RAFTX_WANT_Z, or RAFTX_WANT_FWAVE | RAFTX_WANT_BDRAG)");
    if (nUnit < 1 || T.nDesign % nUnit != 0 || !Xi) FAIL(c, "solve_system_resident: bad arguments (nDesign=%d, nUnit=%d)", T.nDesign, nUnit);
    HIPCHK(c, hipSetDevice(c->device));
    const int nGroup = T.nDesign / nUnit, nSys = nGroup * T.nCase, n = 6 * nUnit, nRhs = T.nHead, nw = T.nw;
    size_t lds = 0;
    solve_system_shape(n, nRhs, &lds);
    if (lds > 150 * 1024) FAIL(c, "solve_system: %d DOFs x %d rhs does not fit the LDS-resident solver", n, nRhs);
    Scratch sc(c);
    const size_t nc = (size_t)nGroup * n * n;
    const bool rows = solve_system_rows_ok(nUnit, nRhs);
    double *dM = sc.in<double>(Mc, nc), *dB = sc.in<double>(Bc, nc), *dC = sc.in<double>(Cc, nc);
    cplx *dX = sc.out<cplx>(Xi, (size_t)nSys * nRhs * n * nw);
    const size_t nz = assemble && !rows && nSys ? (size_t)T.nDesign * T.nCase * 36 * nw : 0;
    cplx *dZ = sc.tmp<cplx>(nz);
    if (int rc = sc.upload("solve_system_resident")) return rc;
    const cplx *Zsrc = c->rZ;
    if (dZ) {                                            // no register-resident solver for this shape: materialise Z once
        hipLaunchKernelGGL(k_assemble_unit_z, dim3((unsigned)((nz + 255) / 256)), dim3(256), 0, c->stream, T.nDesign * T.nCase, T.nCase, nw,
                           T.w, T.M0, T.B0, T.C0, c->rB, dZ);
        Zsrc = dZ;
    }
    if (sc.begin()) return -2;
    bool done = !nSys;
    if (!done && rows)
        done = assemble ? launch_solve_system_rows<true, true>(c->stream, nSys, nUnit, nRhs, nw, T.nCase, T.w, nullptr, dM, dB, dC, c->rFw, dX,
                                                               T.M0, T.B0, T.C0, c->rB)
                        : launch_solve_system_rows<true>(c->stream, nSys, nUnit, nRhs, nw, T.nCase, T.w, c->rZ, dM, dB, dC, c->rFw, dX);
    if (!done)
        if (int rc = launch_solve_system_lds<true>(c, nSys, nUnit, nRhs, nw, T.nCase, T.w, Zsrc, dM, dB, dC, c->rFw, dX)) return rc;
    return sc.finish();
}

extern "C" int raftx_qtf_kay(raftx_ctx *c, int nSet, int nw2, const double *w2, const double *k2, double depth, double rho,
                             double g, const int64_t *itemOff, const double *items, const double *beta, int Nm,
                             raftx_c128 *kay_out) {
    if (!c) return -1;
    if (nSet < 0 || nw2 < 1 || !w2 || !k2 || !itemOff || !beta) FAIL(c, "qtf_kay: bad arguments");
    if (Nm < 0 || Nm + 2 > KAY_MAXN) FAIL(c, "qtf_kay: Nm=%d outside 0..%d", Nm, KAY_MAXN - 2);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nItem = (size_t)itemOff[nSet], nq = (size_t)nSet * nw2 * nw2 * 6;
    if (nItem && !items) FAIL(c, "qtf_kay: missing items");
    c->kay_ready = false;
    if (grow_device(c, c->rKay, nq)) return -2;
    Scratch sc(c);
    double *dw = sc.in<double>(w2, nw2), *dk = sc.in<double>(k2, nw2), *dB = sc.in<double>(beta, nSet);
    int64_t *dio = sc.in<int64_t>(itemOff, (size_t)nSet + 1);
    double *dI = sc.in<double>(items, nItem * QK_N), *dq = sc.tmp<double>(nw2);
    cplx *dH = sc.tmp<cplx>(nItem * KAY_ROWS * nw2);
    sc.out_from(kay_out, c->rKay.p, nq);
    if (int rc = sc.upload("qtf_kay")) return rc;
    if (nSet) HIPCHK(c, hipMemsetAsync(c->rKay.p, 0, nq * sizeof(cplx), c->stream));       // lower triangle stays zero
    if (sc.begin()) return -2;
    if (nSet) {
        if (nItem) hipLaunchKernelGGL(k_kay_tables, dim3((unsigned)nItem), dim3(128), 0, c->stream, nw2, Nm + 2, nSet, depth, dk, dio, dI, dB, dH, dq);
        if (nItem) hipLaunchKernelGGL(k_kay_pairs, dim3((unsigned)((size_t)nSet * nw2)), dim3(nw2 > 64 ? 128 : 64), 0, c->stream, nw2, Nm,
                                      depth, rho, g, dw, dk, dio, dI, dH, dq, c->rKay.p);
    }
    if (int rc = sc.finish()) return rc;
    c->rKay_sets = nSet;
    c->rKay_nw2 = nw2;
    c->kay_ready = true;
    return 0;
}

static int qtf_slender_impl(raftx_ctx *c, int nSet, int nw2, const double *w2, const double *k2, double depth,
                            double rho, double g, const int64_t *stripOff, const double *strips,
                            const int64_t *memOff, const double *members, const raftx_c128 *Xi,
                            const double *beta, const double *Mstruc, const raftx_c128 *kay, int row_off, int row_stride,
                            raftx_c128 *qtf) {
    if (!c) return -1;
    if (nSet < 0 || nw2 < 1 || !w2 || !k2 || !stripOff || !memOff || !beta || !Mstruc)
        FAIL(c, "qtf_slender: bad arguments");
    if (!Xi && (!c->rXi || !c->have_cases || c->r_npair != (size_t)nSet))
        FAIL(c, "qtf_slender: Xi == NULL asks for the RAOs of the resident responses, but %s",
             !c->rXi ? "nothing is resident" : "the number of sets differs from the resident (design, case) pairs");
    if (row_stride < 1 || row_off < 0 || row_off >= row_stride) FAIL(c, "qtf_slender: bad row partition %d/%d", row_off, row_stride);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nStrip = (size_t)stripOff[nSet], nMem = (size_t)memOff[nSet];
    if ((nStrip && !strips) || (nMem && !members)) FAIL(c, "qtf_slender: missing tables");
    std::vector<int> sset(nStrip), mset(nMem);
    for (int s = 0; s < nSet; s++) {
        if (stripOff[s + 1] < stripOff[s] || memOff[s + 1] < memOff[s]) FAIL(c, "qtf_slender: offsets not monotone");
        for (int64_t i = stripOff[s]; i < stripOff[s + 1]; i++) sset[(size_t)i] = s;
        for (int64_t i = memOff[s]; i < memOff[s + 1]; i++) mset[(size_t)i] = s;
    }
    Scratch sc(c);
    const size_t nq = (size_t)nSet * nw2 * nw2 * 6;
    QtfArgs A;
    A.nSet = nSet;
    A.nw = nw2;
    A.depth = depth;
    A.rho = rho;
    A.g = g;
    double *dw = sc.in<double>(w2, nw2), *dk = sc.in<double>(k2, nw2), *dS = sc.in<double>(strips, nStrip * QS_N),
           *dM = sc.in<double>(members, nMem * QM_N), *dB = sc.in<double>(beta, nSet), *dMs = sc.in<double>(Mstruc, (size_t)nSet * 36);
    int64_t *dso = sc.in<int64_t>(stripOff, (size_t)nSet + 1), *dmo = sc.in<int64_t>(memOff, (size_t)nSet + 1);
    int *dss = sc.in<int>(sset.data(), nStrip), *dms = sc.in<int>(mset.data(), nMem);
    const bool use_resident_kay = !kay && c->kay_ready && c->rKay_sets == nSet && c->rKay_nw2 == nw2;
    c->kay_ready = false;                                // one-shot: a table never outlives the call it was made for
    const size_t nXi = (size_t)nSet * 6 * nw2;           // the motion RAOs: the caller's, or k_rao_to_grid's below
    cplx *dXi = Xi ? sc.in<cplx>(Xi, nXi) : sc.tmp<cplx>(nXi), *dK = kay ? sc.in<cplx>(kay, nq) : (use_resident_kay ? c->rKay.p : nullptr);
    cplx *dT = sc.tmp<cplx>(nStrip * QT_N * nw2), *dTM = sc.tmp<cplx>(nMem * QTM_N * nw2), *dTS = sc.tmp<cplx>((size_t)nSet * QTS_N * nw2);
    double *dD = sc.tmp<double>(nStrip * QD_N);
    cplx *dTA = sc.tmp<cplx>(nStrip * QT_N * nw2);
    // the result stays resident (raftx_qtf_force can reuse it)
    if (grow_device(c, c->rQtf, nq)) return -2;
    c->rQtf_sets = nSet;
    c->rQtf_nw2 = nw2;
    cplx *dQ = c->rQtf.p;
    sc.out_from(qtf, dQ, nq);
    if (int rc = sc.upload("qtf_slender")) return rc;
    A.w = dw; A.k = dk; A.soff = dso; A.strips = dS; A.moff = dmo; A.members = dM; A.sset = dss; A.mset = dms;
    A.srec = A.mrec = nullptr;                           // one table per set
    A.Xi = dXi; A.beta = dB; A.Ms = dMs; A.kay = dK; A.T = dT; A.TA = dTA; A.D = dD; A.TM = dTM; A.TS = dTS; A.qtf = dQ;
    A.row_off = row_off;
    A.row_stride = row_stride;
    A.nrow = (nw2 - row_off + row_stride - 1) / row_stride;           // rows w1 = row_off + m*row_stride of this call
    if (A.nrow < 0) A.nrow = 0;
    if (nSet && row_stride > 1) HIPCHK(c, hipMemsetAsync(dQ, 0, nq * sizeof(cplx), c->stream));   // other ranks' rows stay 0
    if (sc.begin()) return -2;
    if (nSet && !Xi)                                     // motion RAOs straight from the resident first-order responses
        hipLaunchKernelGGL(k_rao_to_grid, dim3((unsigned)((size_t)nSet * 6)), dim3(128), 0, c->stream, c->T.nCase, c->T.nHead,
                           c->T.nw, nw2, c->T.w, c->T.zeta, dw, c->rXi, dXi);
    if (nSet) {
        hipLaunchKernelGGL(k_qtf_tables, dim3((unsigned)(nStrip + nMem + nSet)), dim3(nw2 > 128 ? 256 : 128), 0, c->stream, A,
                           (int)nStrip, (int)nMem);
        if (A.nrow) {
            const int blk = nw2 > 64 ? 128 : 64;
            const size_t per_xcd = ((size_t)nSet * A.nrow + 7) / 8;                 // see k_qtf_pairs: a slab of the (set, row) list per XCD
            hipLaunchKernelGGL(k_qtf_pairs, dim3((unsigned)(per_xcd * 8)), dim3(blk), 0, c->stream, A);
        }
    }
    return sc.finish();
}

extern "C" int raftx_qtf_slender(raftx_ctx *c, int nSet, int nw2, const double *w2, const double *k2, double depth,
                                 double rho, double g, const int64_t *stripOff, const double *strips,
                                 const int64_t *memOff, const double *members, const raftx_c128 *Xi,
                                 const double *beta, const double *Mstruc, const raftx_c128 *kay, raftx_c128 *qtf) {
    return qtf_slender_impl(c, nSet, nw2, w2, k2, depth, rho, g, stripOff, strips, memOff, members, Xi, beta, Mstruc, kay, 0, 1, qtf);
}

extern "C" int raftx_qtf_slender_rows(raftx_ctx *c, int nSet, int nw2, const double *w2, const double *k2, double depth,
                                      double rho, double g, const int64_t *stripOff, const double *strips,
                                      const int64_t *memOff, const double *members, const raftx_c128 *Xi,
                                      const double *beta, const double *Mstruc, const raftx_c128 *kay, int row_off,
                                      int row_stride, raftx_c128 *qtf) {
    return qtf_slender_impl(c, nSet, nw2, w2, k2, depth, rho, g, stripOff, strips, memOff, members, Xi, beta, Mstruc, kay,
                            row_off, row_stride, qtf);
}

extern "C" int raftx_qtf_force(raftx_ctx *c, int nSet, int nw2, const double *w2, const raftx_c128 *qtf, int nw,
                               const double *w, double dw, const double *S0, double *f_mean, double *f) {
    if (!c) return -1;
    if (nSet < 0 || nw2 < 2 || nw < 1 || !w2 || !w || !S0 || !f_mean || !f) FAIL(c, "qtf_force: bad arguments");
    // k_qtf_force keeps the interpolation index and weight of every first-order bin in LDS
    const size_t lds = sizeof(double) * ((size_t)nw + ((size_t)nw + 1) / 2 + 8);
    if (lds > 65536) FAIL(c, "qtf_force: nw=%d needs %zu bytes of LDS, a workgroup may ask for 65536", nw, lds);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nq = (size_t)nSet * nw2 * nw2 * 6;
    Scratch sc(c);
    if (!qtf && (!c->rQtf.p || c->rQtf_sets != nSet || c->rQtf_nw2 != nw2))
        FAIL(c, "qtf_force: no resident QTFs of this shape (run raftx_qtf_slender first or pass qtf)");
    const cplx *dQ = qtf ? sc.in<cplx>(qtf, nq) : c->rQtf.p;
    double *dw2 = sc.in<double>(w2, nw2), *dwv = sc.in<double>(w, nw), *dS = sc.in<double>(S0, (size_t)nSet * nw),
           *dfm = sc.out<double>(f_mean, (size_t)nSet * 6), *df = sc.out<double>(f, (size_t)nSet * 6 * nw);
    if (int rc = sc.upload("qtf_force")) return rc;
    if (sc.begin()) return -2;
    if (nSet) {
        hipLaunchKernelGGL(k_qtf_force, dim3((unsigned)(nSet * 6)), dim3(256), lds, c->stream, nSet, nw2, dw2, dQ, nw, dwv, dw,
                           dS, dfm, df);
    }
    return sc.finish();
}

// ------------------------------------------------------------------ one-call sweep crossing
// raftx_sweep_stats = prepare + launch + wait on a free slot.  The designs are cut into a few blocks, every block owns a
// block context (device tables, result buffers, memory pool, events -- created on first use, kept by the parent ctx) and
// ONE host thread drives the streams of the parent ctx.  The steps, and the streams each of them enqueues on:
//   prepare  checks | crossing_streams (creates sCopy, sPrep, sD2H, sGen) | acquire_cases (pins the sea-state set) |
//            cut_blocks | upload_offsets | block_phase1 of the first blocks
//   launch   slab_streams (creates sSlab) | per block launch_block: phase1_ahead, gate_generation, build_phase2,
//            hand_sea_states, solve_enqueue, enqueue_stats | stats_after_join (slab mode)
//   wait     sweep_drain | solve_span | collect_block per block | debug_timeline
//   sCopy   descriptor H2D of every block, back to back (the first block is small, so its tables are ready early); ahead of
//           them the sea-state tables (acquire_cases), the offsets and the inputs of raftx_sweep_modal / raftx_sweep_current /
//           raftx_sweep_channels
//   sPrep   member pass + scans of a block as soon as its descriptors have landed, totals to page-locked memory
//           (block_phase1, from prepare or, one block ahead, from launch)
//   stream  (the ctx stream; every kernel that matters) strip generation, per-design reduction, the fused fixed point
//           and the statistics of block 0, 1, 2, ... strictly one after the other -- the HIP events around each
//           k_solve_dynamics launch therefore time that launch alone
//   sGen    strip generation of a crossing launched beside others (launch_block), gated by gate_generation; with
//           sSlab[0..1] the streams the slabs of an isolated crossing with responses out go to (slab_streams, SlabPlan)
//   sD2H    full responses, only when the caller asks for Xi (download_stream: sD2Hhigh where the device has priority
//           classes): whole blocks from enqueue_stats, or slab by slab from the slab plan
// The host waits only for the few bytes of totals that size a block's strip table (they are ready long before the
// compute stream reaches the block) and, at the end, for the streams to drain.
// The slot of an entry point as `SweepSlot &S`; an index out of range is refused under the entry point's own name.
#define SLOT_REF(S, c, slot, who)                                                                          \
    if ((slot) < 0 || (slot) >= RAFTX_NSLOT) FAIL(c, who ": slot must be 0 .. %d", RAFTX_NSLOT - 1);       \
    SweepSlot &S = (c)->slots[slot]
// The slot of a request entry point (raftx_sweep_modal / _current / _channels / _mooring, `who`): prepared and not yet
// launched, and still with its sea-state set where the request reads it (sea).
static int request_slot(raftx_ctx *c, int slot, const char *who, bool sea, SweepSlot **out) {
    if (slot < 0 || slot >= RAFTX_NSLOT) FAIL(c, "%s: slot must be 0 .. %d", who, RAFTX_NSLOT - 1);
    SweepSlot &S = c->slots[slot];
    if (S.busy) FAIL(c, "%s: slot %d has been launched (call it between raftx_sweep_prepare and raftx_sweep_launch)", who, slot);
    if (!S.prepared) FAIL(c, "%s: nothing prepared on slot %d (raftx_sweep_prepare first)", who, slot);
    if (sea && S.cset < 0) FAIL(c, "%s: slot %d has lost its sea-state tables (internal error)", who, slot);
    *out = &S;
    return 0;
}
static int block_ctx(raftx_ctx *c, int slot, size_t i, raftx_ctx **out) {
    std::vector<raftx_ctx *> &W = c->workers[slot];
    while (W.size() <= i) {
        raftx_ctx *sub = nullptr;
        const int rc = raftx_ctx_create(c->device, &sub);
        if (rc) FAIL(c, "sweep_stats: cannot create a block context (rc=%d)", rc);
        sub->stream.borrow(c->stream);                // block contexts run on the parent's stream: their own is destroyed
        W.push_back(sub);
    }
    *out = W[i];
    return 0;
}
// block sizes: nChunk equal blocks | default: ONE block when the other slot
// has a crossing in flight (streamed batches: that crossing's kernels hide this one's upload), otherwise a small first block
// whose kernels hide the descriptor upload of the rest (every further block costs a partial last residency round of the
// fused kernel plus the fixed latencies of the generation kernels: two blocks measured best, also for a crossing that
// downloads its responses -- profiles/MEASUREMENT_HISTORY.md, "Closed scheduling experiments of the crossing")
static std::vector<int> sweep_bounds(int nDesign, long pairs, int nChunk, bool pipelined) {
    std::vector<double> fr;
    if (nChunk > 0) fr.assign((size_t)nChunk, 1.0);
    else if (pipelined) fr = {1.0};              // the crossing in the other slot hides this one's upload: one launch, no extra tail
    else if (pairs >= 3072) fr = {0.2, 0.8};     // measured on MI355X at 10 k pairs (profiles/r02_crossing_splits.txt)
    else fr = {1.0};
    double tot = 0;
    for (double v : fr) tot += v;
    std::vector<int> b{0};
    double acc = 0;
    for (size_t i = 0; i < fr.size(); i++) {
        acc += fr[i];
        int hi = (i + 1 == fr.size()) ? nDesign : (int)llround(acc / tot * nDesign);
        if (hi > nDesign) hi = nDesign;
        if (hi > b.back()) b.push_back(hi);
    }
    if (b.back() != nDesign) b.push_back(nDesign);
    return b;
}

// is a crossing of another slot prepared or solving?
static bool others_in_flight(raftx_ctx *c, int slot) {
    for (int sl = 0; sl < RAFTX_NSLOT; sl++)
        if (sl != slot && (c->slots[sl].busy || c->slots[sl].prepared)) return true;
    return false;
}

// the crossing of slot S no longer reads its sea-state set
static void slot_release_cases(raftx_ctx *c, SweepSlot &S) {
    if (S.cset >= 0 && c->csets[S.cset].users > 0) c->csets[S.cset].users--;
    S.cset = -1;
    if (S.frec >= 0 && c->vprog.recs[S.frec].users > 0) c->vprog.recs[S.frec].users--;
    S.frec = -1;
}

// a crossing failed while it was being enqueued: drains the device, retires the jobs of its blocks, unpins its sea states
static int sweep_fail_drain(raftx_ctx *c, SweepSlot &S, int rc) {
    (void)hipDeviceSynchronize();
    for (raftx_ctx *sub : S.blk)
        if (sub) build_abandon(sub);
    S.pose.on = false;                   // (its blocks' second passes went with the jobs)
    slot_release_cases(c, S);
    return rc;
}

// the streams of the crossings, owned by the parent ctx and shared by its slots, and the slot's download marker
static int crossing_streams(raftx_ctx *c, SweepSlot &S) {
    // All four are ordinary streams (the generation stream in a high priority class lost: profiles/MEASUREMENT_HISTORY.md,
    // "Closed scheduling experiments of the crossing").  Measured (scripts/ubench/queue_probe2.hip, scripts/gpu_prep.sh): a HIGH-priority
    // preparation stream whose hardware queue happens to sit apart from the busy one does get the next batch's member
    // pass onto the chip early -- and the step gets SLOWER (4.21 vs 4.02 ms): its 184-VGPR waves break up the
    // 2 x 256-VGPR residency of the fused kernel's workgroups, and the earlier generation / fused kernel of the next
    // batch then only share the chip with the current one.  As it is, the member pass runs beside the fused kernel's
    // last residency round, which costs nothing.  (A stream whose creation failed is tried again by the next prepare.)
    HIPCHK(c, c->sCopy.ensure(hipStreamNonBlocking));
    HIPCHK(c, c->sPrep.ensure(hipStreamNonBlocking));
    HIPCHK(c, c->sD2H.ensure(hipStreamNonBlocking));
    HIPCHK(c, c->sGen.ensure(hipStreamNonBlocking));
    HIPCHK(c, S.evXi.ensure());
    return 0;
}
// Sea-state tables: sets resident on the parent, shared by the blocks of every slot that was prepared with the same
// tables; identical tables are not uploaded again (others: on sCopy, into the idle set used longest ago).  The slot pins
// its set (S.cset) until it is retired (wait / cancel / failure), so other sea states prepared meanwhile leave it alone.
static int acquire_cases(raftx_ctx *c, SweepSlot &S, const SeaStates &sea) {
    const int nCase = sea.nCase, nHead = sea.nHead, nw = sea.nw;
    std::vector<double> key;
    key.reserve((size_t)nw * 2 + (size_t)nCase * nHead * (nw + 1) + 6);
    key.push_back(nCase); key.push_back(nHead); key.push_back(nw); key.push_back(sea.depth); key.push_back(sea.rho); key.push_back(sea.g);
    key.insert(key.end(), sea.w, sea.w + nw);
    key.insert(key.end(), sea.k, sea.k + nw);
    key.insert(key.end(), sea.zeta, sea.zeta + (size_t)nCase * nHead * nw);
    key.insert(key.end(), sea.beta, sea.beta + (size_t)nCase * nHead);
    int hit = -1, idle = -1;
    for (int i = 0; i <= RAFTX_NSLOT; i++) {
        CaseSet &cs = c->csets[i];
        if (!cs.key.empty() && cs.key.size() == key.size() && memcmp(key.data(), cs.key.data(), key.size() * sizeof(double)) == 0) hit = i;
        else if (cs.users == 0 && (idle < 0 || cs.stamp < c->csets[idle].stamp)) idle = i;
    }
    if (hit < 0) {
        if (idle < 0) FAIL(c, "sweep_prepare: no free sea-state set (every set is pinned by a crossing in flight)");   // cannot happen: NSLOT + 1 sets
        CaseSet &cs = c->csets[idle];
        cs.key.clear();
        cs.allocs.release();                      // users == 0: every crossing that read it has been waited for
        if (int rc = upload_case_tables(c, c->sCopy, cs.allocs, cs.T, sea)) {
            cs.allocs.release();
            return rc;
        }
        cs.key.swap(key);
        hit = idle;
    }
    c->csets[hit].users++;
    c->csets[hit].stamp = ++c->cset_clock;
    S.cset = hit;
    return 0;
}
// what the solve of a crossing is given: fixed-point settings, block count, and the caller's outputs
struct SweepRun { int nIter; double tol, XiStart; int nChunk; double *sd; int32_t *niter, *flags; raftx_c128 *Xi; int64_t *stripOffsets; };
// The slot takes the crossing: block bounds, settings and outputs.  The slot's previous crossing has been waited for, so
// what it kept on the device goes back to the pool.
static void cut_blocks(raftx_ctx *c, int slot, int nDesign, const SeaStates &sea, const SweepRun &run) {
    SweepSlot &S = c->slots[slot];
    S.bnd = sweep_bounds(nDesign, (long)nDesign * sea.nCase, std::min(run.nChunk, 64), others_in_flight(c, slot));
    S.dw = sea.nw > 1 ? sea.w[1] - sea.w[0] : sea.w[0];
    S.nIter = run.nIter; S.tol = run.tol; S.XiStart = run.XiStart;
    S.blk.assign(S.bnd.size() - 1, nullptr);
    S.nCase = sea.nCase; S.nHead = sea.nHead; S.nw = sea.nw;
    S.sd = run.sd; S.niter = run.niter; S.flags = run.flags; S.Xi = run.Xi; S.stripOffsets = run.stripOffsets;
    S.tl[0] = S.since();
    S.allocs.release();
    S.clear_requests();
}
// The batch's offset arrays: one upload on sCopy, shared by the blocks; its wave numbers are those of the sea-state set.
static int upload_offsets(raftx_ctx *c, SweepSlot &S, const BuildSource &src, int nDesign) {
    S.p1 = src;
    S.p1.k_dev = c->csets[S.cset].T.k;
    const int64_t nMemberAll = src.memberOff[nDesign];
    DevOffsets &dOff = S.p1.dOff;
    int rc = upload_on(c, c->sCopy, S.allocs, src.memberOff, (size_t)nDesign + 1, &dOff.memberOff);
    rc |= upload_on(c, c->sCopy, S.allocs, src.stationOff, (size_t)nMemberAll + 1, &dOff.stationOff);
    if (src.capOff) rc |= upload_on(c, c->sCopy, S.allocs, src.capOff, (size_t)nMemberAll + 1, &dOff.capOff);
    return rc ? -2 : 0;
}
// phase 1 of block b: descriptor H2D on sCopy, member pass + scans on sPrep
static int block_phase1(raftx_ctx *c, SweepSlot &S, size_t b) {
    return build_phase1(S.blk[b], c->sCopy, c->sPrep, S.p1, S.bnd[b], S.bnd[b + 1] - S.bnd[b]);
}

static void launch_mean_pose(hipStream_t st, MeanPoseArgs &A, int nDesign, int nLine, double depth, double tolT, double tolR, int max_iter);
// The pose steps of block b (raftx_sweep_mean_pose), on the preparation stream behind the block's phase 1, no host wait between
// them: K_hs and F0 from the statics the reductions left at the reference pose (k_pose_assemble, behind the side stream),
// the Newton solve (k_mean_pose), the poses of the second pass and the outputs to the landing area (k_pose_place), then the
// member pass, the reductions and the scans again at those poses.  The fixed members' record is for an unposed unit: off.
static int block_pose(raftx_ctx *c, SweepSlot &S, size_t b) {
    raftx_ctx *sub = S.blk[b];
    BuildJob &J = sub->job;
    GeomArgs &A = J.A;
    const size_t lo = (size_t)S.bnd[b], nAll = (size_t)S.bnd.back();
    const int n = S.bnd[b + 1] - S.bnd[b];
    HIPCHK(sub, sub->evPose.ensure(hipEventDisableTiming));
    hipStream_t sPrep = c->sPrep;
    if (n > 0) {
        if (!J.active || J.nDesign != n) FAIL(sub, "sweep_mean_pose: the block has no member pass in flight (internal error)");
        HIPCHK(sub, hipStreamWaitEvent(sPrep, S.pose.evUp, 0));
        if (J.reduce_stream) HIPCHK(sub, hipStreamWaitEvent(sPrep, sub->evRed, 0));
        const auto &P = S.pose;
        PoseAssembleArgs Q;
        memset(&Q, 0, sizeof(Q));
        Q.n = n; Q.Cs = A.Cs; Q.Ch = A.Ch; Q.Ws = A.Ws; Q.Wh = A.Wh;
        Q.strideC = P.nX > 1 ? 36 : 0; Q.strideF = P.nX > 1 ? 6 : 0;
        Q.Cx = P.Cx ? P.Cx + lo * Q.strideC : nullptr;
        Q.Fx = P.Fx ? P.Fx + lo * Q.strideF : nullptr;
        Q.K = P.K + lo * 36; Q.F0 = P.F0 + lo * 6;
        hipLaunchKernelGGL(k_pose_assemble, dim3((unsigned)(((size_t)n * 42 + 255) / 256)), dim3(256), 0, sPrep, Q);
        MeanPoseArgs M;
        memset(&M, 0, sizeof(M));
        M.lines = P.lines + lo * P.nLine * RAFTX_ML_N;
        M.chains = P.chains;
        M.K_hs = Q.K; M.F0 = Q.F0;
        M.F_env = P.Fenv ? P.Fenv + lo * 6 : nullptr;
        M.x_ref = A.pose;                                        // the block's own upload of the caller's pose, or null
        M.lw = P.lw + lo * P.nLine * MOOR_LW_N;
        M.bw = P.bw ? P.bw + lo * P.nLine * MOOR_BW_N : nullptr;
        M.pose = P.solved + lo * 6; M.Fres = P.Fres + lo * 6;
        M.iterations = P.iter + lo; M.flags = P.fl + lo;
        launch_mean_pose(sPrep, M, n, P.nLine, c->csets[S.cset].T.depth, P.tolT, P.tolR, P.maxIter);
        PosePlaceArgs L;
        memset(&L, 0, sizeof(L));
        L.n = n; L.solved = M.pose; L.x_ref = A.pose; L.Fres = M.Fres; L.iterations = M.iterations; L.flags = M.flags;
        L.placed = P.placed + lo * 6;
        const landing::Pose land = landing::pose(nAll);
        L.hPose = P.pin.p + land.pose + lo * 6; L.hFres = P.pin.p + land.Fres + lo * 6;
        L.hIter = land.iterations.in(P.pin.p) + lo; L.hFlags = land.flags.in(P.pin.p) + lo;
        hipLaunchKernelGGL(k_pose_place, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, sPrep, L);
        HIPCHK(sub, hipGetLastError());
        A.pose = L.placed;
        A.fixRec = nullptr; A.fixInt = nullptr; A.fixIdx = nullptr; A.fixNM = 0;
    }
    HIPCHK(sub, hipEventRecord(sub->evPose, sPrep));
    if (n > 0) {
        if (int rc = enqueue_member_repass(sub, sPrep)) return rc;
        if (int rc = enqueue_scan_reduce(sub, sPrep)) return rc;
    }
    return 0;
}
// phase 1 of a block that has not had it yet (S.next_p1), with the pose steps of a crossing that asked for them
static int block_phase1_next(raftx_ctx *c, SweepSlot &S, size_t *which = nullptr) {
    const size_t bn = S.next_p1++;
    if (which) *which = bn;
    if (int rc = block_phase1(c, S, bn)) return rc;
    return S.pose.on ? block_pose(c, S, bn) : 0;
}

static int acquire_fixed(raftx_ctx *c, SweepSlot &S);
static int sweep_prepare_impl(raftx_ctx *c, int slot, int nDesign, const BuildSource &src, const SeaStates &sea, const SweepRun &run) {
    RangeScope range_("raftx_sweep_prepare: descriptor H2D + member pass (enqueue)");
    if (!c) return -1;
    SLOT_REF(S, c, slot, "sweep_prepare");
    if (S.busy || S.prepared) FAIL(c, "sweep_prepare: slot %d is still in flight (call raftx_sweep_wait first)", slot);
    if (int rc = check_source(c, src, nDesign, "sweep_stats", "bad design arguments")) return rc;
    if (sea.nCase < 1 || sea.nHead < 1 || sea.nw < 1 || !sea.w || !sea.k || !sea.zeta || !sea.beta) FAIL(c, "sweep_stats: bad sea-state arguments");
    if (!run.sd || !run.niter || !run.flags) FAIL(c, "sweep_stats: std, niter and flags are required");
    if (run.nIter < 0) FAIL(c, "sweep_stats: nIter < 0");
    HIPCHK(c, hipSetDevice(c->device));
    S.t0 = std::chrono::steady_clock::now();
    if (int rc = crossing_streams(c, S)) return rc;
    if (sea.nw > MAX_NW) FAIL(c, "nw=%d exceeds the %d bins per workgroup supported by this build", sea.nw, MAX_NW);
    if (int rc = acquire_cases(c, S, sea)) return rc;
    // ---- the set is pinned: every return below releases it (slot_release_cases; sweep_fail_drain once work is enqueued)
    cut_blocks(c, slot, nDesign, sea, run);
    if (src.memberOff[nDesign] < 0) {
        slot_release_cases(c, S);
        FAIL(c, "sweep_stats: member offsets not monotone");
    }
    if (int rc = upload_offsets(c, S, src, nDesign)) return sweep_fail_drain(c, S, rc);
    if (int rc = acquire_fixed(c, S)) return sweep_fail_drain(c, S, rc);
    // ---- phase 1: H2D on sCopy, member pass + scans on sPrep.  Every block here -- except for an isolated crossing cut into
    // slabs (responses wanted, nothing else in flight): there only the first two; raftx_sweep_launch enqueues the others one
    // block ahead of the block it launches.  (The ordinary streams share hardware queues: with every block's copies queued
    // first, the first slab's generation sat behind 1.7 ms of uploads -- profiles/r04_iso_timeline.txt.)
    const size_t nB = S.blk.size(), nFirst = (run.Xi && nB > 2 && !others_in_flight(c, slot)) ? 2 : nB;
    for (size_t b = 0; b < nB; b++)
        if (block_ctx(c, slot, b, &S.blk[b])) return sweep_fail_drain(c, S, -1);
    for (size_t b = 0; b < nFirst; b++)
        if (const int rc = block_phase1(c, S, b)) {
            snprintf(c->err, sizeof(c->err), "sweep_stats (block %zu): %s", b, S.blk[b]->err);
            return sweep_fail_drain(c, S, rc);
        }
    S.next_p1 = nFirst;
    S.tl[1] = S.since();
    S.prepared = true;
    return 0;
}

extern "C" int raftx_sweep_prepare(raftx_ctx *c, int slot, int nDesign, const int64_t *memberOff, const double *members,
                                  const int64_t *stationOff, const double *stations, const int64_t *capOff,
                                  const double *caps, const double *pose, double rho, double g, int add_mask,
                                  const double *M0, const double *B0, const double *C0, const double *Fz_moor, int nCase,
                                  int nHead, int nw, const double *w, const double *k, double depth, double rho_wave,
                                  double g_wave, const double *zeta, const double *beta, int nIter, double tol,
                                  double XiStart, int nChunk, double *sd, int32_t *niter, int32_t *flags,
                                  raftx_c128 *Xi, int64_t *stripOffsets) {
    const BuildSource src{memberOff, stationOff, capOff, members, stations, caps, pose, M0, B0, C0, nullptr, Fz_moor, k, rho, g, nw, add_mask};
    return sweep_prepare_impl(c, slot, nDesign, src, SeaStates{nCase, nHead, nw, w, k, depth, rho_wave, g_wave, zeta, beta},
                              SweepRun{nIter, tol, XiStart, nChunk, sd, niter, flags, Xi, stripOffsets});
}

// ---- parametric variants of one base unit (include/raftx.h; raft/parametersweep.py:39-87)
extern "C" int raftx_variant_program(raftx_ctx *c, int nMember, const double *members, const int64_t *stationOff, const double *stations,
                                     const int64_t *capOff, const double *caps, int nParam, const double *endCoef,
                                     const int32_t *endEdit, const double *headCS, const double *diaCoef, const int32_t *diaEdit) {
    if (!c) return -1;
    for (int sl = 0; sl < RAFTX_NSLOT; sl++)
        if ((c->slots[sl].busy || c->slots[sl].prepared) && c->slots[sl].p1.var.prog)
            FAIL(c, "variant_program: a batch of variants is still in flight (raftx_sweep_wait first)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    VariantProg &P = c->vprog;
    variant_release(c);                               // the fixed members' records go with the program
    if (nMember == 0) return 0;
    if (nMember < 0 || nParam < 0 || nParam > 64 || !members || !stationOff || !stations || (capOff == nullptr) != (caps == nullptr))
        FAIL(c, "variant_program: bad arguments");
    if (!endEdit || !endCoef || !headCS || !diaEdit || !diaCoef) FAIL(c, "variant_program: the edit tables are required (all-zero flags = no edit)");
    const int nM = nMember, nP = nParam;
    if (stationOff[0] != 0 || (capOff && capOff[0] != 0)) FAIL(c, "variant_program: offsets must start at 0");
    for (int m = 0; m < nM; m++)
        if (stationOff[m + 1] < stationOff[m] || (capOff && capOff[m + 1] < capOff[m])) FAIL(c, "variant_program: offsets not monotone");
    const int nSt = (int)stationOff[nM], nCap = capOff ? (int)capOff[nM] : 0;
    std::vector<int> stM((size_t)nSt), cpM((size_t)nCap);
    std::vector<double> stF((size_t)nSt), flF((size_t)nSt), cpF((size_t)nCap);
    for (int m = 0; m < nM; m++) {
        const double L = members[(size_t)m * RAFTX_GM_N + RAFTX_GM_L];
        if (endEdit[m] && !(L > 0.0)) FAIL(c, "variant_program: member %d has no length", m);
        for (int64_t i = stationOff[m]; i < stationOff[m + 1]; i++) {
            stM[(size_t)i] = m;
            stF[(size_t)i] = stations[(size_t)i * RAFTX_GS_N + RAFTX_GS_S] / L;          // fractions of the length: what the deck's
            flF[(size_t)i] = stations[(size_t)i * RAFTX_GS_N + RAFTX_GS_LFILL] / L;      // arbitrary station units mean
        }
        if (capOff)
            for (int64_t i = capOff[m]; i < capOff[m + 1]; i++) {
                cpM[(size_t)i] = m;
                cpF[(size_t)i] = caps[(size_t)i * RAFTX_GC_N + RAFTX_GC_S] / L;
            }
    }
    P.nM = nM; P.nSt = nSt; P.nCap = nCap; P.nP = nP; P.has_caps = capOff != nullptr;
    P.hS.assign(stationOff, stationOff + nM + 1);
    if (capOff) P.hC.assign(capOff, capOff + nM + 1);
    else P.hC.assign((size_t)nM + 1, 0);
    auto up = [&](const void *h, size_t bytes, void **d) -> int {
        *d = nullptr;
        if (!bytes) bytes = 8, h = nullptr;
        HIPCHK(c, P.allocs.get_outside(c->pool, bytes, d));
        if (h) HIPCHK(c, hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice));
        return 0;
    };
    int rc = 0;
    rc |= up(members, (size_t)nM * RAFTX_GM_N * 8, (void **)&P.gm);
    rc |= up(stations, (size_t)nSt * RAFTX_GS_N * 8, (void **)&P.gs);
    rc |= up(nCap ? caps : nullptr, (size_t)nCap * RAFTX_GC_N * 8, (void **)&P.gc);
    rc |= up(stM.data(), (size_t)nSt * 4, (void **)&P.stMember);
    rc |= up(nCap ? cpM.data() : nullptr, (size_t)nCap * 4, (void **)&P.capMember);
    rc |= up(stF.data(), (size_t)nSt * 8, (void **)&P.stFrac);
    rc |= up(flF.data(), (size_t)nSt * 8, (void **)&P.fillFrac);
    rc |= up(nCap ? cpF.data() : nullptr, (size_t)nCap * 8, (void **)&P.capFrac);
    rc |= up(endCoef, (size_t)nM * 6 * (nP + 1) * 8, (void **)&P.endCoef);
    rc |= up(headCS, (size_t)nM * 2 * 8, (void **)&P.headCS);
    rc |= up(diaCoef, (size_t)nSt * 2 * (nP + 1) * 8, (void **)&P.diaCoef);
    rc |= up(endEdit, (size_t)nM * 4, (void **)&P.endEdit);
    rc |= up(diaEdit, (size_t)nSt * 4, (void **)&P.diaEdit);
    // fixed members: no end edit and no diameter edit on any of their stations
    std::vector<int> desc, fidx((size_t)nM, -1);
    for (int m = 0; m < nM; m++) {
        bool fixed = endEdit[m] == 0;
        for (int64_t i = stationOff[m]; fixed && i < stationOff[m + 1]; i++) fixed = diaEdit[i] == 0;
        if (!fixed) continue;
        fidx[(size_t)m] = P.nFix++;
        desc.insert(desc.end(), {m, (int)stationOff[m], (int)(stationOff[m + 1] - stationOff[m]), capOff ? (int)capOff[m] : 0,
                                 capOff ? (int)(capOff[m + 1] - capOff[m]) : -1});
    }
    if (P.nFix) {
        rc |= up(desc.data(), desc.size() * 4, (void **)&P.fixDesc);
        rc |= up(fidx.data(), (size_t)nM * 4, (void **)&P.fixIdx);
        for (FixedRecord &R : P.recs) {
            rc |= up(nullptr, (size_t)P.nFix * FR_N * 8, (void **)&R.rec);
            rc |= up(nullptr, (size_t)P.nFix * FR_I * 4, (void **)&R.irec);
            if (!rc) HIPCHK(c, hipMemset(R.rec, 0, (size_t)P.nFix * FR_N * 8));
        }
    }
    if (rc) {
        variant_release(c);
        return rc;
    }
    return 0;
}
// The record of the program's fixed members for the slot's crossing: the one with the crossing's key, or -- on sPrep,
// ahead of the member passes that copy it -- k_geom_member_fixed into the idle record used longest ago.  Pinned by the
// slot until it is retired (slot_release_cases).  No record: no fixed member, or per-design poses.
static int acquire_fixed(raftx_ctx *c, SweepSlot &S) {
    VariantProg &P = c->vprog;
    BuildSource &src = S.p1;
    src.var.rec = nullptr;
    if (src.var.prog != &P || !P.nFix || src.pose) return 0;
    const int trim = (src.add_mask & RAFTX_TRIM_BALLAST) != 0, haveK = src.k_dev != nullptr;
    int hit = -1, idle = -1;
    for (int i = 0; i <= RAFTX_NSLOT; i++) {
        const FixedRecord &R = P.recs[i];
        if (R.valid && R.rho == src.rho && R.g == src.g && R.trim == trim && R.haveK == haveK) hit = i;
        else if (R.users == 0 && (idle < 0 || R.stamp < P.recs[idle].stamp)) idle = i;
    }
    if (hit < 0) {
        if (idle < 0) FAIL(c, "sweep_prepare_variants: no free record of the fixed members");      // cannot happen: NSLOT + 1 records
        FixedRecord &R = P.recs[idle];                // users == 0: every crossing that read it has been waited for
        R.valid = false;
        HIPCHK(c, R.ev.ensure(hipEventDisableTiming));
        FixedArgs F{P.nFix, P.gm, P.gs, P.gc, P.fixDesc, src.rho, src.g, trim, haveK, R.rec, R.irec};
        hipLaunchKernelGGL(k_geom_member_fixed, dim3((unsigned)((P.nFix + 63) / 64)), dim3(64), 0, c->sPrep, F);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(R.ev, c->sPrep));
        R.stream = c->sPrep;
        R.rho = src.rho; R.g = src.g; R.trim = trim; R.haveK = haveK;
        R.valid = true;
        hit = idle;
    }
    P.recs[hit].users++;
    P.recs[hit].stamp = ++P.rec_clock;
    S.frec = hit;
    src.var.rec = &P.recs[hit];
    return 0;
}
// uniform offsets of n variants, cached on the program
static void variant_offsets(VariantProg &P, int n) {
    if (P.cachedN == n) return;
    P.memberOff.resize((size_t)n + 1);
    P.stationOff.resize((size_t)n * P.nM + 1);
    P.capOff.resize((size_t)n * P.nM + 1);
    for (int d = 0; d <= n; d++) P.memberOff[(size_t)d] = (int64_t)d * P.nM;
    for (int d = 0; d < n; d++)
        for (int m = 0; m < P.nM; m++) {
            P.stationOff[(size_t)d * P.nM + m] = (int64_t)d * P.nSt + P.hS[(size_t)m];
            P.capOff[(size_t)d * P.nM + m] = (int64_t)d * P.nCap + P.hC[(size_t)m];
        }
    P.stationOff[(size_t)n * P.nM] = (int64_t)n * P.nSt;
    P.capOff[(size_t)n * P.nM] = (int64_t)n * P.nCap;
    P.cachedN = n;
}
extern "C" int raftx_expand_variants(raftx_ctx *c, int nDesign, const double *params, double *members, double *stations, double *caps) {
    if (!c) return -1;
    const VariantProg &P = c->vprog;
    if (!P.nM) FAIL(c, "expand_variants: no program (raftx_variant_program first)");
    if (nDesign < 0 || (!params && nDesign && P.nP) || !members || !stations) FAIL(c, "expand_variants: bad arguments");
    if (!nDesign) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    const size_t nc = (size_t)nDesign * P.nCap * RAFTX_GC_N;
    double *dp = sc.in<double>(params, (size_t)nDesign * P.nP), *dg = sc.out<double>(members, (size_t)nDesign * P.nM * RAFTX_GM_N),
           *ds_ = sc.out<double>(stations, (size_t)nDesign * P.nSt * RAFTX_GS_N),
           *dc = caps ? sc.out<double>(caps, nc) : sc.tmp<double>(nc);        // (the kernel writes the caps whether they are asked for or not)
    if (int rc = sc.upload("expand_variants")) return rc;
    ExpandArgs E;
    memset(&E, 0, sizeof(E));
    E.params = dp;
    expand_args(P, nDesign, dg, ds_, dc, E);
    if (sc.begin()) return -2;
    launch_expand(E, c->stream);
    return sc.finish();
}
extern "C" int raftx_sweep_prepare_variants(raftx_ctx *c, int slot, int nDesign, const double *params, const double *pose, double rho,
                                           double g, int add_mask, const double *M0, const double *B0, const double *C0,
                                           const double *Fz_moor, int nCase, int nHead, int nw, const double *w, const double *k,
                                           double depth, double rho_wave, double g_wave, const double *zeta, const double *beta,
                                           int nIter, double tol, double XiStart, int nChunk, double *sd, int32_t *niter,
                                           int32_t *flags, raftx_c128 *Xi, int64_t *stripOffsets) {
    if (!c) return -1;
    VariantProg &P = c->vprog;
    if (!P.nM) FAIL(c, "sweep_prepare_variants: no program (raftx_variant_program first)");
    if (nDesign < 0 || (!params && nDesign && P.nP)) FAIL(c, "sweep_prepare_variants: bad arguments");
    SLOT_REF(S, c, slot, "sweep_prepare_variants");
    if (S.busy || S.prepared)                       // before the cached offset arrays are touched: the batch on this slot reads them
        FAIL(c, "sweep_prepare_variants: slot %d is still in flight (call raftx_sweep_wait first)", slot);
    for (int sl = 0; sl < RAFTX_NSLOT; sl++)        // the offset arrays of batches in flight are the cached ones: one batch size at a time
        if (sl != slot && (c->slots[sl].busy || c->slots[sl].prepared) && c->slots[sl].p1.var.prog && P.cachedN != nDesign)
            FAIL(c, "sweep_prepare_variants: batches of variants in flight together must have the same size (%d in flight, %d asked)",
                 P.cachedN, nDesign);
    variant_offsets(P, nDesign);
    BuildSource src{P.memberOff.data(), P.stationOff.data(), P.has_caps ? P.capOff.data() : nullptr, nullptr, nullptr, nullptr,
                    pose, M0, B0, C0, nullptr, Fz_moor, k, rho, g, nw, add_mask};
    src.var = {&P, params};
    return sweep_prepare_impl(c, slot, nDesign, src, SeaStates{nCase, nHead, nw, w, k, depth, rho_wave, g_wave, zeta, beta},
                              SweepRun{nIter, tol, XiStart, nChunk, sd, niter, flags, Xi, stripOffsets});
}

// ------------------------------------------------------------------ second-order tables on the device (include/raftx_qtfgen.h)
static bool all_finite(const double *a, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(a[i])) return false;
    return true;
}
// The generator on descriptors that are in device memory already (uploaded, or written by k_geom_expand on the ctx stream):
// member pass, offsets inside the designs, scan over the designs, the totals to the host, the write pass.  The tables of an
// earlier build have been released by the caller's checks passing; `sc` owns the descriptors and the per-member scratch.
static int qtfgen_run(raftx_ctx *c, Scratch &sc, const char *who, int nDesign, int64_t nMember, const int64_t *dMemberOff,
                      const int64_t *dStationOff, const double *dgm, const double *dgs, const double *dpose, int64_t *stripOff_out,
                      int64_t *memOff_out) {
    QtfResident &Q = c->qt;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    Q = QtfResident();                                // (move assignment: the old records' bag gives its blocks back first)
    const size_t nD1 = (size_t)nDesign + 1;
    QGenArgs A;
    memset(&A, 0, sizeof(A));
    A.nDesign = nDesign; A.nMember = nMember; A.memberOff = dMemberOff; A.stationOff = dStationOff;
    A.gm = dgm; A.gs = dgs; A.pose = dpose;
    const size_t ntot = (size_t)std::max(nDesign, 1) * QG_CNT_N;
    A.mdesign = sc.tmp<int>((size_t)nMember); A.mpose = sc.tmp<double>((size_t)nMember * QG_MP_N);
    A.mcnt = sc.tmp<int>((size_t)nMember * QG_CNT_N); A.mcand = sc.tmp<int>((size_t)nMember);
    A.dtot = sc.tmp<int>(ntot); A.err = sc.tmp<int>(1);
    if (pool_alloc(c, Q.allocs, QG_CNT_N * nD1, &Q.dOff)) return -2;
    A.off = Q.dOff;
    if (int rc = sc.upload(who)) return rc;           // (the caller's arrays are on their way already: nothing new to send)
    HIPCHK(c, hipMemsetAsync(A.err, 0, sizeof(int), c->stream));
    HIPCHK(c, hipMemsetAsync(A.dtot, 0, ntot * sizeof(int), c->stream));
    if (sc.begin()) return -2;
    const int64_t nThread = std::max<int64_t>(nMember, nDesign);
    if (nThread) hipLaunchKernelGGL(k_qtfgen_member, dim3((unsigned)((nThread + 127) / 128)), dim3(128), 0, c->stream, A);
    if (nDesign) hipLaunchKernelGGL(k_qtfgen_design, dim3((unsigned)((nDesign + 255) / 256)), dim3(256), 0, c->stream, A);
    hipLaunchKernelGGL(k_qtfgen_scan, dim3(1), dim3(QG_SCAN_T), 0, c->stream, nDesign, A.dtot, A.off);
    HIPCHK(c, hipGetLastError());
    Q.off.resize(QG_CNT_N * nD1);
    int err = 0;
    D2H(c, Q.off.data(), Q.dOff, QG_CNT_N * nD1 * sizeof(int64_t));
    D2H(c, &err, A.err, sizeof(int));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    Q.nDesign = nDesign;
    if (err) {
        Q = QtfResident();
        FAIL(c, "%s: member %d has fewer than two stations, dlsMax <= 0 or no length", who, err - 1);
    }
    if (pool_alloc(c, Q.allocs, (size_t)Q.total(0) * QS_N, &Q.strips) || pool_alloc(c, Q.allocs, (size_t)Q.total(1) * QM_N, &Q.members) ||
        pool_alloc(c, Q.allocs, (size_t)Q.total(2) * QKR_N, &Q.kay)) {
        Q = QtfResident();
        return -2;
    }
    A.strips = Q.strips; A.members = Q.members; A.kay = Q.kay;
    if (nMember) hipLaunchKernelGGL(k_qtfgen_write, dim3((unsigned)((nMember + 3) / 4)), dim3(256), 0, c->stream, A);
    if (finish_timed(c)) return -2;
    Q.valid = true;
    if (stripOff_out) memcpy(stripOff_out, Q.off.data(), nD1 * sizeof(int64_t));
    if (memOff_out) memcpy(memOff_out, Q.off.data() + nD1, nD1 * sizeof(int64_t));
    return 0;
}

extern "C" int raftx_qtf_tables_build(raftx_ctx *c, int nDesign, const int64_t *memberOff, const double *members,
                                      const int64_t *stationOff, const double *stations, const double *pose, int64_t *stripOff_out,
                                      int64_t *memOff_out) {
    if (!c) return -1;
    if (nDesign < 0 || !memberOff || !stationOff) FAIL(c, "qtf_tables_build: bad arguments");
    for (int d = 0; d < nDesign; d++)
        if (memberOff[d + 1] < memberOff[d]) FAIL(c, "qtf_tables_build: member offsets not monotone at design %d", d);
    const int64_t m0 = memberOff[0], nMember = memberOff[nDesign] - m0;
    if (m0 < 0) FAIL(c, "qtf_tables_build: member offsets not monotone at design 0");
    for (int64_t m = 0; m < nMember; m++)
        if (stationOff[m0 + m + 1] < stationOff[m0 + m]) FAIL(c, "qtf_tables_build: station offsets not monotone at member %lld", (long long)(m0 + m));
    const int64_t s0 = stationOff[m0], nSta = stationOff[m0 + nMember] - s0;
    if (s0 < 0) FAIL(c, "qtf_tables_build: station offsets not monotone at member %lld", (long long)m0);
    if ((nMember && !members) || (nSta && !stations)) FAIL(c, "qtf_tables_build: bad arguments");
    if (nMember >= ((int64_t)1 << 31)) FAIL(c, "qtf_tables_build: %lld members in one batch", (long long)nMember);
    if (!all_finite(members + (size_t)m0 * RAFTX_GM_N, (size_t)nMember * RAFTX_GM_N) ||
        !all_finite(stations + (size_t)s0 * RAFTX_GS_N, (size_t)nSta * RAFTX_GS_N) || (pose && !all_finite(pose, (size_t)nDesign * 6)))
        FAIL(c, "qtf_tables_build: a member, station or pose value is not finite");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<int64_t> mo((size_t)nDesign + 1), so((size_t)nMember + 1);
    for (int d = 0; d <= nDesign; d++) mo[(size_t)d] = memberOff[d] - m0;
    for (int64_t m = 0; m <= nMember; m++) so[(size_t)m] = stationOff[m0 + m] - s0;
    Scratch sc(c);
    int64_t *dmo = sc.in<int64_t>(mo.data(), mo.size()), *dso = sc.in<int64_t>(so.data(), so.size());
    double *dgm = sc.in<double>(members + (size_t)m0 * RAFTX_GM_N, (size_t)nMember * RAFTX_GM_N),
           *dgs = sc.in<double>(stations + (size_t)s0 * RAFTX_GS_N, (size_t)nSta * RAFTX_GS_N), *dps = sc.in<double>(pose, (size_t)nDesign * 6);
    if (int rc = sc.upload("qtf_tables_build")) return rc;
    return qtfgen_run(c, sc, "qtf_tables_build", nDesign, nMember, dmo, dso, dgm, dgs, dps, stripOff_out, memOff_out);
}

extern "C" int raftx_qtf_tables_build_variants(raftx_ctx *c, int nDesign, const double *params, const double *pose,
                                               int64_t *stripOff_out, int64_t *memOff_out) {
    if (!c) return -1;
    const VariantProg &P = c->vprog;
    if (!P.nM) FAIL(c, "qtf_tables_build_variants: no program (raftx_variant_program first)");
    if (nDesign < 0 || (!params && nDesign && P.nP)) FAIL(c, "qtf_tables_build_variants: bad arguments");
    if ((params && !all_finite(params, (size_t)nDesign * P.nP)) || (pose && !all_finite(pose, (size_t)nDesign * 6)))
        FAIL(c, "qtf_tables_build_variants: a parameter or pose value is not finite");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t nMember = (int64_t)nDesign * P.nM, nSta = (int64_t)nDesign * P.nSt;
    if (nMember >= ((int64_t)1 << 31)) FAIL(c, "qtf_tables_build_variants: %lld members in one batch", (long long)nMember);
    std::vector<int64_t> mo((size_t)nDesign + 1), so((size_t)nMember + 1);      // the uniform offsets of the batch
    for (int d = 0; d <= nDesign; d++) mo[(size_t)d] = (int64_t)d * P.nM;
    for (int d = 0; d < nDesign; d++)
        for (int m = 0; m < P.nM; m++) so[(size_t)d * P.nM + m] = (int64_t)d * P.nSt + P.hS[(size_t)m];
    so[(size_t)nMember] = nSta;
    Scratch sc(c);
    int64_t *dmo = sc.in<int64_t>(mo.data(), mo.size()), *dso = sc.in<int64_t>(so.data(), so.size());
    double *dp = sc.in<double>(params, (size_t)nDesign * P.nP), *dps = sc.in<double>(pose, (size_t)nDesign * 6);
    double *dgm = sc.tmp<double>((size_t)nMember * RAFTX_GM_N), *dgs = sc.tmp<double>((size_t)nSta * RAFTX_GS_N),
           *dgc = sc.tmp<double>((size_t)nDesign * P.nCap * RAFTX_GC_N);
    if (int rc = sc.upload("qtf_tables_build_variants")) return rc;
    if (nDesign) {
        ExpandArgs E;
        memset(&E, 0, sizeof(E));
        E.params = dp;
        expand_args(P, nDesign, dgm, dgs, dgc, E);
        launch_expand(E, c->stream);
    }
    return qtfgen_run(c, sc, "qtf_tables_build_variants", nDesign, nMember, dmo, dso, dgm, dgs, dps, stripOff_out, memOff_out);
}

extern "C" int raftx_qtf_tables_counts(raftx_ctx *c, int64_t *counts) {
    if (!c) return -1;
    if (!counts) FAIL(c, "qtf_tables_counts: bad arguments");
    if (!c->qt.valid) FAIL(c, "qtf_tables_counts: no resident tables (raftx_qtf_tables_build first)");
    counts[0] = c->qt.nDesign;
    for (int j = 0; j < QG_CNT_N; j++) counts[1 + j] = c->qt.total(j);
    return 0;
}

extern "C" int raftx_qtf_tables_fetch(raftx_ctx *c, double *strips, double *members, int64_t *kayOff, double *kayNodes) {
    if (!c) return -1;
    const QtfResident &Q = c->qt;
    if (!Q.valid) FAIL(c, "qtf_tables_fetch: no resident tables (raftx_qtf_tables_build first)");
    HIPCHK(c, hipSetDevice(c->device));
    if (strips && Q.total(0)) D2H(c, strips, Q.strips, (size_t)Q.total(0) * QS_N * sizeof(double));
    if (members && Q.total(1)) D2H(c, members, Q.members, (size_t)Q.total(1) * QM_N * sizeof(double));
    if (kayNodes && Q.total(2)) D2H(c, kayNodes, Q.kay, (size_t)Q.total(2) * QKR_N * sizeof(double));
    if (kayOff) memcpy(kayOff, Q.off.data() + 2 * ((size_t)Q.nDesign + 1), ((size_t)Q.nDesign + 1) * sizeof(int64_t));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// virtual offsets of the sets s = d * nCase + c over a per-design offset array: set s starts at nCase * off[d] + c * n_d
static std::vector<int64_t> set_offsets(const int64_t *off, int nDesign, int nCase) {
    std::vector<int64_t> v((size_t)nDesign * nCase + 1);
    for (int d = 0; d < nDesign; d++)
        for (int ic = 0; ic < nCase; ic++) v[(size_t)d * nCase + ic] = off[d] * nCase + ic * (off[d + 1] - off[d]);
    v[(size_t)nDesign * nCase] = off[nDesign] * nCase;
    return v;
}

extern "C" int raftx_qtf_tables_kay_items(raftx_ctx *c, int nCase, const double *beta, int64_t *itemOff, double *items) {
    if (!c) return -1;
    const QtfResident &Q = c->qt;
    if (!Q.valid) FAIL(c, "qtf_tables_kay_items: no resident tables (raftx_qtf_tables_build first)");
    if (nCase < 1 || !beta) FAIL(c, "qtf_tables_kay_items: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nSet = (size_t)Q.nDesign * nCase, nItem = (size_t)Q.total(3) * nCase;
    if (itemOff) {
        const std::vector<int64_t> v = set_offsets(Q.off.data() + 3 * ((size_t)Q.nDesign + 1), Q.nDesign, nCase);
        memcpy(itemOff, v.data(), v.size() * sizeof(int64_t));
    }
    if (!items || !nItem) return 0;
    Scratch sc(c);
    double *dB = sc.in<double>(beta, nCase), *dI = sc.out<double>(items, nItem * QK_N);
    if (int rc = sc.upload("qtf_tables_kay_items")) return rc;
    if (sc.begin()) return -2;
    hipLaunchKernelGGL(k_qtfgen_kay_items, dim3((unsigned)nSet), dim3(64), 0, c->stream, nCase, Q.nDesign, dB, Q.dOff, Q.kay, dI);
    return sc.finish();
}

extern "C" int raftx_qtf_slender_resident(raftx_ctx *c, int nCase, int nw2, const double *w2, const double *k2, double depth,
                                          double rho, double g, const raftx_c128 *Xi, const double *beta, const double *Mstruc,
                                          int Nm, raftx_c128 *qtf) {
    if (!c) return -1;
    const QtfResident &Q = c->qt;
    if (!Q.valid) FAIL(c, "qtf_slender_resident: no resident tables (raftx_qtf_tables_build first)");
    if (nCase < 1 || nw2 < 1 || !w2 || !k2 || !beta || !Mstruc) FAIL(c, "qtf_slender_resident: bad arguments");
    if (Nm < 0 || Nm + 2 > KAY_MAXN) FAIL(c, "qtf_slender_resident: Nm=%d outside 0..%d", Nm, KAY_MAXN - 2);
    const int nDesign = Q.nDesign;
    const size_t nSet = (size_t)nDesign * nCase;
    if (!Xi && (!c->rXi || !c->have_cases || c->r_npair != nSet || c->T.nCase != nCase))
        FAIL(c, "qtf_slender_resident: Xi == NULL asks for the RAOs of the resident responses, but %s",
             !c->rXi ? "nothing is resident" : "the resident (design, case) pairs are not these designs x sea states");
    const size_t nStrip = (size_t)Q.total(0) * nCase, nMem = (size_t)Q.total(1) * nCase;
    const size_t nItem = Nm > 0 ? (size_t)Q.total(3) * nCase : 0;
    if (nStrip + nMem + nSet >= ((size_t)1 << 31)) FAIL(c, "qtf_slender_resident: %zu strips x sea states in one batch: cut it", nStrip);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nD1 = (size_t)nDesign + 1, nq = nSet * nw2 * nw2 * 6;
    const std::vector<int64_t> soff = set_offsets(Q.off.data(), nDesign, nCase), moff = set_offsets(Q.off.data() + nD1, nDesign, nCase),
                               ioff = set_offsets(Q.off.data() + 3 * nD1, nDesign, nCase);
    std::vector<double> hB(nSet), hMs(nSet * 36);
    for (size_t s = 0; s < nSet; s++) {
        hB[s] = beta[s % nCase];
        memcpy(&hMs[s * 36], Mstruc + (s / nCase) * 36, 36 * sizeof(double));
    }
    // bytes of device scratch this batch asks for (the tables of k_qtf_tables dominate), for the message of a failure
    const size_t bytes = 16 * ((size_t)nw2 * (2 * nStrip * QT_N + nMem * QTM_N + nSet * (QTS_N + 6)) + nItem * KAY_ROWS * (size_t)nw2) +
                         8 * (nStrip * (QD_N + 1) + nMem + nSet * 39 + nItem * QK_N) + 16 * nq * (nItem ? 2 : 1);
    Scratch sc(c);
    QtfArgs A;
    A.nSet = (int)nSet; A.nw = nw2; A.depth = depth; A.rho = rho; A.g = g;
    double *dw = sc.in<double>(w2, nw2), *dk = sc.in<double>(k2, nw2), *dB = sc.in<double>(hB.data(), nSet), *dBc = sc.in<double>(beta, nCase),
           *dMs = sc.in<double>(hMs.data(), nSet * 36);
    int64_t *dso = sc.in<int64_t>(soff.data(), nSet + 1), *dmo = sc.in<int64_t>(moff.data(), nSet + 1), *dio = sc.in<int64_t>(ioff.data(), nSet + 1);
    const size_t nXi = nSet * 6 * nw2;                   // the motion RAOs: the caller's, or k_rao_to_grid's below
    cplx *dXi = Xi ? sc.in<cplx>(Xi, nXi) : sc.tmp<cplx>(nXi);
    int *dss = sc.tmp<int>(nStrip), *dsr = sc.tmp<int>(nStrip), *dms = sc.tmp<int>(nMem), *dmr = sc.tmp<int>(nMem);
    cplx *dT = sc.tmp<cplx>(nStrip * QT_N * nw2), *dTM = sc.tmp<cplx>(nMem * QTM_N * nw2), *dTS = sc.tmp<cplx>(nSet * QTS_N * nw2);
    double *dD = sc.tmp<double>(nStrip * QD_N);
    cplx *dTA = sc.tmp<cplx>(nStrip * QT_N * nw2);
    double *dI = sc.tmp<double>(nItem * QK_N), *dq = sc.tmp<double>(nw2);
    cplx *dH = sc.tmp<cplx>(nItem * KAY_ROWS * nw2);
    bool ok = !sc.failed;
    if (ok && nSet && grow_device(c, c->rQtf, nq)) ok = false;
    if (ok && nItem && grow_device(c, c->rKay, nq)) ok = false;
    if (!ok)
        FAIL(c, "qtf_slender_resident: device allocation failed: %zu bytes of scratch asked for (%zu sets, %zu per set): cut the batch",
             bytes, nSet, nSet ? bytes / nSet : (size_t)0);
    c->rQtf_sets = (int)nSet;
    c->rQtf_nw2 = nw2;
    c->kay_ready = false;                                // the table below belongs to this call alone
    if (!nSet) return 0;
    sc.out_from(qtf, c->rQtf.p, nq);
    if (int rc = sc.upload("qtf_slender_resident")) return rc;
    if (nItem) HIPCHK(c, hipMemsetAsync(c->rKay.p, 0, nq * sizeof(cplx), c->stream));       // lower triangle stays zero
    A.w = dw; A.k = dk; A.soff = dso; A.strips = Q.strips; A.moff = dmo; A.members = Q.members; A.sset = dss; A.mset = dms;
    A.srec = dsr; A.mrec = dmr;
    A.Xi = dXi; A.beta = dB; A.Ms = dMs; A.kay = nItem ? c->rKay.p : nullptr; A.T = dT; A.TA = dTA; A.D = dD; A.TM = dTM; A.TS = dTS;
    A.qtf = c->rQtf.p;
    A.row_off = 0; A.row_stride = 1; A.nrow = nw2;
    if (sc.begin()) return -2;
    hipLaunchKernelGGL(k_qtfgen_sets, dim3((unsigned)nSet), dim3(64), 0, c->stream, nCase, nDesign, Q.dOff, dss, dsr, dms, dmr);
    if (nItem) {
        hipLaunchKernelGGL(k_qtfgen_kay_items, dim3((unsigned)nSet), dim3(64), 0, c->stream, nCase, nDesign, dBc, Q.dOff, Q.kay, dI);
        hipLaunchKernelGGL(k_kay_tables, dim3((unsigned)nItem), dim3(128), 0, c->stream, nw2, Nm + 2, (int)nSet, depth, dk, dio, dI, dB, dH, dq);
        hipLaunchKernelGGL(k_kay_pairs, dim3((unsigned)(nSet * nw2)), dim3(nw2 > 64 ? 128 : 64), 0, c->stream, nw2, Nm, depth, rho, g, dw,
                           dk, dio, dI, dH, dq, c->rKay.p);
    }
    if (!Xi)                                             // motion RAOs straight from the resident first-order responses
        hipLaunchKernelGGL(k_rao_to_grid, dim3((unsigned)(nSet * 6)), dim3(128), 0, c->stream, c->T.nCase, c->T.nHead, c->T.nw, nw2,
                           c->T.w, c->T.zeta, dw, c->rXi, dXi);
    hipLaunchKernelGGL(k_qtf_tables, dim3((unsigned)(nStrip + nMem + nSet)), dim3(nw2 > 128 ? 256 : 128), 0, c->stream, A, (int)nStrip,
                       (int)nMem);
    {
        const int blk = nw2 > 64 ? 128 : 64;
        const size_t per_xcd = (nSet * A.nrow + 7) / 8;  // see k_qtf_pairs: a slab of the (set, row) list per XCD
        hipLaunchKernelGGL(k_qtf_pairs, dim3((unsigned)(per_xcd * 8)), dim3(blk), 0, c->stream, A);
    }
    return sc.finish();
}

static void launch_modal(hipStream_t st, int n, const double *M, const double *C, const double *dM, const double *dC,
                         const double *props_in, double *props_out, double *fn, double *modes, int32_t *flags) {
    ModalArgs A{n, M, C, dM, dC, props_in, props_out, fn, modes, flags};
    hipLaunchKernelGGL(k_modal, dim3((unsigned)(((size_t)n + MODAL_BS - 1) / MODAL_BS)), dim3(MODAL_BS), 0, st, A);
}
// The eigen analysis of one block of a crossing (raftx_sweep_modal) on stream st, which is behind whatever wrote the
// block's summed M0 / C0 (k_geom_addup, k_geom_design with the add-up folded in, or the generating fused kernel): one
// system per lane, the results written straight into the block's page-locked landing area (landing::modal), which
// raftx_sweep_wait copies out.
static hipError_t modal_block(raftx_ctx *sub, SweepSlot &S, int lo, int n, hipStream_t st) {
    const landing::Modal land = landing::modal((size_t)n, RAFTX_SP_N);
    hipError_t e = sub->pinModal.reserve(land.need);
    if (e != hipSuccess || n == 0) return e;
    if (S.modal.evUp) e = hipStreamWaitEvent(st, S.modal.evUp, 0);
    if (e != hipSuccess) return e;
    double *pm = sub->pinModal.p;
    launch_modal(st, n, sub->T.M0, sub->T.C0, S.modal.dM ? S.modal.dM + (size_t)lo * 36 : nullptr,
                 S.modal.dC ? S.modal.dC + (size_t)lo * 36 : nullptr, S.modal.props ? sub->g_props : nullptr, pm + land.props,
                 pm + land.fn, pm + land.modes, land.flags.in(pm));
    return hipGetLastError();
}

// (the launch raftx_current_loads shares: the n designs of the tables T, par = speed | cos | sin [3,nCur])
static void launch_current(hipStream_t st, const DevTables &T, int n, int nCur, const double *par, const double *Zref, double depth,
                           double shearExp, double *D) {
    CurrentArgs A{n, nCur, T.off, T.ds, T.dsi, par, Zref, depth, shearExp, D};
    hipLaunchKernelGGL(k_current_loads, dim3(current_grid(n, nCur)), dim3(64 * CUR_WAVES), 0, st, A);
}
// The current loads of one block of a crossing (raftx_sweep_current) on stream st, behind the block's statistics kernel:
// the block's strip tables are resident until the block is retired.  One wave per (design, tile of currents), the sums
// written straight into the block's page-locked landing area [n,nCur,6], which raftx_sweep_wait copies out.
static hipError_t current_block(raftx_ctx *sub, SweepSlot &S, int lo, int n, double depth, hipStream_t st) {
    hipError_t e = sub->pinCur.reserve((size_t)n * S.current.nCur * 6);
    if (e != hipSuccess || n == 0) return e;
    if (sub->T.nDesign != n || !sub->T.off || !sub->T.ds || !sub->T.dsi) return hipErrorInvalidValue;   // (the block kept no tables: internal error)
    e = hipStreamWaitEvent(st, S.current.evUp, 0);
    if (e != hipSuccess) return e;
    launch_current(st, sub->T, n, S.current.nCur, S.current.par, S.current.Zref ? S.current.Zref + lo : nullptr, depth,
                   S.current.shearExp, sub->pinCur.p);
    return hipGetLastError();
}

// k_sweep_channels on one block of a crossing, on stream st behind the event `up` of the request that asked for it: one
// workgroup per pair, the standard deviations of nChan channels written straight into the page-locked landing area
// [pairs,nChan] that raftx_sweep_wait copies out.  L and Gw (or null) at the block's first design; a zero stride: shared rows.
static hipError_t channel_rows_block(raftx_ctx *sub, const SweepSlot &S, int n, hipStream_t st, hipEvent_t up, int nChan, const double *L,
                                     size_t strideL, const cplx *Gw, size_t strideG, Pinned<double> &land) {
    const size_t npair = (size_t)n * S.nCase;
    hipError_t e = land.reserve(npair * nChan);
    if (e != hipSuccess || npair == 0) return e;
    if (!sub->rXi || sub->r_nx < npair * S.nHead * 6 * S.nw || !sub->T.w) return hipErrorInvalidValue;   // (no resident responses: internal error)
    e = hipStreamWaitEvent(st, up, 0);
    if (e != hipSuccess) return e;
    ChannelArgs A;
    A.nCase = S.nCase; A.nHead = S.nHead; A.nw = S.nw; A.nChan = nChan;
    A.strideL = strideL;
    A.strideG = strideG;
    const dim3 grid((unsigned)npair), wg = bin_threads(S.nw);
    if (Gw) hipLaunchKernelGGL(k_sweep_channels<true>, grid, wg, 0, st, A, (const double *)sub->T.w, (const cplx *)sub->rXi, L, Gw, land.p);
    else hipLaunchKernelGGL(k_sweep_channels<false>, grid, wg, 0, st, A, (const double *)sub->T.w, (const cplx *)sub->rXi, L, Gw, land.p);
    return hipGetLastError();
}
// The output channels of one block of a crossing (raftx_sweep_channels), behind the block's statistics kernel (and so behind
// everything that wrote the block's responses, the slabs of a crossing with responses out included).  Per-design rows are
// taken at the block's first design.
static hipError_t channels_block(raftx_ctx *sub, SweepSlot &S, int lo, int n, hipStream_t st) {
    const int nChan = S.channels.nChan;
    const size_t strideL = S.channels.nL > 1 ? (size_t)nChan * 18 : 0, strideG = S.channels.nG > 1 ? (size_t)nChan * 6 * S.nw : 0;
    return channel_rows_block(sub, S, n, st, S.channels.evUp, nChan, S.channels.L + (size_t)lo * strideL, strideL,
                              S.channels.Gw ? S.channels.Gw + (size_t)lo * strideG : nullptr, strideG, sub->pinChan);
}
// The tension statistics of one block of a crossing (raftx_sweep_mooring with T_std): k_sweep_channels once more, on the rows
// k_moor_design left in device memory (J in the first plane), into a landing area of its own -- a raftx_sweep_channels
// request on the same slot keeps its rows and its area.
static hipError_t mooring_std_block(raftx_ctx *sub, SweepSlot &S, int lo, int n, hipStream_t st) {
    const int nChan = 2 * S.mooring.nLine;
    const size_t strideL = (size_t)nChan * 18;
    return channel_rows_block(sub, S, n, st, S.mooring.evUp, nChan, S.mooring.Lr + (size_t)lo * strideL, strideL, nullptr, 0, sub->pinMoorT);
}
// C_moor into the C0 of block b (raftx_sweep_mooring with add_stiffness): on the copy stream, which is in order -- behind the
// block's own upload of C0 and behind the mooring kernels of the request -- and ahead of everything that reads C0: the
// generation stream and the ctx stream (k_geom_addup, the add-up inside k_geom_design, the generating fused kernel) wait for it.
static int mooring_add_block(raftx_ctx *c, raftx_ctx *sub, SweepSlot &S, int lo, int n, bool pipelined) {
    if (!n) return 0;
    if (!sub->job.active || !sub->job.C0d) FAIL(sub, "sweep_mooring: the block has no uploaded C0 (internal error)");
    HIPCHK(sub, sub->evMoor.ensure(hipEventDisableTiming));
    hipLaunchKernelGGL(k_moor_add, dim3(moor_grid((long long)n * 36)), dim3(MOOR_THREADS), 0, c->sCopy, sub->job.C0d,
                       S.mooring.C + (size_t)lo * 36, (long long)n * 36);
    HIPCHK(sub, hipGetLastError());
    HIPCHK(sub, hipEventRecord(sub->evMoor, c->sCopy));
    HIPCHK(sub, hipStreamWaitEvent(c->stream, sub->evMoor, 0));
    if (pipelined && c->sGen) HIPCHK(sub, hipStreamWaitEvent(c->sGen, sub->evMoor, 0));
    return 0;
}

// The stream the responses of a crossing are downloaded on: one of the HIGHEST priority class, created when first needed (so
// late, it does not move the other streams' hardware queues).  A priority class has hardware queues of its own and the highest
// is served at once: the copy never sits in a queue with the next batch's kernels (ordinary stream) nor starts a step late
// (lowest class): profiles/MEASUREMENT_HISTORY.md, "Closed scheduling experiments of the crossing".  A device with one class,
// or a failed creation: the ordinary download stream.
static hipStream_t download_stream(raftx_ctx *c) {
    (void)c->sD2Hhigh.ensure_highest(hipStreamNonBlocking);
    return c->sD2Hhigh ? c->sD2Hhigh : c->sD2H;
}

// Statistics, iteration counts and flags of block b go straight into its page-locked landing area (the kernels store there:
// no small D2H copy that could queue on the DMA engine behind a bulk download), on the ctx stream behind the block's fused
// launch; behind them, on the download stream, the block's responses unless they leave slab by slab.
static int enqueue_stats(raftx_ctx *c, SweepSlot &S, size_t b, hipStream_t sDown) {
    raftx_ctx *sub = S.blk[b];
    const int lo = S.bnd[b], nCase = S.nCase, nHead = S.nHead, nw = S.nw;
    const size_t npair = (size_t)(S.bnd[b + 1] - lo) * nCase;
    hipError_t e = hipEventRecord(sub->evS0, c->stream);
    if (npair) {
        const landing::Stats land = landing::stats(npair);              // (niter and flags: one run of 2 npair ints, from niter on)
        hipLaunchKernelGGL(k_motion_stats, dim3((unsigned)npair), bin_threads(nw), 0, c->stream,
                           (int)npair, nHead, nw, 1.0 / S.dw, sub->rXi, sub->pinRes.p + land.sd, (double *)nullptr, (const int *)sub->rNi,
                           (const int *)sub->rFl, land.niter.in(sub->pinRes.p));
    }
    if (e == hipSuccess) e = hipEventRecord(sub->evS1, c->stream);
    if (e == hipSuccess && S.modal.on) e = modal_block(sub, S, lo, S.bnd[b + 1] - lo, c->stream);
    if (e == hipSuccess && S.current.on) e = current_block(sub, S, lo, S.bnd[b + 1] - lo, c->csets[S.cset].T.depth, c->stream);
    if (e == hipSuccess && S.channels.on) e = channels_block(sub, S, lo, S.bnd[b + 1] - lo, c->stream);
    if (e == hipSuccess && S.mooring.on && S.mooring.Tstd_out) e = mooring_std_block(sub, S, lo, S.bnd[b + 1] - lo, c->stream);
    if (e == hipSuccess) e = hipEventRecord(sub->evDone, c->stream);
    if (e == hipSuccess && S.Xi && !S.slab) {
        e = hipStreamWaitEvent(sDown, sub->evDone, 0);
        if (e == hipSuccess && sub->r_nx)
            e = hipMemcpyAsync(S.Xi + (size_t)lo * nCase * nHead * 6 * nw, sub->rXi, sub->r_nx * sizeof(cplx), hipMemcpyDeviceToHost, sDown);
    }
    if (e != hipSuccess) {
        snprintf(sub->err, sizeof(sub->err), "statistics / download of the block: %s", hipGetErrorString(e));
        return -2;
    }
    return 0;
}

// Responses wanted and nothing else in flight: the launch of block b is cut into slabs of the pair list on the slab
// stream(s), each followed by its own download (SlabPlan).  The download (3.5 ms for 192 MB) is longer than the solve, so
// the call ends one slab's download after the last slab when the first download starts early and the copy engine is then
// never left waiting.  Measured (profiles/DESIGN_HISTORY_r01-r05.md, 10 000 pairs, one box, median of six calls): whole
// blocks 7.7 ms; slabs of 512 / 768 / 1024 / 1536 pairs on one slab stream 7.9 / 6.2 / 5.7 / 6.1 -- one residency round per
// slab (256 CUs x 4 pairs) -- and no better on two or three streams (6.0-6.3).  RAFTX_XI_SLAB_PAIRS: pairs per slab (0: whole
// blocks); RAFTX_XI_SLAB_STREAMS: 1 .. 3.
static void slab_plan_block(SlabPlan &plan, SweepSlot &S, size_t b, size_t slab_pairs, hipStream_t sDown) {
    raftx_ctx *sub = S.blk[b];
    const size_t npair = (size_t)(S.bnd[b + 1] - S.bnd[b]) * S.nCase;
    plan.bnd.clear();
    for (size_t p = 0; p < npair; p += slab_pairs) plan.bnd.push_back(p);
    if (plan.bnd.size() > 1 && npair - plan.bnd.back() < slab_pairs / 2) plan.bnd.pop_back();   // no sliver at the end
    plan.bnd.push_back(npair);
    size_t *kslab = &S.nSlabEv;
    S.nSlabEv = 0;
    const size_t per = (size_t)S.nHead * 6 * S.nw;
    raftx_c128 *out = S.Xi + (size_t)S.bnd[b] * S.nCase * per;
    plan.after = [=](size_t q0, size_t q1, hipStream_t s) -> int {
        if (q1 <= q0) return 0;
        while (sub->evSlab.size() <= *kslab) {
            Event e;
            if (e.ensure(hipEventDisableTiming) != hipSuccess) return -2;
            sub->evSlab.push_back(std::move(e));
        }
        hipEvent_t e = sub->evSlab[(*kslab)++];
        if (hipEventRecord(e, s) != hipSuccess || hipStreamWaitEvent(sDown, e, 0) != hipSuccess) return -2;
        return hipMemcpyAsync(out + q0 * per, sub->rXi + q0 * per, (q1 - q0) * per * sizeof(cplx), hipMemcpyDeviceToHost, sDown) ==
                       hipSuccess ? 0 : -2;
    };
}

// what raftx_sweep_launch decides once for all blocks of a crossing (with SweepSlot::slab): other crossings are prepared or
// solving | the download stream, or null: no responses asked for | pairs per slab and the plan of the block being launched
struct LaunchMode { bool pipelined; hipStream_t sDown; size_t slab_pairs; SlabPlan plan; };
// the streams the slabs go to: the generation stream first, then the two slab streams (created when first needed)
static int slab_streams(raftx_ctx *c, int n, SlabPlan &plan) {
    Stream *ss[3] = {&c->sGen, &c->sSlab[0], &c->sSlab[1]};
    for (int i = 0; i < n; i++) {
        HIPCHK(c, ss[i]->ensure(hipStreamNonBlocking));
        plan.alts.push_back(*ss[i]);
    }
    return 0;
}
// deferred phase 1: keeps one block's upload ahead of block b, the block being launched (whose err takes the text)
static int phase1_ahead(raftx_ctx *c, SweepSlot &S, size_t b) {
    if (S.next_p1 >= S.blk.size() || S.next_p1 > b + 1) return 0;
    size_t bn = 0;
    const int rc = block_phase1_next(c, S, &bn);
    if (rc) snprintf(S.blk[b]->err, sizeof(S.blk[b]->err), "%s", S.blk[bn]->err);
    return rc;
}
// A crossing launched while another one is solving generates its tables on the generation stream: its member pass ran
// a step earlier (raftx_sweep_prepare), so the tables can be built in the drain of the running fused kernel.  (The
// blocks of an isolated crossing wait for their descriptor upload: everything on the ctx stream,
// profiles/r02_crossing_splits.txt.)  Enqueued now, beside a fused kernel that has only just started, the generation
// would be dispatched at once and take LDS from that kernel for its whole run (measured: +0.25 ms on the kernel).  A
// small kernel queued BEHIND a running big grid is dispatched when that grid has been handed out -- which is when
// the member pass of the batch prepared last gets onto the chip: the generation waits for that batch's first
// kernel and so runs in the drain, beside that member pass.
static int gate_generation(raftx_ctx *c, int slot) {
    for (int sl = 0; sl < RAFTX_NSLOT; sl++)
        if (sl != slot && c->slots[sl].prepared && !c->slots[sl].blk.empty() && c->slots[sl].blk[0])
            if (hipStreamWaitEvent(c->sGen, c->slots[sl].blk[0]->evZ, 0) != hipSuccess) return -2;
    return 0;
}
// the sea states a crossing was prepared with (the pinned set P of the parent) become those of a block's tables
static void hand_sea_states(const DevTables &P, raftx_ctx *sub) {
    DevTables &T = sub->T;
    T.nCase = P.nCase; T.nHead = P.nHead; T.nw = P.nw;
    T.w = P.w; T.k = P.k; T.csh = P.csh; T.cch = P.cch; T.zeta = P.zeta; T.beta = P.beta;
    T.depth = P.depth; T.rho = P.rho; T.g = P.g;
    sub->have_cases = true;
}
// Phase 2 + fixed point + statistics of block b on the ctx stream, behind the blocks before it (the scheduling variants that
// lost -- a second compute stream among them: profiles/MEASUREMENT_HISTORY.md, "Closed scheduling experiments of the crossing").
static int launch_block(raftx_ctx *c, SweepSlot &S, int slot, size_t b, LaunchMode &M) {
    raftx_ctx *sub = S.blk[b];
    // (C_moor into this block's C0 first: on the copy stream ahead of the next block's uploads)
    int rc = (S.mooring.on && S.mooring.add) ? mooring_add_block(c, sub, S, S.bnd[b], S.bnd[b + 1] - S.bnd[b], M.pipelined) : 0;
    if (!rc) rc = phase1_ahead(c, S, b);
    if (!rc && b == 0 && M.pipelined) rc = gate_generation(c, slot);
    S.tlb.push_back(S.since());
    // (a crossing: no ABI copy of the strip records; with RAFTX_FUSED_GEN=1 the tables are left to the fused kernel itself,
    // raftx_fusedgen.h -- build_phase2 / solve_enqueue decide)
    // (a crossing with current loads reads the tables after the solve: they are never left to the fused kernel)
    // (nor with a mean-pose request: the second member pass is the plain one, and so is the generation)
    const int kind = GEN_CROSSING | ((S.nCase == 1 && !S.slab && !S.current.on && !S.pose.on) ? GEN_MAY_DEFER : 0) | (M.pipelined ? GEN_PIPELINED : 0);
    if (!rc) rc = build_phase2(sub, nullptr, M.pipelined ? c->sGen : nullptr, kind);
    S.tlb.push_back(S.since());
    if (!rc) {
        hand_sea_states(c->csets[S.cset].T, sub);
        if (S.slab) slab_plan_block(M.plan, S, b, M.slab_pairs, M.sDown);
        rc = solve_enqueue(sub, S.nIter, S.tol, S.XiStart, nullptr, 0, S.slab ? &M.plan : nullptr);
        if (!rc) c->last_persist = sub->last_persist, c->last_grid = sub->last_grid, c->last_pairs = sub->last_pairs;
    }
    if (!rc && sub->pinRes.reserve(landing::stats((size_t)(S.bnd[b + 1] - S.bnd[b]) * S.nCase).need) != hipSuccess) rc = -2;
    if (!rc && !S.slab) rc = enqueue_stats(c, S, b, M.sDown);         // (slab mode: stats_after_join)
    S.tlb.push_back(S.since());
    if (rc) snprintf(c->err, sizeof(c->err), "sweep_stats (block %zu): %s", b, sub->err);
    return rc;
}
// slab mode: the statistics read what the slabs wrote, so they go behind all of them, joined into the ctx stream
static int stats_after_join(raftx_ctx *c, SweepSlot &S, LaunchMode &M) {
    const size_t nB = S.blk.size();
    if (!nB) return 0;
    if (S.blk[0]->evJoin.ensure(hipEventDisableTiming) != hipSuccess) return -2;
    if (int rc = slab_join(S.blk[0], c->stream, M.plan.alts)) return rc;
    if (hipEventRecord(S.blk[nB - 1]->ev1, c->stream) != hipSuccess) return -2;
    for (size_t b = 0; b < nB; b++)
        if (int rc = enqueue_stats(c, S, b, M.sDown)) {
            snprintf(c->err, sizeof(c->err), "sweep_stats (block %zu): %s", b, S.blk[b]->err);
            return rc;
        }
    return 0;
}

extern "C" int raftx_sweep_launch(raftx_ctx *c, int slot) {
    RangeScope range_("raftx_sweep_launch: generation + fused fixed point + statistics (enqueue)");
    if (!c) return -1;
    SLOT_REF(S, c, slot, "sweep_launch");
    if (!S.prepared) FAIL(c, "sweep_launch: nothing prepared on slot %d (raftx_sweep_prepare first)", slot);
    if (S.cset < 0 || c->csets[S.cset].T.nCase != S.nCase || c->csets[S.cset].T.nHead != S.nHead || c->csets[S.cset].T.nw != S.nw)
        FAIL(c, "sweep_launch: slot %d has lost its sea-state tables (internal error)", slot);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->evEpoch) {
        HIPCHK(c, c->evEpoch.ensure());
        HIPCHK(c, hipEventRecord(c->evEpoch, c->stream));
    }
    S.prepared = false;                                 // from here on every failure goes through sweep_fail_drain
    // ---- full responses, if asked for: every block's download is enqueued right behind the block's kernels (after ALL blocks,
    // the first download of an isolated call waited for the host to see the member pass of the LAST block: 1.6 ms late)
    static const long slab_pairs = getenv("RAFTX_XI_SLAB_PAIRS") ? atol(getenv("RAFTX_XI_SLAB_PAIRS")) : 1024;
    static const int slab_streams_n = getenv("RAFTX_XI_SLAB_STREAMS") ? std::min(3, std::max(1, atoi(getenv("RAFTX_XI_SLAB_STREAMS")))) : 1;
    LaunchMode M{others_in_flight(c, slot), S.Xi ? download_stream(c) : nullptr, (size_t)slab_pairs, {}};
    S.slab = S.Xi && M.sDown && slab_pairs > 0 && !M.pipelined;
    S.tlb.clear();
    int rc = S.slab ? slab_streams(c, slab_streams_n, M.plan) : 0;
    for (size_t b = 0; b < S.blk.size() && !rc; b++) rc = launch_block(c, S, slot, b, M);
    if (!rc && S.slab) rc = stats_after_join(c, S, M);
    if (!rc && S.Xi && hipEventRecord(S.evXi, M.sDown) != hipSuccess) rc = -2;
    if (rc) return sweep_fail_drain(c, S, rc);
    S.tl[2] = S.since();
    S.busy = true;
    return 0;
}

// raftx_sweep_submit = prepare + launch (the two-call form the earlier rounds had)
extern "C" int raftx_sweep_submit(raftx_ctx *c, int slot, int nDesign, const int64_t *memberOff, const double *members,
                                  const int64_t *stationOff, const double *stations, const int64_t *capOff,
                                  const double *caps, const double *pose, double rho, double g, int add_mask,
                                  const double *M0, const double *B0, const double *C0, const double *Fz_moor, int nCase,
                                  int nHead, int nw, const double *w, const double *k, double depth, double rho_wave,
                                  double g_wave, const double *zeta, const double *beta, int nIter, double tol,
                                  double XiStart, int nChunk, double *sd, int32_t *niter, int32_t *flags,
                                  raftx_c128 *Xi, int64_t *stripOffsets) {
    const int rc = raftx_sweep_prepare(c, slot, nDesign, memberOff, members, stationOff, stations, capOff, caps, pose, rho, g, add_mask,
                                       M0, B0, C0, Fz_moor, nCase, nHead, nw, w, k, depth, rho_wave, g_wave, zeta, beta, nIter, tol,
                                       XiStart, nChunk, sd, niter, flags, Xi, stripOffsets);
    if (rc) return rc;
    return raftx_sweep_launch(c, slot);
}

// Retires a crossing that was prepared and will not be launched: its uploads and member pass are drained, its scratch and
// sea-state set released; the output arrays given at prepare time are not touched.
extern "C" int raftx_sweep_cancel(raftx_ctx *c, int slot) {
    if (!c) return -1;
    SLOT_REF(S, c, slot, "sweep_cancel");
    if (S.busy) FAIL(c, "sweep_cancel: slot %d has been launched (raftx_sweep_wait collects it)", slot);
    if (!S.prepared) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    hipError_t e = hipSuccess;
    for (hipStream_t st : {c->sCopy.s, c->sPrep.s})
        if (st && e == hipSuccess) e = hipStreamSynchronize(st);
    for (raftx_ctx *sub : S.blk)
        if (sub) {
            if (sub->sAux && e == hipSuccess) e = hipStreamSynchronize(sub->sAux);
            build_abandon(sub);
        }
    S.prepared = false;
    S.clear_requests();
    slot_release_cases(c, S);
    HIPCHK(c, e);
    return 0;
}

// Waits for the last block's statistics (the ctx stream is in order: all blocks are done), then for the responses.  Either
// way the sea-state set is released; a failure also drains the device and abandons the jobs of the blocks.
static hipError_t sweep_drain(raftx_ctx *c, SweepSlot &S) {
    hipError_t es = S.blk.empty() ? hipSuccess : hipEventSynchronize(S.blk.back()->evDone);
    S.tl[3] = S.since();
    if (es == hipSuccess && S.Xi) es = hipEventSynchronize(S.evXi);
    if (es == hipSuccess) es = hipGetLastError();
    if (es == hipSuccess) slot_release_cases(c, S);
    else (void)sweep_fail_drain(c, S, -2);
    return es;
}
// ms from one event to another, best effort: a timing query must not lose the results of work that has been waited for.
// On an error the value is zero, *ok (if given) is cleared, and the error does not stay behind for a later call to find.
static double elapsed_ms(hipEvent_t from, hipEvent_t to, bool *ok = nullptr) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, from, to) == hipSuccess) return ms;
    (void)hipGetLastError();
    if (ok) *ok = false;
    return 0.0;
}
// where the fused launches of the crossing ran, ms since the ctx epoch (both zero: no span)
static void solve_span(raftx_ctx *c, SweepSlot &S) {
    S.span[0] = S.span[1] = 0;
    if (S.blk.empty() || !c->evEpoch) return;
    bool ok = true;
    const double a = elapsed_ms(c->evEpoch, S.blk[0]->ev0, &ok), b = elapsed_ms(c->evEpoch, S.blk.back()->ev1, &ok);
    if (ok) { S.span[0] = a; S.span[1] = b; }
}
// Block b of a crossing that has been waited for: its kernel times into t [.., generation, solve, statistics], its strip
// offsets and landing areas out to the caller's arrays, its job retired.
static void collect_block(SweepSlot &S, size_t b, double *t) {
    raftx_ctx *sub = S.blk[b];
    const int lo = S.bnd[b], n = S.bnd[b + 1] - lo;
    const size_t npair = (size_t)n * S.nCase, p0 = (size_t)lo * S.nCase, nB = S.blk.size();
    // slabs on their own streams: the span from the first block's first launch to the last slab's end (the generation
    // of the later blocks runs inside it)
    if (!S.slab) t[2] += elapsed_ms(sub->ev0, sub->ev1);
    else if (b + 1 == nB) t[2] += elapsed_ms(S.blk[0]->ev0, sub->ev1);
    t[3] += elapsed_ms(sub->evS0, sub->evS1);
    if (S.stripOffsets)                                                 // block-relative offsets of phase 1 -> batch offsets
        for (int i = 0; i < n; i++) S.stripOffsets[lo + i + 1] = S.stripOffsets[lo] + sub->pin.p[PIN_OFF + i + 1];
    if (sub->job.active) t[1] += elapsed_ms(sub->evG2, sub->evG3) + elapsed_ms(sub->evG0, sub->evG1);   // (as build_retire)
    build_abandon(sub);
    const landing::Stats land = landing::stats(npair);
    const double *res = sub->pinRes.p;
    memcpy(S.sd + p0 * 6, res + land.sd, npair * 6 * sizeof(double));
    memcpy(S.niter + p0, land.niter.in(res), npair * sizeof(int));
    memcpy(S.flags + p0, land.flags.in(res), npair * sizeof(int));
    S.modal.collect(sub->pinModal.p, lo, n, S.nCase);
    S.current.collect(sub->pinCur.p, lo, n, S.nCase);
    S.channels.collect(sub->pinChan.p, lo, n, S.nCase);
    S.mooring.collect(sub->pinMoorT.p, lo, n, S.nCase);                 // (the pose request has nothing per block: collect_pose)
}
// the crossing's mooring results out of their landing area (the copies were waited for with the crossing: sCopy is ahead of
// every block through evUp, or waited for here)
static hipError_t collect_mooring(SweepSlot &S) {
    if (!S.mooring.on) return hipSuccess;
    const hipError_t e = hipEventSynchronize(S.mooring.evUp);
    if (e != hipSuccess) return e;
    const size_t n = S.bnd.empty() ? 0 : (size_t)S.bnd.back(), nT = 2 * (size_t)S.mooring.nLine;
    const landing::Mooring land = landing::mooring(n, (size_t)S.mooring.nLine);
    const double *p = S.mooring.pin.p;
    rows_out(S.mooring.C_out, p + land.C, 0, n, 36);
    rows_out(S.mooring.F_out, p + land.F, 0, n, 6);
    rows_out(S.mooring.T_out, p + land.T, 0, n, nT);
    memcpy(S.mooring.flags_out, land.flags.in(p), n * sizeof(int32_t));
    return hipSuccess;
}
// The solve's outputs out of their landing area (k_pose_place wrote them ahead of the block's second member pass, which the
// crossing has been waited for through), and the pose-flagged designs: such a design was solved at the reference pose so that
// its block could go on, and nothing of that may pass for a result -- everything handed out for it becomes NaN and its
// flags take RAFTX_FLAG_NAN.  Host work after the copies: no other design's bits change.
static void collect_pose(SweepSlot &S) {
    if (!S.pose.on) return;
    const size_t n = S.bnd.empty() ? 0 : (size_t)S.bnd.back(), nC = (size_t)S.nCase;
    const landing::Pose land = landing::pose(n);
    const double *p = S.pose.pin.p;
    const int32_t *fl = land.flags.in(p);
    rows_out(S.pose.pose_out, p + land.pose, 0, n, 6);
    rows_out(S.pose.Fres_out, p + land.Fres, 0, n, 6);
    if (S.pose.iter_out) memcpy(S.pose.iter_out, land.iterations.in(p), n * sizeof(int32_t));
    memcpy(S.pose.flags_out, fl, n * sizeof(int32_t));
    for (size_t d = 0; d < n; d++) {
        if (!fl[d]) continue;
        blank_row(S.sd, d, nC * 6);
        for (size_t i = 0; i < nC; i++) S.flags[d * nC + i] |= RAFTX_FLAG_NAN;
        blank_row(reinterpret_cast<double *>(S.Xi), d, nC * S.nHead * 6 * S.nw * 2);
        S.modal.blank(d, nC);
        S.current.blank(d, nC);
        S.channels.blank(d, nC);
        S.mooring.blank(d, nC);
    }
}
// RAFTX_SWEEP_DEBUG: the host's timeline of the crossing on stderr
static void debug_timeline(const SweepSlot &S, int slot, double wall) {
    static const bool dbg_host = getenv("RAFTX_SWEEP_DEBUG") != nullptr;
    if (!dbg_host) return;
    fprintf(stderr, "[raftx_sweep slot %d] host ms since submit: pre %.3f | phase-1 enqueued %.3f | phase-2 enqueued %.3f | ctx stream "
            "reached the end %.3f | done %.3f\n", slot, S.tl[0], S.tl[1], S.tl[2], S.tl[3], wall);
    if (S.tlb.size() <= 3) return;
    fprintf(stderr, "[raftx_sweep slot %d] launch loop, host ms per block (next upload enqueued | totals seen | block enqueued):", slot);
    for (size_t i = 0; i + 2 < S.tlb.size(); i += 3) fprintf(stderr, "  %.3f %.3f %.3f", S.tlb[i], S.tlb[i + 1], S.tlb[i + 2]);
    fprintf(stderr, "\n");
}

// Two ways out of a busy slot: the drain failed (-2; nothing copied, blocks abandoned) or not (0; every block collected and
// retired, whatever the timing queries said).  Both leave the slot idle, without eigen-analysis / current-load requests.
extern "C" int raftx_sweep_wait(raftx_ctx *c, int slot, double *timing_ms) {
    RangeScope range_("raftx_sweep_wait: drain + outputs");
    if (!c) return -1;
    SLOT_REF(S, c, slot, "sweep_wait");
    if (!S.busy) FAIL(c, "sweep_wait: nothing submitted on slot %d", slot);
    HIPCHK(c, hipSetDevice(c->device));
    S.busy = false;
    const hipError_t es = sweep_drain(c, S);
    if (es != hipSuccess) S.clear_requests();
    HIPCHK(c, es);
    solve_span(c, S);
    double t[4] = {0, 0, 0, 0};                           // wall | generation, solve, statistics kernels
    if (S.stripOffsets) S.stripOffsets[0] = 0;
    for (size_t b = 0; b < S.blk.size(); b++) collect_block(S, b, t);
    const hipError_t em = collect_mooring(S);
    if (em == hipSuccess) collect_pose(S);
    S.clear_requests();
    HIPCHK(c, em);
    t[0] = S.since();
    debug_timeline(S, slot, t[0]);
    if (timing_ms) memcpy(timing_ms, t, sizeof(t));
    c->last_ms = t[2];
    return 0;
}

extern "C" int raftx_sweep_solve_span(raftx_ctx *c, int slot, double *start_ms, double *end_ms) {
    if (!c) return -1;
    SLOT_REF(S, c, slot, "sweep_solve_span");
    if (S.busy) FAIL(c, "sweep_solve_span: slot %d has not been waited for", slot);
    if (start_ms) *start_ms = S.span[0];
    if (end_ms) *end_ms = S.span[1];
    return 0;
}

extern "C" int raftx_sweep_generation(raftx_ctx *c, int slot, int *blocks_fused, int *blocks) {
    if (!c) return -1;
    SLOT_REF(S, c, slot, "sweep_generation");
    int nf = 0, nb = 0;
    for (raftx_ctx *sub : S.blk)
        if (sub) {
            nb++;
            nf += sub->last_gen_fused ? 1 : 0;
        }
    if (blocks_fused) *blocks_fused = nf;
    if (blocks) *blocks = nb;
    return 0;
}

// ---- eigen analysis of rigid 6-DOF systems (include/raftx_modal.h, raftx_modal.h)
static int modal_launch(raftx_ctx *c, int n, const double *M, const double *C, const double *dM, const double *dC,
                        const double *props_in, double *fn, double *modes, int32_t *flags, double *props) {
    Scratch sc(c);
    double *dfn = sc.out<double>(fn, (size_t)n * 6), *dmo = sc.out<double>(modes, (size_t)n * 36);
    int32_t *dfl = sc.out<int32_t>(flags, (size_t)n);
    double *dpr = sc.out<double>(props, (size_t)n * RAFTX_SP_N);
    if (int rc = sc.upload("modal")) return rc;
    if (sc.begin()) return -2;
    launch_modal(c->stream, n, M, C, dM, dC, props_in, dpr, dfn, dmo, dfl);
    return sc.finish();
}

extern "C" int raftx_modal_batch(raftx_ctx *c, int n, const double *M, const double *C, double *fn, double *modes,
                                 int32_t *flags) {
    if (!c) return -1;
    if (n < 0 || (n > 0 && (!M || !C || !fn || !modes || !flags))) FAIL(c, "modal_batch: bad arguments");
    if (n == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    double *dM = sc.in<double>(M, (size_t)n * 36), *dC = sc.in<double>(C, (size_t)n * 36);
    if (int rc = sc.upload("modal_batch")) return rc;
    return modal_launch(c, n, dM, dC, nullptr, nullptr, nullptr, fn, modes, flags, nullptr);
}

extern "C" int raftx_modal_resident(raftx_ctx *c, const double *dM, const double *dC, double *fn, double *modes,
                                    int32_t *flags, double *props) {
    if (!c) return -1;
    if (!c->have_designs) FAIL(c, "modal_resident: no design set on this ctx (raftx_upload_designs / raftx_build_designs)");
    if (!fn || !modes || !flags) FAIL(c, "modal_resident: bad arguments");
    const int n = c->T.nDesign;
    if (props && (c->g_n != n || !c->g_props))
        FAIL(c, "modal_resident: props are generated by raftx_build_designs only (the resident set was uploaded)");
    if (n == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    double *ddM = sc.in<double>(dM, (size_t)n * 36), *ddC = sc.in<double>(dC, (size_t)n * 36);
    if (int rc = sc.upload("modal_resident")) return rc;
    return modal_launch(c, n, c->T.M0, c->T.C0, ddM, ddC, props ? c->g_props : nullptr, fn, modes, flags, props);
}

extern "C" int raftx_sweep_modal(raftx_ctx *c, int slot, const double *dM, const double *dC, double *fn, double *modes,
                                 int32_t *flags, double *props) {
    if (!c) return -1;
    SweepSlot *slot_ = nullptr;
    if (int rc = request_slot(c, slot, "sweep_modal", false, &slot_)) return rc;
    SweepSlot &S = *slot_;
    if (!fn || !modes || !flags) FAIL(c, "sweep_modal: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = S.bnd.empty() ? 0 : (size_t)S.bnd.back();
    const double *ddM = nullptr, *ddC = nullptr;
    if (upload_on(c, c->sCopy, S.allocs, dM, dM ? n * 36 : 0, &ddM) || upload_on(c, c->sCopy, S.allocs, dC, dC ? n * 36 : 0, &ddC))
        return -2;
    HIPCHK(c, S.modal.evUp.ensure(hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(S.modal.evUp, c->sCopy));
    S.modal.dM = ddM; S.modal.dC = ddC;
    S.modal.fn = fn; S.modal.modes = modes; S.modal.flags = flags; S.modal.props = props;
    S.modal.on = true;
    return 0;
}

// ---- mean current loads (include/raftx_current.h, raftx_current.h)
// speed | cos | sin [3,nCur] (+ Zref [nDesign]) checked and laid out for the kernel (raft_member.py:1848: the heading in
// degrees, cos / sin in libm precision on the host)
static int current_params(raftx_ctx *c, const char *who, int nCur, const double *speed, const double *heading_deg, const double *Zref,
                          size_t nDesign, double depth, double shearExp, std::vector<double> &host) {
    if (nCur <= 0) FAIL(c, "%s: nCur must be positive (got %d)", who, nCur);
    if (!speed || !heading_deg) FAIL(c, "%s: bad arguments", who);
    if (!std::isfinite(depth) || !std::isfinite(shearExp)) FAIL(c, "%s: depth and shearExp must be finite", who);
    host.resize((size_t)3 * nCur + (Zref ? nDesign : 0));
    for (int i = 0; i < nCur; i++) {
        if (!std::isfinite(speed[i]) || !std::isfinite(heading_deg[i])) FAIL(c, "%s: current %d has a non-finite speed or heading", who, i);
        const double h = heading_deg[i] * (3.14159265358979323846 / 180.0);      // np.deg2rad
        host[(size_t)i] = speed[i];
        host[(size_t)nCur + i] = cos(h);
        host[(size_t)2 * nCur + i] = sin(h);
    }
    for (size_t d = 0; d < nDesign; d++) {
        const double z = Zref ? Zref[d] : 0.0;
        if (!std::isfinite(z)) FAIL(c, "%s: Zref of design %zu is not finite", who, d);
        if (!(depth + z > 0.0)) FAIL(c, "%s: depth + Zref must be positive (design %zu: %g + %g)", who, d, depth, z);
        if (Zref) host[(size_t)3 * nCur + d] = z;
    }
    if (!Zref && !(depth > 0.0)) FAIL(c, "%s: depth + Zref must be positive (depth %g)", who, depth);
    return 0;
}

extern "C" int raftx_current_loads(raftx_ctx *c, int nCur, const double *speed, const double *heading_deg, const double *Zref,
                                   double depth, double shearExp, double *D) {
    if (!c) return -1;
    if (!c->have_designs) FAIL(c, "current_loads: no design set on this ctx (raftx_upload_designs / raftx_build_designs)");
    if (!D) FAIL(c, "current_loads: bad arguments");
    const int n = c->T.nDesign;
    std::vector<double> host;
    if (int rc = current_params(c, "current_loads", nCur, speed, heading_deg, Zref, (size_t)n, depth, shearExp, host)) return rc;
    if (n == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    double *dpar = sc.in<double>(host.data(), host.size()), *dD = sc.out<double>(D, (size_t)n * nCur * 6);
    if (int rc = sc.upload("current_loads")) return rc;
    if (sc.begin()) return -2;
    launch_current(c->stream, c->T, n, nCur, dpar, Zref ? dpar + (size_t)3 * nCur : nullptr, depth, shearExp, dD);
    return sc.finish();
}

extern "C" int raftx_sweep_current(raftx_ctx *c, int slot, int nCur, const double *speed, const double *heading_deg,
                                   const double *Zref, double shearExp, double *D) {
    if (!c) return -1;
    SweepSlot *slot_ = nullptr;
    if (int rc = request_slot(c, slot, "sweep_current", true, &slot_)) return rc;
    SweepSlot &S = *slot_;
    if (!D) FAIL(c, "sweep_current: bad arguments");
    const size_t n = S.bnd.empty() ? 0 : (size_t)S.bnd.back();
    std::vector<double> host;
    if (int rc = current_params(c, "sweep_current", nCur, speed, heading_deg, Zref, n, c->csets[S.cset].T.depth, shearExp, host)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (S.current.evUp) HIPCHK(c, hipEventSynchronize(S.current.evUp));   // (a second request on one slot: the first copy has left the host array)
    S.current.host.swap(host);                                           // alive until the slot is prepared again
    const double *dpar = nullptr;
    if (upload_on(c, c->sCopy, S.allocs, S.current.host.data(), S.current.host.size(), &dpar)) return -2;
    HIPCHK(c, S.current.evUp.ensure(hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(S.current.evUp, c->sCopy));
    S.current.nCur = nCur; S.current.shearExp = shearExp;
    S.current.par = dpar; S.current.Zref = Zref ? dpar + (size_t)3 * nCur : nullptr;
    S.current.D = D;
    S.current.on = true;
    return 0;
}

// ---- quasi-static mooring lines (include/raftx_mooring.h, raftx_mooring.h)
// The line source of an entry point `who`: what valid records are, which calls may leave them to the mooring program, and
// how either kind reaches the device.  (raftx_mooring_program checks its one unit's records itself, in its own wording.)
// *chains: the kind of the records, which picks the kernels: 0 single rows only, 1 a continuation row of a composite line among
// them (the CHAINS kernels), 2 a leg row of a bridle (the BRIDLES kernels, which cover composite lines too)
static int check_lines(raftx_ctx *c, const char *who, size_t nDesign, int nLine, const double *lines, int *chains) {
    *chains = 0;
    int kind = 0;
    for (size_t d = 0; d < nDesign; d++) {
        const double *row = lines + d * (size_t)nLine * RAFTX_ML_N;
        int run = 0, legs = 0;                                   // rows of the line the current row belongs to; legs of its bridle so far
        for (int l = 0; l < nLine; l++, row += RAFTX_ML_N) {
            const double cb = row[9];
            if (std::isfinite(cb) && cb != 0.0)
                FAIL(c, "%s: line %d of design %zu has seabed friction CB = %g: friction is not covered (CB must be 0)", who, l, d, cb);
            const bool cont = row[RAFTX_ML_CONT] != 0.0, leg = row[RAFTX_ML_LEG] != 0.0;
            if (!cont && !leg) {                                 // a head row or a single line
                if (legs == 1) FAIL(c, "%s: the bridle before row %d of design %zu has exactly one leg: a bridle has 2 to %d", who, l, d, RAFTX_MOOR_MAX_LEG);
                run = 1;
                legs = 0;
            } else if (leg) {
                if (cont) FAIL(c, "%s: row %d of design %zu is marked as a leg row and as a continuation row", who, l, d);
                if (!run) FAIL(c, "%s: row %d of design %zu is a leg row that follows no head row", who, l, d);
                if (!legs) {
                    const double *head = row - (size_t)run * RAFTX_ML_N;
                    if (head[3] != 0.0 || head[4] != 0.0 || head[5] != 0.0)
                        FAIL(c, "%s: row %d of design %zu heads a bridle and has a fairlead: its fields 3-5 must be zero (the stem ends at the junction)",
                             who, l - run, d);
                }
                if (++legs > RAFTX_MOOR_MAX_LEG) FAIL(c, "%s: the bridle with leg row %d of design %zu has more than %d legs", who, l, d, RAFTX_MOOR_MAX_LEG);
                kind = 2;
            } else {
                if (l == 0) FAIL(c, "%s: row 0 of design %zu is a continuation row: a composite line starts with its head row", who, d);
                if (legs) FAIL(c, "%s: row %d of design %zu is a continuation row after a leg row: the stem's rows come first", who, l, d);
                if (++run > RAFTX_MOOR_MAX_SEG)
                    FAIL(c, "%s: the composite line ending in row %d of design %zu has more than %d rows", who, l, d, RAFTX_MOOR_MAX_SEG);
                kind |= 1;
            }
        }
        if (legs == 1) FAIL(c, "%s: the bridle ending design %zu has exactly one leg: a bridle has 2 to %d", who, d, RAFTX_MOOR_MAX_LEG);
    }
    *chains = kind >= 2 ? 2 : kind;
    return 0;
}
static int check_depth(raftx_ctx *c, const char *who, double depth) {
    if (!std::isfinite(depth) || !(depth > 0.0)) FAIL(c, "%s: the depth must be positive and finite (got %g)", who, depth);
    return 0;
}
// lines == NULL: the records are those of the mooring program, evaluated at nP_expected parameters per design
static int check_line_program(raftx_ctx *c, const char *who, int nLine, int nP_expected, bool slot_has_variants) {
    if (!slot_has_variants) FAIL(c, "%s: lines == NULL needs a slot prepared with raftx_sweep_prepare_variants", who);
    if (!c->mprog.nLine) FAIL(c, "%s: no mooring program (raftx_mooring_program first)", who);
    if (c->mprog.nP != nP_expected) FAIL(c, "%s: the mooring program has %d parameters, the variant program %d", who, c->mprog.nP, nP_expected);
    if (nLine != c->mprog.nLine) FAIL(c, "%s: nLine=%d is not the %d lines of the mooring program", who, nLine, c->mprog.nLine);
    return 0;
}
// ... of a request `who` on the prepared slot S of n designs, with the depth of the slot's sea states
static int check_slot_lines(raftx_ctx *c, const char *who, const SweepSlot &S, size_t n, int nLine, const double *lines, int *chains) {
    const VariantProg *vp = S.p1.var.prog;
    if (!lines) {
        if (int rc = check_line_program(c, who, nLine, vp ? vp->nP : 0, vp != nullptr)) return rc;
        *chains = c->mprog.chains;
    } else {
        if (nLine < 1) FAIL(c, "%s: nLine must be positive (got %d)", who, nLine);
        if (int rc = check_lines(c, who, n, nLine, lines, chains)) return rc;
    }
    return check_depth(c, who, c->csets[S.cset].T.depth);
}
// The records [n,nLine,RAFTX_ML_N] on the device, in blocks of `bag`, by copies on `st`: the caller's records uploaded, or
// (records == nullptr) the program's parameters [n,nP] uploaded and a block taken that expand_lines fills.
struct StagedLines { const double *lines = nullptr, *params = nullptr; double *expanded = nullptr; };
static int stage_lines(raftx_ctx *c, hipStream_t st, Bag &bag, size_t n, int nLine, const double *records, const double *params,
                       StagedLines &L) {
    L = StagedLines{};
    const size_t nrec = n * (size_t)nLine * RAFTX_ML_N;
    if (records) return upload_on(c, st, bag, records, nrec, &L.lines);
    if (upload_on(c, st, bag, params, n * (size_t)c->mprog.nP, &L.params) || pool_alloc(c, bag, nrec, &L.expanded)) return -2;
    L.lines = L.expanded;
    return 0;
}
// ... and k_moor_expand on `st`, when the source is the program (the caller's records: nothing)
static int expand_lines(raftx_ctx *c, hipStream_t st, size_t n, int nLine, const StagedLines &L) {
    if (!L.expanded || !n) return 0;
    MoorExpandArgs E{(int)n, nLine, c->mprog.nP, c->mprog.base.p, c->mprog.coef.p, c->mprog.edit.p, L.params, L.expanded};
    hipLaunchKernelGGL(k_moor_expand, dim3(moor_grid((long long)n * nLine)), dim3(MOOR_THREADS), 0, st, E);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// k_moor_line and k_moor_design over the records of A: the chain instantiation only where a continuation row is among them, the
// bridle instantiations only where a leg row is
static void launch_moor_design(hipStream_t st, const MoorArgs &A) {
    const dim3 grid(moor_grid((long long)A.nDesign));
    if (A.chains == 2) hipLaunchKernelGGL(k_moor_design<true>, grid, dim3(MOOR_THREADS), 0, st, A);
    else hipLaunchKernelGGL(k_moor_design<false>, grid, dim3(MOOR_THREADS), 0, st, A);
}
static void launch_moor_line(hipStream_t st, const MoorArgs &A) {
    const dim3 grid(moor_grid((long long)A.nDesign * A.nLine));
    if (A.chains == 2) hipLaunchKernelGGL((k_moor_line<true, true>), grid, dim3(MOOR_THREADS), 0, st, A);
    else if (A.chains) hipLaunchKernelGGL(k_moor_line<true>, grid, dim3(MOOR_THREADS), 0, st, A);
    else hipLaunchKernelGGL(k_moor_line<false>, grid, dim3(MOOR_THREADS), 0, st, A);
}

extern "C" int raftx_mooring_lines(raftx_ctx *c, int nDesign, int nLine, const double *lines, const double *pose, double depth,
                                   double *C_moor, double *F_moor, double *T, double *J, double *line_out, int32_t *flags) {
    if (!c) return -1;
    if (nLine < 1) FAIL(c, "mooring_lines: nLine must be positive (got %d)", nLine);
    if (nDesign < 0) FAIL(c, "mooring_lines: nDesign must not be negative (got %d)", nDesign);
    if (!lines || !flags) FAIL(c, "mooring_lines: bad arguments (lines and flags are required)");
    if (int rc = check_depth(c, "mooring_lines", depth)) return rc;
    int chains = 0;
    if (int rc = check_lines(c, "mooring_lines", (size_t)nDesign, nLine, lines, &chains)) return rc;
    if (nDesign == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    const size_t nl = (size_t)nDesign * nLine;
    StagedLines L;
    if (stage_lines(c, c->stream, sc.bag, (size_t)nDesign, nLine, lines, nullptr, L)) return -2;
    MoorArgs A;
    memset(&A, 0, sizeof(A));
    A.nDesign = nDesign; A.nLine = nLine; A.depth = depth;
    A.lines = L.lines;
    A.pose = sc.in<double>(pose, (size_t)nDesign * 6);
    A.lw = sc.tmp<double>(nl * MOOR_LW_N);
    if (chains == 2) A.bw = sc.tmp<double>(nl * MOOR_BW_N);
    A.C = sc.out<double>(C_moor, (size_t)nDesign * 36);
    A.F = sc.out<double>(F_moor, (size_t)nDesign * 6);
    A.T = sc.out<double>(T, nl * 2);
    A.J = sc.out<double>(J, nl * 12);
    A.line_out = sc.out<double>(line_out, nl * MOOR_LO_N);
    A.flags = sc.out<int>(flags, (size_t)nDesign);
    if (int rc = sc.upload("mooring_lines")) return rc;
    if (sc.begin()) return -2;
    A.chains = chains;
    launch_moor_line(c->stream, A);
    launch_moor_design(c->stream, A);
    return sc.finish();
}

extern "C" int raftx_mooring_program(raftx_ctx *c, int nLine, const double *lines, int nParam, const double *lineCoef,
                                     const int32_t *lineEdit) {
    if (!c) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (nLine == 0) {
        mooring_program_release(c);
        return 0;
    }
    if (nLine < 0 || !lines || !lineCoef || !lineEdit) FAIL(c, "mooring_program: bad arguments");
    if (!c->vprog.nM) FAIL(c, "mooring_program: no variant program on this ctx (raftx_variant_program first)");
    if (nParam != c->vprog.nP)
        FAIL(c, "mooring_program: nParam=%d is not the %d parameters of the installed variant program", nParam, c->vprog.nP);
    int chains = 0;
    for (int l = 0, run = 0; l < nLine; l++) {
        const double cb = lines[(size_t)l * RAFTX_ML_N + 9];
        if (std::isfinite(cb) && cb != 0.0)
            FAIL(c, "mooring_program: line %d has seabed friction CB = %g: friction is not covered (CB must be 0)", l, cb);
        if (lines[(size_t)l * RAFTX_ML_N + RAFTX_ML_LEG] != 0.0) continue;          // (leg rows: check_lines below)
        if (lines[(size_t)l * RAFTX_ML_N + RAFTX_ML_CONT] != 0.0) {
            if (l == 0) FAIL(c, "mooring_program: row 0 is a continuation row: a composite line starts with its head row");
            if (++run > RAFTX_MOOR_MAX_SEG) FAIL(c, "mooring_program: the composite line ending in row %d has more than %d rows", l, RAFTX_MOOR_MAX_SEG);
        } else
            run = 1;
    }
    if (int rc = check_lines(c, "mooring_program", 1, nLine, lines, &chains)) return rc;     // the bridle errors, and the kind of the records
    for (int l = 0; l < nLine; l++) {
        if (!lineEdit[l]) continue;
        const double *row = lines + (size_t)l * RAFTX_ML_N;
        if (row[RAFTX_ML_CONT] != 0.0)
            FAIL(c, "mooring_program: lineEdit on row %d, a continuation row: the anchor and the fairlead are the head row's", l);
        // a leg row has a fairlead and no anchor, the head row of a bridle an anchor and no fairlead: the coefficients of the
        // other three fields must all be zero (k_moor_expand then writes the zeros the record format asks for)
        int lo = 0, hi = 0;
        if (row[RAFTX_ML_LEG] != 0.0) { lo = 0; hi = 3; }
        else {
            int k = l + 1;
            while (k < nLine && lines[(size_t)k * RAFTX_ML_N + RAFTX_ML_CONT] != 0.0) k++;
            if (k < nLine && lines[(size_t)k * RAFTX_ML_N + RAFTX_ML_LEG] != 0.0) { lo = 3; hi = 6; }
        }
        for (int f = lo; f < hi; f++)
            for (int k = 0; k <= nParam; k++)
                if (lineCoef[((size_t)l * 6 + f) * (nParam + 1) + k] != 0.0)
                    FAIL(c, "mooring_program: lineEdit on row %d, %s, has a coefficient for field %d: only fields %s may be edited there", l,
                         lo == 0 ? "a leg row of a bridle" : "the head row of a bridle", f, lo == 0 ? "3-5 (the leg's fairlead)" : "0-2 (the anchor)");
    }
    mooring_program_release(c);
    const size_t nb = (size_t)nLine * RAFTX_ML_N * 8, nc = (size_t)nLine * 6 * (nParam + 1) * 8, ne = (size_t)nLine * 4;
    if (c->mprog.base.grow(nb / 8) != hipSuccess || c->mprog.coef.grow(nc / 8) != hipSuccess || c->mprog.edit.grow(ne / 4) != hipSuccess) {
        mooring_program_release(c);
        FAIL(c, "mooring_program: device allocation failed");
    }
    HIPCHK(c, hipMemcpy(c->mprog.base.p, lines, nb, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->mprog.coef.p, lineCoef, nc, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->mprog.edit.p, lineEdit, ne, hipMemcpyHostToDevice));
    c->mprog.nLine = nLine;
    c->mprog.nP = nParam;
    c->mprog.chains = chains;
    return 0;
}

extern "C" int raftx_mooring_expand(raftx_ctx *c, int nDesign, const double *params, double *lines_out) {
    if (!c) return -1;
    if (!c->mprog.nLine) FAIL(c, "mooring_expand: no program (raftx_mooring_program first)");
    const int nP = c->mprog.nP, nLine = c->mprog.nLine;
    if (nDesign < 0 || (!params && nDesign && nP) || !lines_out) FAIL(c, "mooring_expand: bad arguments");
    if (!nDesign) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    StagedLines L;
    if (stage_lines(c, c->stream, sc.bag, (size_t)nDesign, nLine, nullptr, params, L)) return -2;
    sc.out_from(lines_out, L.expanded, (size_t)nDesign * nLine * RAFTX_ML_N);
    if (sc.begin()) return -2;
    if (int rc = expand_lines(c, c->stream, (size_t)nDesign, nLine, L)) return rc;
    return sc.finish();
}

// ---- the mean equilibrium pose (include/raftx_statics.h, raftx_statics.h)
// the tolerances of an entry point `who`: {m, rad}, or null for the defaults
static int mean_pose_tol(raftx_ctx *c, const char *who, const double tol[2], double *tolT, double *tolR) {
    *tolT = tol ? tol[0] : 1e-9;
    *tolR = tol ? tol[1] : 1e-10;
    if (!std::isfinite(*tolT) || !std::isfinite(*tolR) || *tolT < 0.0 || *tolR < 0.0)
        FAIL(c, "%s: the tolerances must be finite and not negative (got %g m, %g rad)", who, *tolT, *tolR);
    return 0;
}
// The launch both entries share (raftx_mean_pose: a batch; raftx_sweep_mean_pose: a block of a crossing): A holds the arrays
// of nDesign > 0 designs, the settings are filled in here, the whole iteration is one launch on st.
static void launch_mean_pose(hipStream_t st, MeanPoseArgs &A, int nDesign, int nLine, double depth, double tolT, double tolR, int max_iter) {
    A.nDesign = nDesign; A.nLine = nLine; A.G = mean_pose_group(nLine); A.maxIter = max_iter > 0 ? max_iter : MP_MAX_IT;
    A.depth = depth; A.tolT = tolT; A.tolR = tolR;
    const int perBlock = MP_THREADS / A.G;
    const dim3 grid((unsigned)((nDesign + perBlock - 1) / perBlock));
    if (A.chains == 2) hipLaunchKernelGGL((k_mean_pose<true, true>), grid, dim3(MP_THREADS), 0, st, A);
    else if (A.chains) hipLaunchKernelGGL(k_mean_pose<true>, grid, dim3(MP_THREADS), 0, st, A);
    else hipLaunchKernelGGL(k_mean_pose<false>, grid, dim3(MP_THREADS), 0, st, A);
}
extern "C" int raftx_mean_pose(raftx_ctx *c, int nDesign, int nLine, const double *lines, const double *params, double depth,
                               const double *K_hs, const double *F0, const double *F_env, const double *x_ref, const double tol[2],
                               int max_iter, double *pose, double *C_moor, double *F_moor, double *T, double *J, double *F_res,
                               int32_t *iterations, int32_t *flags) {
    if (!c) return -1;
    if (nLine < 1) FAIL(c, "mean_pose: nLine must be positive (got %d)", nLine);
    if (nDesign < 0) FAIL(c, "mean_pose: nDesign must not be negative (got %d)", nDesign);
    if (!K_hs || !F0 || !flags) FAIL(c, "mean_pose: bad arguments (K_hs, F0 and flags are required)");
    if (int rc = check_depth(c, "mean_pose", depth)) return rc;
    double tolT, tolR;
    if (int rc = mean_pose_tol(c, "mean_pose", tol, &tolT, &tolR)) return rc;
    const size_t n = (size_t)nDesign, nl = n * nLine;
    int chains = 0;
    if (!lines) {
        // (a batch has no slot and no variant program to agree with; its no-program wording is its own)
        if (!c->mprog.nLine) FAIL(c, "mean_pose: lines == NULL without a mooring program (raftx_mooring_program first)");
        if (int rc = check_line_program(c, "mean_pose", nLine, c->mprog.nP, true)) return rc;
        if (!params && nDesign && c->mprog.nP) FAIL(c, "mean_pose: lines == NULL needs params [nDesign,%d]", c->mprog.nP);
        chains = c->mprog.chains;
    } else if (int rc = check_lines(c, "mean_pose", n, nLine, lines, &chains))
        return rc;
    if (nDesign == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    StagedLines L;
    if (stage_lines(c, c->stream, sc.bag, n, nLine, lines, params, L)) return -2;
    MeanPoseArgs A;
    memset(&A, 0, sizeof(A));
    A.lines = L.lines;
    A.chains = chains;
    A.K_hs = sc.in<double>(K_hs, n * 36);
    A.F0 = sc.in<double>(F0, n * 6);
    A.F_env = sc.in<double>(F_env, n * 6);
    A.x_ref = sc.in<double>(x_ref, n * 6);
    A.lw = sc.tmp<double>(nl * MOOR_LW_N);
    if (chains == 2) A.bw = sc.tmp<double>(nl * MOOR_BW_N);
    A.pose = sc.out<double>(pose, n * 6);
    A.C = sc.out<double>(C_moor, n * 36);
    A.F = sc.out<double>(F_moor, n * 6);
    A.T = sc.out<double>(T, nl * 2);
    A.J = sc.out<double>(J, nl * 12);
    A.Fres = sc.out<double>(F_res, n * 6);
    A.iterations = sc.out<int>(iterations, n);
    A.flags = sc.out<int>(flags, n);
    if (int rc = sc.upload("mean_pose")) return rc;
    if (sc.begin()) return -2;
    if (int rc = expand_lines(c, c->stream, n, nLine, L)) return rc;   // (inside the timed window, as raftx_mooring_expand)
    launch_mean_pose(c->stream, A, nDesign, nLine, depth, tolT, tolR, max_iter);
    return sc.finish();
}

// ---- staticsMod 1 (raftx_mean_pose_nonlinear / _variants; k_mean_pose_nl, raftx_statics.h)
// what the two entries share besides the geometry: the checks that do not concern it ...
struct NlCommon {
    double rho, g;
    const double *drho;
    int nLine;
    const double *lines;
    double depth;
    int nPM, nX;
    const double *pm, *C_extra, *F_extra, *F_env, *x_ref, *tol;
    int max_iter;
    double *pose, *K_hs, *F0, *C_moor, *F_moor, *T, *J, *F_res;
    int32_t *iterations, *flags;
};
static int nl_check(raftx_ctx *c, const char *who, int nDesign, const NlCommon &U, double *tolT, double *tolR) {
    if (U.nLine < 1) FAIL(c, "%s: nLine must be positive (got %d)", who, U.nLine);
    if (nDesign < 0) FAIL(c, "%s: nDesign must not be negative (got %d)", who, nDesign);
    if (!U.flags) FAIL(c, "%s: bad arguments (flags is required)", who);
    if (int rc = check_depth(c, who, U.depth)) return rc;
    if (int rc = mean_pose_tol(c, who, U.tol, tolT, tolR)) return rc;
    if (!std::isfinite(U.rho) || !std::isfinite(U.g) || !(U.rho > 0.0) || !(U.g > 0.0))
        FAIL(c, "%s: rho and g must be positive and finite (got %g, %g)", who, U.rho, U.g);
    if (U.nX != 0 && U.nX != 1 && U.nX != nDesign) FAIL(c, "%s: nX must be 0, 1 or nDesign (got %d)", who, U.nX);
    if (U.nPM < 0) FAIL(c, "%s: nPM must not be negative (got %d)", who, U.nPM);
    if (U.nX && U.nPM && !U.pm) FAIL(c, "%s: nPM=%d point masses and pm is NULL", who, U.nPM);
    return 0;
}
// ... and the staging, the launch and the results, once the geometry fields of N are set.  maxMember: members of the largest design.
template <class Rows>
static void launch_mean_pose_nl(hipStream_t st, const MeanPoseNlArgs &N, dim3 grid) {
    if (N.P.chains == 2) hipLaunchKernelGGL((k_mean_pose_nl<Rows, true, true>), grid, dim3(MP_THREADS), 0, st, N);
    else if (N.P.chains) hipLaunchKernelGGL((k_mean_pose_nl<Rows, true, false>), grid, dim3(MP_THREADS), 0, st, N);
    else hipLaunchKernelGGL((k_mean_pose_nl<Rows, false, false>), grid, dim3(MP_THREADS), 0, st, N);
}
static int nl_run(raftx_ctx *c, const char *who, Scratch &sc, MeanPoseNlArgs &N, int nDesign, size_t nMember, int maxMember,
                  const NlCommon &U, const double *params, int chains, double tolT, double tolR) {
    const size_t n = (size_t)nDesign, nl = n * U.nLine, nx = (size_t)U.nX;
    StagedLines L;
    if (stage_lines(c, c->stream, sc.bag, n, U.nLine, U.lines, U.lines ? nullptr : params, L)) return -2;
    MeanPoseArgs &A = N.P;
    A.lines = L.lines;
    A.chains = chains;
    A.F_env = sc.in<double>(U.F_env, n * 6);
    A.x_ref = sc.in<double>(U.x_ref, n * 6);
    A.lw = sc.tmp<double>(nl * MOOR_LW_N);
    if (chains == 2) A.bw = sc.tmp<double>(nl * MOOR_BW_N);
    A.pose = sc.out<double>(U.pose, n * 6);
    A.C = sc.out<double>(U.C_moor, n * 36);
    A.F = sc.out<double>(U.F_moor, n * 6);
    A.T = sc.out<double>(U.T, nl * 2);
    A.J = sc.out<double>(U.J, nl * 12);
    A.Fres = sc.out<double>(U.F_res, n * 6);
    A.iterations = sc.out<int>(U.iterations, n);
    A.flags = sc.out<int>(U.flags, n);
    N.rho = U.rho; N.g = U.g;
    N.drho = sc.in<double>(U.drho, n);
    N.nPM = U.nPM; N.nX = U.nX;
    N.pm = sc.in<double>(U.pm, nx * 4 * (size_t)U.nPM);
    N.Cx = sc.in<double>(U.C_extra, nx * 36);
    N.Fx = sc.in<double>(U.F_extra, nx * 6);
    N.mw = sc.tmp<double>(std::max<size_t>(nMember, 1) * FR_N);
    N.mflag = sc.tmp<int>(std::max<size_t>(nMember, 1));
    N.red = sc.tmp<double>(n * NL_RED_N);
    N.K_out = sc.out<double>(U.K_hs, n * 36);
    N.F0_out = sc.out<double>(U.F0, n * 6);
    if (int rc = sc.upload(who)) return rc;
    if (sc.begin()) return -2;
    if (int rc = expand_lines(c, c->stream, n, U.nLine, L)) return rc;
    A.nDesign = nDesign; A.nLine = U.nLine; A.G = mean_pose_nl_group(maxMember, U.nLine);
    A.maxIter = U.max_iter > 0 ? U.max_iter : MP_MAX_IT;
    A.depth = U.depth; A.tolT = tolT; A.tolR = tolR;
    const int perBlock = MP_THREADS / A.G;
    const dim3 grid((unsigned)((nDesign + perBlock - 1) / perBlock));
    if (N.prog.params) launch_mean_pose_nl<GeomRowsProg>(c->stream, N, grid);
    else launch_mean_pose_nl<GeomRowsPlain>(c->stream, N, grid);
    return sc.finish();
}
extern "C" int raftx_mean_pose_nonlinear(raftx_ctx *c, int nDesign, const int64_t *memberOff, const double *members,
                                         const int64_t *stationOff, const double *stations, const int64_t *capOff, const double *caps,
                                         double rho, double g, const double *drho, int nLine, const double *lines, double depth, int nPM,
                                         int nX, const double *pm, const double *C_extra, const double *F_extra, const double *F_env,
                                         const double *x_ref, const double tol[2], int max_iter, double *pose, double *K_hs, double *F0,
                                         double *C_moor, double *F_moor, double *T, double *J, double *F_res, int32_t *iterations,
                                         int32_t *flags) {
    if (!c) return -1;
    const char *who = "mean_pose_nonlinear";
    const NlCommon U{rho, g, drho, nLine, lines, depth, nPM, nX, pm, C_extra, F_extra, F_env, x_ref, tol, max_iter,
                     pose, K_hs, F0, C_moor, F_moor, T, J, F_res, iterations, flags};
    double tolT, tolR;
    if (int rc = nl_check(c, who, nDesign, U, &tolT, &tolR)) return rc;
    if (!lines) FAIL(c, "%s: lines is NULL (the mooring program belongs to raftx_mean_pose_nonlinear_variants)", who);
    if (!memberOff || !stationOff) FAIL(c, "%s: bad arguments (memberOff and stationOff are required)", who);
    int maxMember = 0;
    for (int d = 0; d < nDesign; d++) {
        if (memberOff[d + 1] < memberOff[d]) FAIL(c, "%s: member offsets not monotone at design %d", who, d);
        maxMember = (int)std::min<int64_t>(std::max<int64_t>(maxMember, memberOff[d + 1] - memberOff[d]), 1 << 30);
    }
    const int64_t m0 = memberOff[0], nMember = memberOff[nDesign] - m0;
    if (m0 < 0) FAIL(c, "%s: member offsets not monotone at design 0", who);
    if (nMember >= ((int64_t)1 << 31)) FAIL(c, "%s: %lld members in one batch", who, (long long)nMember);
    for (int64_t m = 0; m < nMember; m++) {
        if (stationOff[m0 + m + 1] < stationOff[m0 + m]) FAIL(c, "%s: station offsets not monotone at member %lld", who, (long long)(m0 + m));
        if (capOff && capOff[m0 + m + 1] < capOff[m0 + m]) FAIL(c, "%s: cap offsets not monotone at member %lld", who, (long long)(m0 + m));
    }
    const int64_t s0 = stationOff[m0], nSta = stationOff[m0 + nMember] - s0, c0 = capOff ? capOff[m0] : 0,
                  nCap = capOff ? capOff[m0 + nMember] - c0 : 0;
    if (s0 < 0 || c0 < 0) FAIL(c, "%s: station or cap offsets not monotone at member %lld", who, (long long)m0);
    if ((nMember && !members) || (nSta && !stations) || (nCap && !caps)) FAIL(c, "%s: bad arguments (rows are NULL)", who);
    int chains = 0;
    if (int rc = check_lines(c, who, (size_t)nDesign, nLine, lines, &chains)) return rc;
    if (nDesign == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<int64_t> mo((size_t)nDesign + 1), so((size_t)nMember + 1), co(capOff ? (size_t)nMember + 1 : 0);
    for (int d = 0; d <= nDesign; d++) mo[(size_t)d] = memberOff[d] - m0;
    for (int64_t m = 0; m <= nMember; m++) {
        so[(size_t)m] = stationOff[m0 + m] - s0;
        if (capOff) co[(size_t)m] = capOff[m0 + m] - c0;
    }
    Scratch sc(c);
    MeanPoseNlArgs N;
    memset(&N, 0, sizeof(N));
    N.memberOff = sc.in<int64_t>(mo.data(), mo.size());
    N.stationOff = sc.in<int64_t>(so.data(), so.size());
    N.capOff = capOff ? sc.in<int64_t>(co.data(), co.size()) : nullptr;
    N.gm = sc.in<double>(members ? members + (size_t)m0 * RAFTX_GM_N : nullptr, (size_t)nMember * RAFTX_GM_N);
    N.gs = sc.in<double>(stations ? stations + (size_t)s0 * RAFTX_GS_N : nullptr, (size_t)nSta * RAFTX_GS_N);
    N.gc = sc.in<double>(caps ? caps + (size_t)c0 * RAFTX_GC_N : nullptr, (size_t)std::max<int64_t>(nCap, 1) * RAFTX_GC_N);
    if (capOff && !N.gc) N.gc = sc.tmp<double>(RAFTX_GC_N);      // (no cap in the batch: a block nobody reads)
    return nl_run(c, who, sc, N, nDesign, (size_t)nMember, maxMember, U, nullptr, chains, tolT, tolR);
}
extern "C" int raftx_mean_pose_nonlinear_variants(raftx_ctx *c, int nDesign, const double *params, double rho, double g,
                                                  const double *drho, int nLine, const double *lines, double depth, int nPM, int nX,
                                                  const double *pm, const double *C_extra, const double *F_extra, const double *F_env,
                                                  const double *x_ref, const double tol[2], int max_iter, double *pose, double *K_hs,
                                                  double *F0, double *C_moor, double *F_moor, double *T, double *J, double *F_res,
                                                  int32_t *iterations, int32_t *flags) {
    if (!c) return -1;
    const char *who = "mean_pose_nonlinear_variants";
    const VariantProg &P = c->vprog;
    if (!P.nM) FAIL(c, "%s: no program (raftx_variant_program first)", who);
    const NlCommon U{rho, g, drho, nLine, lines, depth, nPM, nX, pm, C_extra, F_extra, F_env, x_ref, tol, max_iter,
                     pose, K_hs, F0, C_moor, F_moor, T, J, F_res, iterations, flags};
    double tolT, tolR;
    if (int rc = nl_check(c, who, nDesign, U, &tolT, &tolR)) return rc;
    if (!params && nDesign && P.nP) FAIL(c, "%s: bad arguments (params [nDesign,%d] is required)", who, P.nP);
    if (params && !all_finite(params, (size_t)nDesign * P.nP)) FAIL(c, "%s: a parameter value is not finite", who);
    int chains = 0;
    if (!lines) {
        if (!c->mprog.nLine) FAIL(c, "%s: lines == NULL without a mooring program (raftx_mooring_program first)", who);
        if (int rc = check_line_program(c, who, nLine, P.nP, true)) return rc;
        chains = c->mprog.chains;
    } else if (int rc = check_lines(c, who, (size_t)nDesign, nLine, lines, &chains))
        return rc;
    if (nDesign == 0) return 0;
    if ((int64_t)nDesign * P.nM >= ((int64_t)1 << 31)) FAIL(c, "%s: %lld members in one batch", who, (long long)nDesign * P.nM);
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    MeanPoseNlArgs N;
    memset(&N, 0, sizeof(N));
    N.nM = P.nM;
    N.stationOff = sc.in<int64_t>(P.hS.data(), P.hS.size());
    N.capOff = P.has_caps ? sc.in<int64_t>(P.hC.data(), P.hC.size()) : nullptr;
    variant_view(P, N.prog);
    static const double no_param = 0.0;                          // (a program without parameters still marks "rows of the program")
    N.prog.params = sc.in<double>(P.nP ? params : &no_param, P.nP ? (size_t)nDesign * P.nP : 1);
    return nl_run(c, who, sc, N, nDesign, (size_t)nDesign * P.nM, P.nM, U, params, chains, tolT, tolR);
}

// ---- arrays of units with shared lines (include/raftx_array_mooring.h, raftx_array_mooring.h)
// The records of an entry point `who`: the record errors of check_lines, then the unit fields of every row.  A value that is
// not an integer (a NaN too) is refused here, so the kernels may index with it.
static int check_array_lines(raftx_ctx *c, const char *who, size_t nArray, int nUnit, int nLine, const double *lines, int *chains) {
    if (nUnit < 1 || nUnit > RAFTX_ARRAY_MAX_UNIT) FAIL(c, "%s: nUnit must be 1 to %d (got %d)", who, RAFTX_ARRAY_MAX_UNIT, nUnit);
    if (int rc = check_lines(c, who, nArray, nLine, lines, chains)) return rc;
    for (size_t a = 0; a < nArray; a++) {
        const double *row = lines + a * (size_t)nLine * RAFTX_ML_N;
        double headB = 0.0;
        bool headShared = false;
        for (int l = 0; l < nLine; l++, row += RAFTX_ML_N) {
            const double ub = row[RAFTX_ML_UNIT_B], ua = row[RAFTX_ML_UNIT_A];
            if (!(ub == std::floor(ub)) || !(ub >= 0.0) || !(ub < (double)nUnit))
                FAIL(c, "%s: row %d of array %zu has unit B = %g: an integer 0 to %d is required", who, l, a, ub, nUnit - 1);
            if (!(ua == std::floor(ua)) || !(ua >= 0.0) || !(ua <= (double)nUnit))
                FAIL(c, "%s: row %d of array %zu has unit A = %g: 0 (an anchor) or 1 + a unit index, at most %d, is required", who, l, a, ua, nUnit);
            if (row[RAFTX_ML_CONT] != 0.0 || row[RAFTX_ML_LEG] != 0.0) {
                if (headShared)
                    FAIL(c, "%s: row %d of array %zu continues a shared row: a shared row is one suspended line without a continuation or leg row", who, l, a);
                if (ua != 0.0 || ub != headB)
                    FAIL(c, "%s: row %d of array %zu is a continuation or leg row with unit fields (%g, %g): it inherits its head row's unit %g (and 0)",
                         who, l, a, ub, ua, headB);
                continue;
            }
            headB = ub;
            headShared = ua != 0.0;
            if (!headShared) continue;
            if (ua - 1.0 == ub) FAIL(c, "%s: shared row %d of array %zu has both ends on unit %g: unit A and unit B must differ", who, l, a, ub);
            if (row[RAFTX_ML_WJOINT] != 0.0 || row[13] != 0.0 || !(row[9] == 0.0))
                FAIL(c, "%s: shared row %d of array %zu has a joint weight, CB or field 13 set: a shared row is one plain suspended line", who, l, a);
        }
    }
    return 0;
}
static void launch_array_moor(hipStream_t st, const ArrayMoorArgs &A) {
    const dim3 gl(moor_grid((long long)A.nArray * A.nLine)), gd(moor_grid((long long)A.nArray * A.nUnit * A.nUnit));
    if (A.chains == 2) hipLaunchKernelGGL((k_array_moor_line<true, true>), gl, dim3(MOOR_THREADS), 0, st, A);
    else if (A.chains) hipLaunchKernelGGL((k_array_moor_line<true, false>), gl, dim3(MOOR_THREADS), 0, st, A);
    else hipLaunchKernelGGL((k_array_moor_line<false, false>), gl, dim3(MOOR_THREADS), 0, st, A);
    if (A.chains == 2) hipLaunchKernelGGL(k_array_moor_design<true>, gd, dim3(MOOR_THREADS), 0, st, A);
    else hipLaunchKernelGGL(k_array_moor_design<false>, gd, dim3(MOOR_THREADS), 0, st, A);
}

extern "C" int raftx_array_mooring_lines(raftx_ctx *c, int nArray, int nUnit, int nLine, const double *lines, const double *pose,
                                         double depth, double *C, double *F, double *T, double *J, double *line_out, int32_t *flags) {
    if (!c) return -1;
    if (nLine < 1) FAIL(c, "array_mooring_lines: nLine must be positive (got %d)", nLine);
    if (nArray < 0) FAIL(c, "array_mooring_lines: nArray must not be negative (got %d)", nArray);
    if (!lines || !pose || !flags) FAIL(c, "array_mooring_lines: bad arguments (lines, pose and flags are required)");
    if (int rc = check_depth(c, "array_mooring_lines", depth)) return rc;
    int chains = 0;
    if (int rc = check_array_lines(c, "array_mooring_lines", (size_t)nArray, nUnit, nLine, lines, &chains)) return rc;
    if (nArray == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    const size_t na = (size_t)nArray, nl = na * nLine, n = (size_t)6 * nUnit;
    StagedLines L;
    if (stage_lines(c, c->stream, sc.bag, na, nLine, lines, nullptr, L)) return -2;
    ArrayMoorArgs A;
    memset(&A, 0, sizeof(A));
    A.nArray = nArray; A.nUnit = nUnit; A.nLine = nLine; A.depth = depth;
    A.lines = L.lines;
    A.pose = sc.in<double>(pose, na * n);
    A.lw = sc.tmp<double>(nl * MOOR_LW_N);
    A.sw = sc.tmp<double>(nl * ARR_SW_N);
    if (chains == 2) A.bw = sc.tmp<double>(nl * MOOR_BW_N);
    A.C = sc.out<double>(C, na * n * n);
    A.F = sc.out<double>(F, na * n);
    A.T = sc.out<double>(T, nl * 2);
    A.J = sc.out<double>(J, nl * 2 * n);
    A.line_out = sc.out<double>(line_out, nl * MOOR_LO_N);
    A.flags = sc.out<int>(flags, na);
    if (int rc = sc.upload("array_mooring_lines")) return rc;
    if (sc.begin()) return -2;
    A.chains = chains;
    launch_array_moor(c->stream, A);
    return sc.finish();
}

extern "C" int raftx_array_mean_pose(raftx_ctx *c, int nArray, int nUnit, int nLine, const double *lines, double depth,
                                     const double *K_hs, const double *F0, const double *F_env, const double *x_ref, const double tol[2],
                                     int max_iter, double *pose, double *C, double *F, double *T, double *J, double *F_res,
                                     int32_t *iterations, int32_t *flags) {
    if (!c) return -1;
    if (nLine < 1) FAIL(c, "array_mean_pose: nLine must be positive (got %d)", nLine);
    if (nArray < 0) FAIL(c, "array_mean_pose: nArray must not be negative (got %d)", nArray);
    if (!lines || !K_hs || !F0 || !x_ref || !flags)
        FAIL(c, "array_mean_pose: bad arguments (lines, K_hs, F0, x_ref and flags are required)");
    if (int rc = check_depth(c, "array_mean_pose", depth)) return rc;
    double tolT, tolR;
    if (int rc = mean_pose_tol(c, "array_mean_pose", tol, &tolT, &tolR)) return rc;
    int chains = 0;
    if (int rc = check_array_lines(c, "array_mean_pose", (size_t)nArray, nUnit, nLine, lines, &chains)) return rc;
    if (nArray == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    const size_t na = (size_t)nArray, nl = na * nLine, n = (size_t)6 * nUnit;
    StagedLines L;
    if (stage_lines(c, c->stream, sc.bag, na, nLine, lines, nullptr, L)) return -2;
    ArrayPoseArgs A;
    memset(&A, 0, sizeof(A));
    A.nArray = nArray; A.nUnit = nUnit; A.nLine = nLine; A.maxIter = max_iter > 0 ? max_iter : MP_MAX_IT;
    A.depth = depth; A.tolT = tolT; A.tolR = tolR;
    A.lines = L.lines;
    A.chains = chains;
    A.K_hs = sc.in<double>(K_hs, na * nUnit * 36);
    A.F0 = sc.in<double>(F0, na * n);
    A.F_env = sc.in<double>(F_env, na * n);
    A.x_ref = sc.in<double>(x_ref, na * n);
    A.lw = sc.tmp<double>(nl * MOOR_LW_N);
    A.sw = sc.tmp<double>(nl * ARR_SW_N);
    if (chains == 2) A.bw = sc.tmp<double>(nl * MOOR_BW_N);
    A.pose = sc.out<double>(pose, na * n);
    A.C = C ? sc.out<double>(C, na * n * n) : sc.tmp<double>(na * n * n);      // the iteration itself passes C and F through memory
    A.F = F ? sc.out<double>(F, na * n) : sc.tmp<double>(na * n);
    A.T = sc.out<double>(T, nl * 2);
    A.J = sc.out<double>(J, nl * 2 * n);
    A.Fres = sc.out<double>(F_res, na * n);
    A.iterations = sc.out<int>(iterations, na);
    A.flags = sc.out<int>(flags, na);
    if (int rc = sc.upload("array_mean_pose")) return rc;
    if (sc.begin()) return -2;
    const dim3 grid((unsigned)nArray);
    if (chains == 2) hipLaunchKernelGGL((k_array_mean_pose<true, true>), grid, dim3(ARR_THREADS), 0, c->stream, A);
    else if (chains) hipLaunchKernelGGL((k_array_mean_pose<true, false>), grid, dim3(ARR_THREADS), 0, c->stream, A);
    else hipLaunchKernelGGL((k_array_mean_pose<false, false>), grid, dim3(ARR_THREADS), 0, c->stream, A);
    return sc.finish();
}

// ---- eigen analysis of moored arrays (include/raftx_array_modal.h, raftx_array_modal.h)
static void launch_array_modal(hipStream_t st, int nUnit, const ArrayModalArgs &A) {
    const dim3 grid((unsigned)A.n), block(64);
    switch (nUnit) {
    case 1: hipLaunchKernelGGL(k_array_modal<6>, grid, block, 0, st, A); break;
    case 2: hipLaunchKernelGGL(k_array_modal<12>, grid, block, 0, st, A); break;
    case 3: hipLaunchKernelGGL(k_array_modal<18>, grid, block, 0, st, A); break;
    case 4: hipLaunchKernelGGL(k_array_modal<24>, grid, block, 0, st, A); break;
    case 5: hipLaunchKernelGGL(k_array_modal<30>, grid, block, 0, st, A); break;
    default: hipLaunchKernelGGL(k_array_modal<36>, grid, block, 0, st, A); break;
    }
}
static_assert(RAFTX_ARRAY_MAX_UNIT == 6, "launch_array_modal instantiates k_array_modal for 1 .. 6 units");

extern "C" int raftx_array_modal_batch(raftx_ctx *c, int nArray, int nUnit, const double *M, const double *C, double *fn,
                                       double *modes, int32_t *flags) {
    if (!c) return -1;
    if (nUnit < 1 || nUnit > RAFTX_ARRAY_MAX_UNIT) FAIL(c, "array_modal_batch: nUnit must be 1 to %d (got %d)", RAFTX_ARRAY_MAX_UNIT, nUnit);
    if (nArray < 0) FAIL(c, "array_modal_batch: nArray must not be negative (got %d)", nArray);
    if (nArray > 0 && (!M || !C || !fn || !modes || !flags)) FAIL(c, "array_modal_batch: bad arguments");
    if (nArray == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    const size_t na = (size_t)nArray, n = (size_t)6 * nUnit;
    ArrayModalArgs A;
    memset(&A, 0, sizeof(A));
    A.n = nArray;
    A.M = sc.in<double>(M, na * n * n);
    A.C = sc.in<double>(C, na * n * n);
    A.fn = sc.out<double>(fn, na * n);
    A.modes = sc.out<double>(modes, na * n * n);
    A.flags = sc.out<int32_t>(flags, na);
    if (int rc = sc.upload("array_modal_batch")) return rc;
    if (sc.begin()) return -2;
    launch_array_modal(c->stream, nUnit, A);
    return sc.finish();
}

extern "C" int raftx_array_modal_moored(raftx_ctx *c, int nArray, int nUnit, int nLine, const double *lines, const double *pose,
                                        double depth, const double *M_unit, const double *K_unit, const double *dC, double *fn,
                                        double *modes, double *C_out, int32_t *flags, int32_t *moor_flags) {
    if (!c) return -1;
    if (nLine < 1) FAIL(c, "array_modal_moored: nLine must be positive (got %d)", nLine);
    if (nArray < 0) FAIL(c, "array_modal_moored: nArray must not be negative (got %d)", nArray);
    if (!lines || !pose || !M_unit || !K_unit || !fn || !modes || !flags || !moor_flags)
        FAIL(c, "array_modal_moored: bad arguments (lines, pose, M_unit, K_unit, fn, modes, flags and moor_flags are required)");
    if (int rc = check_depth(c, "array_modal_moored", depth)) return rc;
    int chains = 0;
    if (int rc = check_array_lines(c, "array_modal_moored", (size_t)nArray, nUnit, nLine, lines, &chains)) return rc;
    if (nArray == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    const size_t na = (size_t)nArray, nl = na * nLine, n = (size_t)6 * nUnit;
    StagedLines L;
    if (stage_lines(c, c->stream, sc.bag, na, nLine, lines, nullptr, L)) return -2;
    ArrayMoorArgs A;                                     // the line kernels of raftx_array_mooring_lines, C alone asked for
    memset(&A, 0, sizeof(A));
    A.nArray = nArray; A.nUnit = nUnit; A.nLine = nLine; A.depth = depth;
    A.lines = L.lines;
    A.pose = sc.in<double>(pose, na * n);
    A.lw = sc.tmp<double>(nl * MOOR_LW_N);
    A.sw = sc.tmp<double>(nl * ARR_SW_N);
    if (chains == 2) A.bw = sc.tmp<double>(nl * MOOR_BW_N);
    A.C = sc.tmp<double>(na * n * n);
    A.flags = sc.out<int>(moor_flags, na);
    ArrayModalAssembleArgs B;
    memset(&B, 0, sizeof(B));
    B.nArray = nArray; B.nUnit = nUnit;
    B.M_unit = sc.in<double>(M_unit, na * nUnit * 36);
    B.K_unit = sc.in<double>(K_unit, na * nUnit * 36);
    B.dC = sc.in<double>(dC, na * n * n);
    B.C_moor = A.C;
    B.M = sc.tmp<double>(na * n * n);
    B.C = C_out ? sc.out<double>(C_out, na * n * n) : sc.tmp<double>(na * n * n);
    ArrayModalArgs E;
    memset(&E, 0, sizeof(E));
    E.n = nArray;
    E.M = B.M; E.C = B.C;
    E.fn = sc.out<double>(fn, na * n);
    E.modes = sc.out<double>(modes, na * n * n);
    E.flags = sc.out<int32_t>(flags, na);
    E.moor_flags = A.flags;
    if (int rc = sc.upload("array_modal_moored")) return rc;
    if (sc.begin()) return -2;
    A.chains = chains;
    launch_array_moor(c->stream, A);
    hipLaunchKernelGGL(k_array_modal_assemble, dim3((unsigned)((na * n * n + 255) / 256)), dim3(256), 0, c->stream, B);
    launch_array_modal(c->stream, nUnit, E);
    return sc.finish();
}

// ---- eigen analysis of units with flexible members (include/raftx_flex_modal.h, raftx_flex_modal.h)
extern "C" int raftx_flex_modal_batch(raftx_ctx *c, int nSys, int n, int nModes, const double *M, const double *C, double *fn,
                                      double *modes, int32_t *flags) {
    if (!c) return -1;
    if (n < 6 || n > RAFTX_FLEX_MODAL_MAX_N) FAIL(c, "flex_modal_batch: n must be 6 to %d (got %d)", RAFTX_FLEX_MODAL_MAX_N, n);
    if (nModes < 0 || nModes > n) FAIL(c, "flex_modal_batch: nModes must be 0 to n = %d (got %d)", n, nModes);
    if (nSys < 0) FAIL(c, "flex_modal_batch: nSys must not be negative (got %d)", nSys);
    if (nSys > 0 && (!M || !C || !fn || !flags || (nModes > 0 && !modes))) FAIL(c, "flex_modal_batch: bad arguments");
    if (nSys == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    // the workgroups of the call: a few per CU, each with its own H | X | Z workspace; RAFTX_FLEX_MODAL_GRID (tests) overrides
    if (!c->nCU) {
        hipDeviceProp_t pr;
        HIPCHK(c, hipGetDeviceProperties(&pr, c->device));
        c->nCU = pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 256;
    }
    long grid = (long)FLEX_MODAL_WG_PER_CU * c->nCU;
    if (const char *env = getenv("RAFTX_FLEX_MODAL_GRID"))
        if (atol(env) > 0) grid = std::min(atol(env), 65535L);
    grid = std::min<long>(grid, nSys);
    Scratch sc(c);
    const size_t ns = (size_t)nSys, nn = (size_t)n * n;
    FlexModalArgs A;
    memset(&A, 0, sizeof(A));
    A.nSys = nSys;
    A.n = n;
    A.nModes = nModes;
    A.pitch = flex_modal_pitch(n);
    A.M = sc.in<double>(M, ns * nn);
    A.C = sc.in<double>(C, ns * nn);
    A.fn = sc.out<double>(fn, ns * n);
    A.modes = nModes ? sc.out<double>(modes, ns * n * nModes) : nullptr;
    A.flags = sc.out<int32_t>(flags, ns);
    A.work = sc.tmp<double>((size_t)grid * 3 * n * A.pitch);
    if (int rc = sc.upload("flex_modal_batch")) return rc;
    if (sc.begin()) return -2;
    hipLaunchKernelGGL(k_flex_modal, dim3((unsigned)grid), dim3(FLEX_MODAL_THREADS), 0, c->stream, A);
    return sc.finish();
}

extern "C" int raftx_sweep_mooring(raftx_ctx *c, int slot, int nLine, const double *lines, int add_stiffness, double *C_moor,
                                   double *F_moor, double *T_mean, double *T_std, int32_t *flags) {
    if (!c) return -1;
    SweepSlot *slot_ = nullptr;
    if (int rc = request_slot(c, slot, "sweep_mooring", true, &slot_)) return rc;
    SweepSlot &S = *slot_;
    if (!flags) FAIL(c, "sweep_mooring: bad arguments (flags is required)");
    const size_t n = S.bnd.empty() ? 0 : (size_t)S.bnd.back();
    int chains = 0;
    if (int rc = check_slot_lines(c, "sweep_mooring", S, n, nLine, lines, &chains)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (S.mooring.evUp) HIPCHK(c, hipEventSynchronize(S.mooring.evUp));   // (a second request on one slot: the landing area is free again)
    else HIPCHK(c, S.mooring.evUp.ensure(hipEventDisableTiming));
    S.mooring.on = false;                              // this request alone, while its landing area is rewritten: not clear_requests(), the slot's others stay
    const size_t nl = n * (size_t)nLine;
    const landing::Mooring land = landing::mooring(n, (size_t)nLine);
    HIPCHK(c, S.mooring.pin.reserve(land.need));
    MoorArgs A;
    memset(&A, 0, sizeof(A));
    A.nDesign = (int)n; A.nLine = nLine; A.depth = c->csets[S.cset].T.depth;
    A.chains = chains;
    const double *dp = nullptr;
    StagedLines L;
    int rc = 0;
    if (S.pose.on) {
        // behind a raftx_sweep_mean_pose request: at the poses its placement kernels leave on the device, so every block's
        // pose steps are enqueued now (the blocks whose phase 1 was left to raftx_sweep_launch included) and the copy stream
        // waits for them
        while (S.next_p1 < S.blk.size())
            if (const int rp = block_phase1_next(c, S)) {
                snprintf(c->err, sizeof(c->err), "sweep_mooring (block %zu): %s", S.next_p1 - 1, S.blk[S.next_p1 - 1]->err);
                S.prepared = false;
                S.clear_requests();
                return sweep_fail_drain(c, S, rp);
            }
        for (raftx_ctx *sub : S.blk) HIPCHK(c, hipStreamWaitEvent(c->sCopy, sub->evPose, 0));
        dp = S.pose.placed;
    } else
        rc = upload_on(c, c->sCopy, S.allocs, S.p1.pose, S.p1.pose ? n * 6 : 0, &dp);
    rc |= stage_lines(c, c->sCopy, S.allocs, n, nLine, lines, S.p1.var.params, L);
    double *dlw = nullptr, *dbw = nullptr, *dC = nullptr, *dF = nullptr, *dT = nullptr, *dLr = nullptr;
    int *dfl = nullptr;
    rc |= pool_alloc(c, S.allocs, nl * MOOR_LW_N, &dlw) | pool_alloc(c, S.allocs, n * 36, &dC) | pool_alloc(c, S.allocs, n * 6, &dF) |
          pool_alloc(c, S.allocs, nl * 2, &dT) | pool_alloc(c, S.allocs, nl * 36, &dLr) | pool_alloc(c, S.allocs, n, &dfl);
    if (chains == 2) rc |= pool_alloc(c, S.allocs, nl * MOOR_BW_N, &dbw);
    if (rc) return -2;
    A.bw = dbw;
    A.lw = dlw; A.C = dC; A.F = dF; A.T = dT; A.Lr = dLr; A.flags = dfl;
    A.lines = L.lines; A.pose = dp;
    if (n) {
        if (int re = expand_lines(c, c->sCopy, n, nLine, L)) return re;
        launch_moor_line(c->sCopy, A);
        launch_moor_design(c->sCopy, A);
        HIPCHK(c, hipGetLastError());
        double *p = S.mooring.pin.p;
        HIPCHK(c, hipMemcpyAsync(p + land.C, A.C, n * 36 * sizeof(double), hipMemcpyDeviceToHost, c->sCopy));
        HIPCHK(c, hipMemcpyAsync(p + land.F, A.F, n * 6 * sizeof(double), hipMemcpyDeviceToHost, c->sCopy));
        HIPCHK(c, hipMemcpyAsync(p + land.T, A.T, nl * 2 * sizeof(double), hipMemcpyDeviceToHost, c->sCopy));
        HIPCHK(c, hipMemcpyAsync(land.flags.in(p), A.flags, n * sizeof(int), hipMemcpyDeviceToHost, c->sCopy));
    }
    HIPCHK(c, hipEventRecord(S.mooring.evUp, c->sCopy));
    S.mooring.nLine = nLine;
    S.mooring.add = add_stiffness != 0;
    S.mooring.C = A.C; S.mooring.Lr = A.Lr;
    S.mooring.C_out = C_moor; S.mooring.F_out = F_moor; S.mooring.T_out = T_mean; S.mooring.Tstd_out = T_std;
    S.mooring.flags_out = flags;
    S.mooring.on = true;
    return 0;
}

// ---- the crossing at every design's mean pose (include/raftx_statics.h)
extern "C" int raftx_sweep_mean_pose(raftx_ctx *c, int slot, int nLine, const double *lines, int nX, const double *C_extra,
                                     const double *F_extra, const double *F_env, const double tol[2], int max_iter, double *pose,
                                     double *F_res, int32_t *iterations, int32_t *flags) {
    if (!c) return -1;
    SweepSlot *slot_ = nullptr;
    if (int rc = request_slot(c, slot, "sweep_mean_pose", true, &slot_)) return rc;
    SweepSlot &S = *slot_;
    if (!flags) FAIL(c, "sweep_mean_pose: bad arguments (flags is required)");
    // (unlike the other requests this one runs phase 1 again: a second one is refused, not taken in place of the first)
    if (S.pose.on) FAIL(c, "sweep_mean_pose: slot %d already has a mean-pose request", slot);
    if (S.mooring.on)
        FAIL(c, "sweep_mean_pose: slot %d already has a mooring request, which was evaluated at the caller's pose (ask for the mean pose first)", slot);
    const size_t n = S.bnd.empty() ? 0 : (size_t)S.bnd.back();
    if (nX != 0 && nX != 1 && (size_t)nX != n)
        FAIL(c, "sweep_mean_pose: nX=%d must be 0 (no extras), 1 (shared) or the %zu designs of the crossing", nX, n);
    int chains = 0;
    if (int rc = check_slot_lines(c, "sweep_mean_pose", S, n, nLine, lines, &chains)) return rc;
    double tolT, tolR;
    if (int rc = mean_pose_tol(c, "sweep_mean_pose", tol, &tolT, &tolR)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    auto &P = S.pose;
    HIPCHK(c, P.evUp.ensure(hipEventDisableTiming));
    HIPCHK(c, P.pin.reserve(landing::pose(n).need));
    const size_t nl = n * (size_t)nLine;
    StagedLines L;
    int rc = stage_lines(c, c->sCopy, S.allocs, n, nLine, lines, S.p1.var.params, L);
    rc |= upload_on(c, c->sCopy, S.allocs, C_extra, (size_t)nX * 36, &P.Cx) | upload_on(c, c->sCopy, S.allocs, F_extra, (size_t)nX * 6, &P.Fx) |
          upload_on(c, c->sCopy, S.allocs, F_env, n * 6, &P.Fenv);
    rc |= pool_alloc(c, S.allocs, n * 36, &P.K) | pool_alloc(c, S.allocs, n * 6, &P.F0) | pool_alloc(c, S.allocs, nl * MOOR_LW_N, &P.lw) |
          pool_alloc(c, S.allocs, n * 6, &P.solved) | pool_alloc(c, S.allocs, n * 6, &P.placed) | pool_alloc(c, S.allocs, n * 6, &P.Fres) |
          pool_alloc(c, S.allocs, n, &P.iter) | pool_alloc(c, S.allocs, n, &P.fl);
    P.bw = nullptr;
    if (chains == 2) rc |= pool_alloc(c, S.allocs, nl * MOOR_BW_N, &P.bw);
    if (rc) return -2;
    if (int re = expand_lines(c, c->sCopy, n, nLine, L)) return re;
    HIPCHK(c, hipEventRecord(P.evUp, c->sCopy));
    P.lines = L.lines; P.nLine = nLine; P.chains = chains; P.nX = nX; P.maxIter = max_iter; P.tolT = tolT; P.tolR = tolR;
    P.pose_out = pose; P.Fres_out = F_res; P.iter_out = iterations; P.flags_out = flags;
    P.on = true;
    // the blocks whose phase 1 raftx_sweep_prepare enqueued; raftx_sweep_launch does the others behind their phase 1
    for (size_t b = 0; b < S.next_p1 && b < S.blk.size(); b++)
        if (const int rb = block_pose(c, S, b)) {
            snprintf(c->err, sizeof(c->err), "sweep_mean_pose (block %zu): %s", b, S.blk[b]->err);
            S.prepared = false;
            S.clear_requests();
            return sweep_fail_drain(c, S, rb);
        }
    return 0;
}

// ---- output channels of a crossing (include/raftx_channels.h, raftx_channels.h)
extern "C" int raftx_sweep_channels(raftx_ctx *c, int slot, int nChan, int nL, const double *L, int nG, const raftx_c128 *Gw,
                                    double *chan_std) {
    if (!c) return -1;
    SweepSlot *slot_ = nullptr;
    if (int rc = request_slot(c, slot, "sweep_channels", false, &slot_)) return rc;
    SweepSlot &S = *slot_;
    const int n = S.bnd.empty() ? 0 : S.bnd.back();
    if (nChan < 1 || nChan > RAFTX_SWEEP_CHAN_MAX) FAIL(c, "sweep_channels: nChan=%d must be 1 .. %d", nChan, RAFTX_SWEEP_CHAN_MAX);
    if (nL != 1 && nL != n) FAIL(c, "sweep_channels: nL=%d must be 1 (shared rows) or the %d designs of the crossing", nL, n);
    if (nG != 0 && nG != 1 && nG != n) FAIL(c, "sweep_channels: nG=%d must be 0 (no Gw), 1 (shared) or the %d designs of the crossing", nG, n);
    if (nG > 0 && !Gw) FAIL(c, "sweep_channels: nG=%d without Gw", nG);
    if (!L || !chan_std) FAIL(c, "sweep_channels: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const double *dL = nullptr;
    const raftx_c128 *dG = nullptr;
    if (upload_on(c, c->sCopy, S.allocs, L, (size_t)nL * nChan * 18, &dL) ||
        upload_on(c, c->sCopy, S.allocs, Gw, nG > 0 ? (size_t)nG * nChan * 6 * S.nw : 0, &dG))
        return -2;
    HIPCHK(c, S.channels.evUp.ensure(hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(S.channels.evUp, c->sCopy));
    S.channels.nChan = nChan; S.channels.nL = nL; S.channels.nG = nG;
    S.channels.L = dL; S.channels.Gw = reinterpret_cast<const cplx *>(dG);
    S.channels.out = chan_std;
    S.channels.on = true;
    return 0;
}

extern "C" int raftx_sweep_stats(raftx_ctx *c, int nDesign, const int64_t *memberOff, const double *members,
                                 const int64_t *stationOff, const double *stations, const int64_t *capOff,
                                 const double *caps, const double *pose, double rho, double g, int add_mask,
                                 const double *M0, const double *B0, const double *C0, const double *Fz_moor, int nCase,
                                 int nHead, int nw, const double *w, const double *k, double depth, double rho_wave,
                                 double g_wave, const double *zeta, const double *beta, int nIter, double tol,
                                 double XiStart, int nChunk, int nWorker, double *sd, int32_t *niter, int32_t *flags,
                                 raftx_c128 *Xi, int64_t *stripOffsets, double *timing_ms) {
    if (!c) return -1;
    (void)nWorker;                                     // reserved (earlier versions drove the blocks from several host threads)
    int slot = 0;                                      // a blocking crossing beside streamed ones takes a free slot
    while (slot < RAFTX_NSLOT - 1 && (c->slots[slot].busy || c->slots[slot].prepared)) slot++;
    const int rc = raftx_sweep_submit(c, slot, nDesign, memberOff, members, stationOff, stations, capOff, caps, pose, rho, g, add_mask,
                                      M0, B0, C0, Fz_moor, nCase, nHead, nw, w, k, depth, rho_wave, g_wave, zeta, beta, nIter, tol,
                                      XiStart, nChunk, sd, niter, flags, Xi, stripOffsets);
    if (rc) return rc;
    return raftx_sweep_wait(c, slot, timing_ms);
}

// ------------------------------------------------------------------ RCCL exchange steps
// librccl is bound at run time (dlopen on the first raftx_comm_* call): single-GPU users never load it.
struct RcclApi {
    void *h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*Broadcast)(const void *, void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Reduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
};
static RcclApi *rccl_api(raftx_ctx *c) {
    static RcclApi api;
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (api.h) return &api;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void *h = nullptr;
    for (const char *n : names)
        if ((h = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!h) {
        snprintf(c->err, sizeof(c->err), "cannot load librccl: %s", dlerror());
        return nullptr;
    }
#define RCCL_SYM(field, name)                                                             \
    *reinterpret_cast<void **>(&api.field) = dlsym(h, name);                              \
    if (!api.field) {                                                                     \
        snprintf(c->err, sizeof(c->err), "librccl does not export %s", name);             \
        return nullptr;                                                                   \
    }
    RCCL_SYM(GetUniqueId, "ncclGetUniqueId")
    RCCL_SYM(CommInitRank, "ncclCommInitRank")
    RCCL_SYM(CommDestroy, "ncclCommDestroy")
    RCCL_SYM(GetErrorString, "ncclGetErrorString")
    RCCL_SYM(Broadcast, "ncclBroadcast")
    RCCL_SYM(Reduce, "ncclReduce")
    RCCL_SYM(AllReduce, "ncclAllReduce")
    RCCL_SYM(Send, "ncclSend")
    RCCL_SYM(Recv, "ncclRecv")
    RCCL_SYM(GroupStart, "ncclGroupStart")
    RCCL_SYM(GroupEnd, "ncclGroupEnd")
#undef RCCL_SYM
    api.h = h;
    return &api;
}
#define NCCLCHK(ctx, api, call)                                                                               \
    do {                                                                                                      \
        ncclResult_t r_ = (call);                                                                             \
        if (r_ != ncclSuccess) {                                                                              \
            snprintf((ctx)->err, sizeof((ctx)->err), "%s failed: %s (%s:%d)", #call, (api)->GetErrorString(r_), \
                     __FILE__, __LINE__);                                                                     \
            return -7;                                                                                        \
        }                                                                                                     \
    } while (0)

extern "C" int raftx_comm_unique_id(raftx_ctx *c, char *id128) {
    if (!c || !id128) return -1;
    RcclApi *R = rccl_api(c);
    if (!R) return -7;
    HIPCHK(c, hipSetDevice(c->device));
    ncclUniqueId id;
    NCCLCHK(c, R, R->GetUniqueId(&id));
    static_assert(sizeof(id) == RAFTX_COMM_ID_BYTES, "RCCL unique id size");
    memcpy(id128, &id, sizeof(id));
    return 0;
}

extern "C" int raftx_comm_destroy(raftx_ctx *c) {
    if (!c) return -1;
    if (c->comm) {
        RcclApi *R = rccl_api(c);
        if (R) {
            (void)hipSetDevice(c->device);
            (void)hipStreamSynchronize(c->stream);
            (void)R->CommDestroy(reinterpret_cast<ncclComm_t>(c->comm));
        }
        c->comm = nullptr;
    }
    c->commFlag.release();
    c->comm_rank = 0;
    c->comm_world = 1;
    return 0;
}

extern "C" int raftx_comm_init(raftx_ctx *c, int rank, int world, const char *id128) {
    if (!c || !id128) return -1;
    if (world < 1 || rank < 0 || rank >= world) FAIL(c, "comm_init: bad rank/world %d/%d", rank, world);
    if (c->comm) FAIL(c, "comm_init: this ctx already has a communicator");
    RcclApi *R = rccl_api(c);
    if (!R) return -7;
    HIPCHK(c, hipSetDevice(c->device));
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    ncclComm_t comm = nullptr;
    // the status word of comm_agree: allocated HERE so that no exchange step can fail on it later, between its peers' collectives
    if (!c->commFlag.p) HIPCHK(c, c->commFlag.grow(1));
    NCCLCHK(c, R, R->CommInitRank(&comm, world, id, rank));
    c->comm = comm;
    c->comm_rank = rank;
    c->comm_world = world;
    return 0;
}

static int comm_ready(raftx_ctx *c, RcclApi **R, int root) {
    if (!c) return -1;
    if (!c->comm) FAIL(c, "no communicator on this ctx (raftx_comm_init)");
    if (root < 0 || root >= c->comm_world) FAIL(c, "root %d outside the communicator (%d ranks)", root, c->comm_world);
    *R = rccl_api(c);
    return *R ? 0 : -7;
}

// Every exchange step starts with the ranks agreeing that all of them can go through with it: each rank validates its
// arguments and allocates its buffers FIRST, then the worst local status is MAX-reduced over the communicator (one int).
// A rank that failed locally (bad argument, allocation) therefore fails the call on EVERY rank, with an error, instead of
// leaving its peers blocked inside a send / receive it never posts.  `local_rc` 0 = ready.
static int comm_agree(raftx_ctx *c, RcclApi *R, int local_rc) {
    // the status word exists since raftx_comm_init.  A local HIP failure on the way INTO the collective is folded into
    // this rank's vote, never returned early: the AllReduce below is always posted, so the peers are not left waiting.
    // What cannot be recovered (documented in include/raftx.h): a rank whose AllReduce itself fails, or that dies.
    int mine = local_rc ? 1 : 0, worst = 0;
    hipError_t e = hipMemcpyAsync(c->commFlag.p, &mine, sizeof(int), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) {                                // vote "failed" through a device-side fill instead (no host source)
        mine = 1;
        if (!local_rc) {
            snprintf(c->err, sizeof(c->err), "comm: status upload failed: %s", hipGetErrorString(e));
            local_rc = -2;
        }
        (void)hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->commFlag.p), 1, 1, c->stream);
    }
    NCCLCHK(c, R, R->AllReduce(c->commFlag.p, c->commFlag.p, 1, ncclInt, ncclMax, reinterpret_cast<ncclComm_t>(c->comm), c->stream));
    e = hipMemcpyAsync(&worst, c->commFlag.p, sizeof(int), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (local_rc) return local_rc;                    // c->err already says why
    if (e != hipSuccess) FAIL(c, "comm: status download failed: %s", hipGetErrorString(e));
    if (worst) FAIL(c, "comm: another rank could not take part in this exchange step (see its error)");
    return 0;
}
// local preparation of an exchange step: returns its status instead of leaving the function (see comm_agree)
#define COMM_LOCAL(rc, cond, ...)                                  \
    do {                                                           \
        if (!(rc) && (cond)) {                                     \
            snprintf(c->err, sizeof(c->err), __VA_ARGS__);         \
            (rc) = -1;                                             \
        }                                                          \
    } while (0)

extern "C" int raftx_comm_broadcast(raftx_ctx *c, void *buf, size_t bytes, int root) {
    RcclApi *R = nullptr;
    if (int rc = comm_ready(c, &R, root)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    int rc = 0;
    char *d = nullptr;
    COMM_LOCAL(rc, !buf && bytes, "comm_broadcast: buf is NULL");
    if (!rc && bytes) {
        d = sc.tmp<char>(bytes);
        COMM_LOCAL(rc, !d, "comm_broadcast: device allocation failed");
    }
    if (int a = comm_agree(c, R, rc)) return a;
    if (!bytes) return 0;
    if (c->comm_rank == root) H2D(c, d, buf, bytes);
    NCCLCHK(c, R, R->Broadcast(d, d, bytes, ncclChar, root, reinterpret_cast<ncclComm_t>(c->comm), c->stream));
    if (c->comm_rank != root) D2H(c, buf, d, bytes);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// rows of every rank onto root, point to point; dsend: this rank's rows already in HBM.  `rc`: status of the caller's own
// preparation.  Everything that can fail locally (counts, root's receive buffer) is done BEFORE the ranks agree to go on;
// inside the ncclGroupStart / ncclGroupEnd pair nothing returns early.
static int gather_rows_dev(raftx_ctx *c, RcclApi *R, const void *dsend, const int64_t *counts, size_t row_bytes, void *recv_host,
                           int root, Scratch &sc, int rc) {
    const int me = c->comm_rank, world = c->comm_world;
    ncclComm_t comm = reinterpret_cast<ncclComm_t>(c->comm);
    size_t total = 0;
    for (int r = 0; r < world && !rc; r++) {
        COMM_LOCAL(rc, counts[r] < 0, "comm_gather: negative count for rank %d", r);
        if (!rc) total += (size_t)counts[r];
    }
    char *dall = nullptr;
    if (!rc && me == root) {
        COMM_LOCAL(rc, !recv_host && total, "comm_gather: recv is NULL on root");
        if (!rc && total) {
            dall = sc.tmp<char>(total * row_bytes);
            COMM_LOCAL(rc, !dall, "comm_gather: device allocation failed");
        }
    }
    if (int a = comm_agree(c, R, rc)) return a;
    ncclResult_t nr = R->GroupStart();
    hipError_t he = hipSuccess;
    if (nr == ncclSuccess) {
        if (me == root) {
            size_t o = 0;
            for (int r = 0; r < world; r++) {
                const size_t nb = (size_t)counts[r] * row_bytes;
                if (nb && nr == ncclSuccess && he == hipSuccess) {
                    if (r == me) he = hipMemcpyAsync(dall + o, dsend, nb, hipMemcpyDeviceToDevice, c->stream);
                    else nr = R->Recv(dall + o, nb, ncclChar, r, comm, c->stream);
                }
                o += nb;
            }
        } else {
            const size_t nb = (size_t)counts[me] * row_bytes;
            if (nb) nr = R->Send(dsend, nb, ncclChar, root, comm, c->stream);
        }
        const ncclResult_t ne = R->GroupEnd();        // always closed, whatever happened inside
        if (nr == ncclSuccess) nr = ne;
    }
    if (nr != ncclSuccess) {
        (void)hipStreamSynchronize(c->stream);
        FAIL(c, "comm_gather: RCCL send / receive failed: %s", R->GetErrorString(nr));
    }
    HIPCHK(c, he);
    if (me == root && total) D2H(c, recv_host, dall, total * row_bytes);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int raftx_comm_gather_rows(raftx_ctx *c, const void *send, const int64_t *counts, size_t row_bytes, void *recv,
                                      int root) {
    RcclApi *R = nullptr;
    if (int rc = comm_ready(c, &R, root)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    int rc = 0;
    COMM_LOCAL(rc, !counts || !row_bytes, "comm_gather_rows: bad arguments");
    const size_t nb = rc ? 0 : (size_t)(counts[c->comm_rank] > 0 ? counts[c->comm_rank] : 0) * row_bytes;
    char *d = nullptr;
    if (!rc && nb) {
        COMM_LOCAL(rc, !send, "comm_gather_rows: send is NULL");
        if (!rc) {
            d = sc.tmp<char>(nb);
            COMM_LOCAL(rc, !d, "comm_gather_rows: device allocation failed");
        }
        if (!rc && hipMemcpyAsync(d, send, nb, hipMemcpyHostToDevice, c->stream) != hipSuccess)
            COMM_LOCAL(rc, true, "comm_gather_rows: H2D of this rank's rows failed");
    }
    if (rc && !counts) return comm_agree(c, R, rc);   // nothing to walk: only tell the peers
    return gather_rows_dev(c, R, d, counts, row_bytes, recv, root, sc, rc);
}

extern "C" int raftx_comm_gather_xi(raftx_ctx *c, const int64_t *counts, raftx_c128 *Xi_all, int root) {
    RcclApi *R = nullptr;
    if (int rc = comm_ready(c, &R, root)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    int rc = 0;
    COMM_LOCAL(rc, !counts, "comm_gather_xi: counts is NULL");
    COMM_LOCAL(rc, !c->rXi, "comm_gather_xi: no resident results");
    COMM_LOCAL(rc, (size_t)counts[c->comm_rank] != c->r_npair, "comm_gather_xi: counts[%d] = %lld but %zu (design, case) pairs are resident",
               c->comm_rank, (long long)counts[c->comm_rank], c->r_npair);
    if (rc && !counts) return comm_agree(c, R, rc);
    const size_t row_bytes = (size_t)c->T.nHead * 6 * c->T.nw * sizeof(cplx);
    return gather_rows_dev(c, R, c->rXi, counts, row_bytes, Xi_all, root, sc, rc);
}

extern "C" int raftx_comm_reduce_sum(raftx_ctx *c, double *buf, size_t n, int root) {
    RcclApi *R = nullptr;
    if (int rc = comm_ready(c, &R, root)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    int rc = 0;
    double *d = nullptr;
    COMM_LOCAL(rc, !buf && n, "comm_reduce_sum: buf is NULL");
    if (!rc && n) {
        d = sc.tmp<double>(n);
        COMM_LOCAL(rc, !d, "comm_reduce_sum: device allocation failed");
    }
    if (int a = comm_agree(c, R, rc)) return a;
    if (!n) return 0;
    H2D(c, d, buf, n * sizeof(double));
    NCCLCHK(c, R, R->Reduce(d, d, n, ncclDouble, ncclSum, root, reinterpret_cast<ncclComm_t>(c->comm), c->stream));
    if (c->comm_rank == root) D2H(c, buf, d, n * sizeof(double));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ------------------------------------------------------------------ diagnostics
#ifdef RAFTX_PHASE_TIMING
// Tuning builds only (csrc/build.py --timing): cycles of the last raftx_solve_dynamics_device,
// summed over the first lane of every workgroup, per phase (set-up+inertial, pass A, strip
// phase, pass B, solve, tail).
extern "C" int raftx_debug_phase_cycles(raftx_ctx *c, unsigned long long *out8) {
    if (!c || !out8 || !c->dbg.p) return -1;
    HIPCHK(c, hipMemcpy(out8, c->dbg.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
}
// timing builds: the clock trace of the last fused launch -- out[2 b], out[2 b + 1] = shader cycles, 100 MHz ticks of the
// workgroups that started in the b-th 125 us of the launch (PT_FLUSH); n_bucket <= 64
extern "C" int raftx_debug_clock_trace(raftx_ctx *c, unsigned long long *out, int n_bucket) {
    if (!c || !out || !c->dbg.p || n_bucket < 1 || n_bucket > PT_CLOCK_BUCKETS) return -1;
    HIPCHK(c, hipMemcpy(out, c->dbg.p + 10, 2 * (size_t)n_bucket * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
}
#endif

__global__ void k_debug_math(int n, const double *__restrict__ x, double *__restrict__ s, double *__restrict__ c,
                             double *__restrict__ e, int table) {
    __shared__ __attribute__((aligned(16))) double tab[2 * RAFTX_SC_N];
    stage_sincos_table((ldptr)tab);
    __syncthreads();
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        if (table) tab_sincos(x[i], (ldptr)tab, s[i], c[i]);
        else fast_sincos(x[i], s[i], c[i]);
        e[i] = fast_exp(x[i]);
    }
}

extern "C" int raftx_device_synchronize(raftx_ctx *c) {
    if (!c) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    return 0;
}
extern "C" int raftx_last_solve_kernel(raftx_ctx *c, int *flags, int *waves_per_simd, int *cache_slots) {
    if (!c || c->last_flags < 0) return -1;
    if (flags) *flags = c->last_flags;
    if (waves_per_simd) *waves_per_simd = c->last_minb;
    if (cache_slots) *cache_slots = c->last_rc;
    return 0;
}
extern "C" int raftx_last_solve_launch(raftx_ctx *c, int *persistent, int *grid, int *pairs) {
    if (!c || c->last_pairs < 0) return -1;
    if (persistent) *persistent = c->last_persist;
    if (grid) *grid = c->last_grid;
    if (pairs) *pairs = c->last_pairs;
    return 0;
}
static int debug_math(raftx_ctx *c, int n, const double *x, double *sin_out, double *cos_out, double *exp_out, int table);
extern "C" int raftx_debug_math(raftx_ctx *c, int n, const double *x, double *sin_out, double *cos_out, double *exp_out) {
    return debug_math(c, n, x, sin_out, cos_out, exp_out, 0);
}
extern "C" int raftx_debug_flex_gemm(raftx_ctx *c, int K, int n, const double *A, const double *W, double *out) {
    if (!c) return -1;
    if (K < 1 || K % 6 || n < 1 || !A || !W || !out) FAIL(c, "debug_flex_gemm: K must be a multiple of 6");
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    const int64_t off[2] = {0, K / 6};
    double *dA = sc.in<double>(A, (size_t)K * n), *dW = sc.in<double>(W, (size_t)K * n), *dO = sc.out<double>(out, (size_t)n * n);
    int64_t *dOff = sc.in<int64_t>(off, 2);
    if (int rc = sc.upload("debug_flex_gemm")) return rc;
    const int nt = (n + 15) / 16;
    hipLaunchKernelGGL(k_flex_gemm_B, dim3((unsigned)((nt * nt + 3) / 4), 1), dim3(256), 0, c->stream, K / 6, 1, n, dOff, dA, dW,
                       (const int *)nullptr, dO);
    return sc.download();
}
extern "C" int raftx_debug_math_table(raftx_ctx *c, int n, const double *x, double *sin_out, double *cos_out, double *exp_out) {
    return debug_math(c, n, x, sin_out, cos_out, exp_out, 1);
}
static int debug_math(raftx_ctx *c, int n, const double *x, double *sin_out, double *cos_out, double *exp_out, int table) {
    if (!c || n < 0 || !x || !sin_out || !cos_out || !exp_out) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch sc(c);
    double *dx = sc.in<double>(x, n), *ds = sc.out<double>(sin_out, n), *dc = sc.out<double>(cos_out, n), *de = sc.out<double>(exp_out, n);
    if (int rc = sc.upload("debug_math")) return rc;
    if (n) hipLaunchKernelGGL(k_debug_math, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, dx, ds, dc, de, table);
    return sc.download();
}
