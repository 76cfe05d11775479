// raftx_array_mooring.h -- the mooring system of an ARRAY of units: anchored lines of every unit and shared lines between two
// units (included by raftx_hip.hip; entry points in include/raftx_array_mooring.h).
//
// A row is the record of raftx_mooring.h with the unit of end B in field 11 and, in field 12, 0 (end A is an anchor) or 1 + the
// unit that carries end A (a SHARED row: one suspended elastic catenary between two units).  Anchored rows -- single lines,
// composite lines, bridles -- are solved by moor_line_record<CHAINS, BRIDLES>, the body of k_moor_line, at the pose of their
// unit.  A shared row is solved by moor_shared_record below for (HF, VF) at end B with the no-contact branch of moor_eval:
// VA = VF - wL may be negative (the line sags below end A), ZF = z_B - z_A may have either sign or be exactly 0, and the ends
// are never exchanged, so nothing jumps as ZF crosses 0.  With u the horizontal direction from A to B and K3 the 3 x 3
// stiffness of the relative end motion (the expression of a single line),
//     force on unit B  (-HF u, -VF) at its arm r_B           force on unit A  (+HF u, +VA) at its arm r_A
//     C blocks         [[K3, -K3], [-K3, K3]], each carried to the reference points with its own arms as moor_line_share
//                      does; the arm-turning term -[f x][r x] of an end on that unit's diagonal block only
//     J                rows of both ends have columns for both units: (g, r_B x g) for B, (-g, -(r_A x g)) for A.
//
// Work decomposition.  k_array_moor_line: a lane per (array, row) leaves the row's record (MOOR_LW_N doubles, and for a shared
// row ARR_SW_N more: the arm and the force of end A).  k_array_moor_design: a lane per (array, unit block (i, j)) OWNS the
// 6 x 6 block (i, j) of C, walks the rows in order and adds their shares (arr_block); the lane of a diagonal block owns that
// unit's six entries of F too, the lane of block (i, 0) the six columns of unit i in every row of J (arr_unit_TJ), the lane of
// block (0, 0) T and the flags.  No atomics: an array's bits depend on its own rows and poses only.
// k_array_mean_pose: ONE workgroup of one wavefront per array runs the whole Newton iteration over the 6 nUnit DOFs.  Per step
// the lanes solve the rows (strided when nLine > 64), the records cross a barrier through memory, the lanes of the unit blocks
// run arr_block -- what k_array_moor_design runs, so C, F, T, J at the returned pose are its bits -- and [K | Y] is built in
// LDS (row stride ARR_LDA = 37 doubles, odd: a lane per row hits distinct banks) and eliminated with partial pivoting by the
// wave: every lane finds the pivot (the first row of the largest |a|, as mp_solve) from broadcast reads, a lane per column exchanges the rows, a lane per row eliminates with the pivot row read as a broadcast.  Every loop
// is bounded (max_iter, MOOR_MAX_IT line steps, 10 diagonal growths) and every barrier is uniform: the state that decides the
// control flow (flags, pivot rows, convergence) is computed by every lane from the same memory.
#pragma once

#define ARR_THREADS 64
#define ARR_SW_N 8                // a shared row's second record: r_A 0:3 | f_A 3:6 | 0 0
#define ARR_MAX_N (6 * RAFTX_ARRAY_MAX_UNIT)
#define ARR_LDA (ARR_MAX_N + 1)   // row stride of [K | Y] in LDS: 37, odd

struct ArrayMoorArgs {
    int nArray, nUnit, nLine;
    const double *__restrict__ lines;   // [nArray,nLine,RAFTX_ML_N]
    const double *__restrict__ pose;    // [nArray,nUnit,6]
    double depth;
    double *__restrict__ lw;            // [nArray,nLine,MOOR_LW_N]
    double *__restrict__ sw;            // [nArray,nLine,ARR_SW_N]
    double *__restrict__ bw;            // [nArray,nLine,MOOR_BW_N], only with bridles
    double *__restrict__ line_out;      // [nArray,nLine,MOOR_LO_N] or null
    double *__restrict__ C, *__restrict__ F, *__restrict__ T, *__restrict__ J;   // [.,n,n] [.,n] [.,2 nLine] [.,2 nLine,n], n = 6 nUnit; each or null
    int *__restrict__ flags;            // [nArray]
    int chains;                         // host side only: the kind of the records (check_lines)
};

struct ArrayPoseArgs {
    int nArray, nUnit, nLine, maxIter;
    const double *__restrict__ lines;   // [nArray,nLine,RAFTX_ML_N]
    const double *__restrict__ K_hs;    // [nArray,nUnit,36]
    const double *__restrict__ F0;      // [nArray,n]
    const double *__restrict__ F_env;   // [nArray,n] or null
    const double *__restrict__ x_ref;   // [nArray,n]
    double depth, tolT, tolR;
    double *__restrict__ lw, *__restrict__ sw, *__restrict__ bw;
    double *__restrict__ C, *__restrict__ F;             // [.,n,n] [.,n]: never null (the host lends a block where the caller wants none)
    double *__restrict__ pose, *__restrict__ T, *__restrict__ J, *__restrict__ Fres;   // each or null
    int *__restrict__ iterations;       // [nArray] or null
    int *__restrict__ flags;            // [nArray]
    int chains;                         // host side only
};

// A shared row at the poses of the units of its ends: the record lw (the layout of a single line's: the force on unit B, its
// arm, K3, the tension gradients for a relative displacement of end B, TA, TB, the flag) and sw (the arm of end A and the force
// on unit A); its line_out row at lo_out (or null).  One source for k_array_moor_line and k_array_mean_pose.  The CHAINS
// instantiations of both reach it through moor_shared_call, ONE non-inlined body, as they reach moor_chain_record.  The default
// instantiations (single rows and shared rows only) inline it, as they inline the single line's body: a call costs a kernel its
// freedom from scratch (64 B per lane for the callee-saved registers alone, measured), and the two inlined copies give the same
// bits as the two copies of moor_line_record<false> do -- tests/test_hip_array_mooring.py holds them to it.  arr_block and
// arr_unit_TJ below follow the same rule with BRIDLES (the template argument k_array_moor_design has).
__device__ __forceinline__ void moor_shared_body(const double *__restrict__ line, const MoorPose poseA, const MoorPose poseB,
                                                const double depth, double *__restrict__ lw, double *__restrict__ sw,
                                                double *__restrict__ lo_out) {
    // No multiply-add contraction in this body's own expressions: which products the compiler fuses depends on the code around
    // an inlined copy (measured: K3 of the two kernels' copies differed in the last bit; forces and tensions never did).
#pragma clang fp contract(off)
    double rec[RAFTX_ML_N], recA[RAFTX_ML_N], pa[6], pb[6];
#pragma unroll
    for (int i = 0; i < RAFTX_ML_N; i++) { rec[i] = line[i]; recA[i] = 0.0; }
    recA[3] = rec[0]; recA[4] = rec[1]; recA[5] = rec[2];        // end A as a point of its unit: moor_arm reads fields 3-5
#pragma unroll
    for (int i = 0; i < 6; i++) { pa[i] = poseA.v[i]; pb[i] = poseB.v[i]; }
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    int flag = 0;
    bool fin = true;
    for (int i = 0; i < 10; i++) fin = fin && isfinite(rec[i]);
    for (int i = 0; i < 6; i++) fin = fin && isfinite(pa[i]) && isfinite(pb[i]);
    const double L = rec[6], EA = rec[7], w = rec[8];
    double rA[3] = {0, 0, 0}, rB[3] = {0, 0, 0}, XF = 0.0, ZF = 0.0, ux = 0.0, uy = 0.0, zA = 0.0, zB = 0.0;
    if (!fin || !(L > 0.0) || !(EA > 0.0) || !(w > 0.0)) flag = RAFTX_MOOR_BAD_LINE;
    if (!flag) {
        moor_arm(recA, pa, rA);
        moor_arm(rec, pb, rB);
        const double dx = (pb[0] + rB[0]) - (pa[0] + rA[0]), dy = (pb[1] + rB[1]) - (pa[1] + rA[1]);
        XF = sqrt(dx * dx + dy * dy);
        zA = pa[2] + rA[2];
        zB = pb[2] + rB[2];
        ZF = zB - zA;
        ux = dx / XF;
        uy = dy / XF;
        if (XF <= 1e-9 * L) flag = RAFTX_MOOR_VERTICAL;         // (no SLACK: a suspended line has a catenary for every L above its chord)
    }
    double H = 0.0, V = 0.0;
    MoorEval e;
    int it = 0;
    if (!flag) {
        const double lam = (L * L <= XF * XF + ZF * ZF) ? 0.2 : sqrt(3.0 * ((L * L - ZF * ZF) / (XF * XF) - 1.0));
        H = fabs(w * XF / (2.0 * lam));
        V = 0.5 * w * (ZF / tanh(lam) + L);
        moor_eval(H, V, L, EA, w, false, e);
        double eX = e.X - XF, eZ = e.Z - ZF, res = fmax(fabs(eX), fabs(eZ)) / L, a = 1.0;
        bool conv = res == 0.0;
        while (!conv && it < MOOR_MAX_IT) {
            it++;
            const double det = e.a11 * e.a22 - e.a12 * e.a12;
            const double dH = -(e.a22 * eX - e.a12 * eZ) / det, dV = -(e.a11 * eZ - e.a12 * eX) / det;
            double s = a;
            if (H + s * dH <= 0.0) s = -0.5 * H / dH;             // keep HF > 0: at most half way to zero
            const double Ht = H + s * dH, Vt = V + s * dV;
            MoorEval n;
            moor_eval(Ht, Vt, L, EA, w, false, n);
            const double nX = n.X - XF, nZ = n.Z - ZF, rn = fmax(fabs(nX), fabs(nZ)) / L;
            if (rn < res) {
                H = Ht; V = Vt; e = n; eX = nX; eZ = nZ; res = rn; a = 1.0;
                conv = res == 0.0;
            } else if (res <= MOOR_TIGHT) {
                conv = true;
            } else {
                a *= 0.5;
                if (a < 0x1p-40) break;
            }
        }
        if (!conv) flag = RAFTX_MOOR_NO_CONVERGENCE;
    }
    const double VA = V - w * L;
    if (!flag) {
        // the lowest point: the sag where V changes sign inside the line, else the lower end
        double zlow = fmin(zA, zB);
        if (VA < 0.0 && V > 0.0) {
            const double vb = VA / H, sb = sqrt(1.0 + vb * vb);
            zlow = zA - ((H / w) * (vb * vb / (sb + 1.0)) + VA * VA / (2.0 * EA * w));
        }
        if (zlow < -depth - 1e-6 * depth) flag = RAFTX_MOOR_GROUNDED;
    }
    if (!flag) {
        const double det = e.a11 * e.a22 - e.a12 * e.a12;
        const double k11 = e.a22 / det, k12 = -e.a12 / det, k22 = e.a11 / det;
        const double TB = sqrt(H * H + V * V), TA = sqrt(H * H + VA * VA);
        const double th = H / XF;
        lw[0] = -H * ux; lw[1] = -H * uy; lw[2] = -V;
        lw[3] = rB[0]; lw[4] = rB[1]; lw[5] = rB[2];
        lw[6] = k11 * ux * ux + th * (1.0 - ux * ux);
        lw[7] = k11 * ux * uy - th * (ux * uy);
        lw[8] = k12 * ux;
        lw[9] = lw[7];
        lw[10] = k11 * uy * uy + th * (1.0 - uy * uy);
        lw[11] = k12 * uy;
        lw[12] = lw[8];
        lw[13] = lw[11];
        lw[14] = k22;
        const double gAX = (H * k11 + VA * k12) / TA, gAZ = (H * k12 + VA * k22) / TA;
        const double gBX = (H * k11 + V * k12) / TB, gBZ = (H * k12 + V * k22) / TB;
        lw[15] = gAX * ux; lw[16] = gAX * uy; lw[17] = gAZ;
        lw[18] = gBX * ux; lw[19] = gBX * uy; lw[20] = gBZ;
        lw[21] = TA;
        lw[22] = TB;
        sw[0] = rA[0]; sw[1] = rA[1]; sw[2] = rA[2];
        sw[3] = H * ux; sw[4] = H * uy; sw[5] = VA;
        sw[6] = 0.0; sw[7] = 0.0;
    }
    if (lo_out) {
        lo_out[0] = flag ? nan : H; lo_out[1] = flag ? nan : V; lo_out[2] = flag ? nan : H; lo_out[3] = flag ? nan : VA;
        lo_out[4] = flag ? nan : 0.0; lo_out[5] = flag ? nan : (double)it; lo_out[6] = flag ? nan : 0.0; lo_out[7] = flag ? nan : 0.0;
    }
    lw[23] = (double)flag;
}

__device__ __noinline__ void moor_shared_call(const double *__restrict__ line, const MoorPose poseA, const MoorPose poseB, const double depth,
                                              double *__restrict__ lw, double *__restrict__ sw, double *__restrict__ lo_out) {
    moor_shared_body(line, poseA, poseB, depth, lw, sw, lo_out);
}
template <bool CALL>
__device__ __forceinline__ void moor_shared_record(const double *__restrict__ line, const MoorPose &poseA, const MoorPose &poseB, const double depth,
                                                   double *__restrict__ lw, double *__restrict__ sw, double *__restrict__ lo_out) {
    if (CALL) moor_shared_call(line, poseA, poseB, depth, lw, sw, lo_out);
    else moor_shared_body(line, poseA, poseB, depth, lw, sw, lo_out);
}

// One row of an array at the poses x [nUnit,6] (global or LDS memory): the lane's part of k_array_moor_line, shared with
// k_array_mean_pose.  A continuation or leg row is solved by the lane of its head row, at the head row's unit.
template <bool CHAINS, bool BRIDLES>
__device__ __forceinline__ void arr_row_record(const double *__restrict__ row, const int nAfter, const double *x, const double depth,
                                               double *__restrict__ lw, double *__restrict__ sw, double *__restrict__ bw,
                                               double *__restrict__ lo_out) {
    const bool plain = row[RAFTX_ML_CONT] == 0.0 && row[RAFTX_ML_LEG] == 0.0;
    const int ub = plain ? (int)row[RAFTX_ML_UNIT_B] : 0, ua = plain ? (int)row[RAFTX_ML_UNIT_A] : 0;
    if (ua > 0) {
        MoorPose pa, pb;
#pragma unroll
        for (int i = 0; i < 6; i++) { pa.v[i] = x[6 * (ua - 1) + i]; pb.v[i] = x[6 * ub + i]; }
        moor_shared_record<CHAINS>(row, pa, pb, depth, lw, sw, lo_out);
        return;
    }
    double ps[6], lo[MOOR_LO_N];
#pragma unroll
    for (int i = 0; i < 6; i++) ps[i] = x[6 * ub + i];
    const bool mine = moor_line_record<CHAINS, BRIDLES>(row, nAfter, ps, depth, lw, lo, lo_out, bw);
    if (lo_out && mine)
#pragma unroll
        for (int i = 0; i < MOOR_LO_N; i++) lo_out[i] = lo[i];
}

// The share of a shared row (records q, s) in the block (row unit, column unit) of C, and in F of the row unit on a diagonal
// block.  iB / jB: the block's row / column unit carries end B (else end A).
__device__ __forceinline__ void arr_shared_share(const double *__restrict__ q, const double *__restrict__ s, const bool iB, const bool jB,
                                                 double C[36], double F[6]) {
    // No multiply-add contraction in this body either: its two inlined copies (k_array_moor_design, k_array_mean_pose) must
    // round alike.
#pragma clang fp contract(off)
    const bool diag = iB == jB;
    const double sg = diag ? 1.0 : -1.0;
    double ri[3], rj[3], f[3], K[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        ri[k] = iB ? q[3 + k] : s[k];
        rj[k] = jB ? q[3 + k] : s[k];
        f[k] = iB ? q[k] : s[3 + k];
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) K[i][j] = sg * q[6 + 3 * i + j];
    const double RI[3][3] = {{0.0, -ri[2], ri[1]}, {ri[2], 0.0, -ri[0]}, {-ri[1], ri[0], 0.0}};
    const double RJ[3][3] = {{0.0, -rj[2], rj[1]}, {rj[2], 0.0, -rj[0]}, {-rj[1], rj[0], 0.0}};
    const double FX[3][3] = {{0.0, -f[2], f[1]}, {f[2], 0.0, -f[0]}, {-f[1], f[0], 0.0}};
    double KR[3][3], RK[3][3];                                // K [r_j x], [r_i x] K
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            KR[i][j] = K[i][0] * RJ[0][j] + K[i][1] * RJ[1][j] + K[i][2] * RJ[2][j];
            RK[i][j] = RI[i][0] * K[0][j] + RI[i][1] * K[1][j] + RI[i][2] * K[2][j];
        }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double rkr = RI[i][0] * KR[0][j] + RI[i][1] * KR[1][j] + RI[i][2] * KR[2][j];
            const double fr = FX[i][0] * RI[0][j] + FX[i][1] * RI[1][j] + FX[i][2] * RI[2][j];     // the arm turning: the end's own unit only
            C[6 * i + j] += K[i][j];
            C[6 * i + 3 + j] += -KR[i][j];
            C[6 * (3 + i) + j] += RK[i][j];
            C[6 * (3 + i) + 3 + j] += diag ? -rkr - fr : -rkr;
        }
    if (diag) {
        F[0] += f[0]; F[1] += f[1]; F[2] += f[2];
        F[3] += ri[1] * f[2] - ri[2] * f[1];
        F[4] += ri[2] * f[0] - ri[0] * f[2];
        F[5] += ri[0] * f[1] - ri[1] * f[0];
    }
}

// The block (bi, bj) of C [n,n] of ONE array and, on a diagonal block, unit bi's entries of F [n]: the rows in order, an
// anchored row (or a whole bridle, from its head row) on the diagonal block of its unit with the sums of k_moor_design, a shared
// row on the four blocks of its two units.  lines, lw, sw, bw, C, F are the array's.  One source for k_array_moor_design and
// k_array_mean_pose.
__device__ __forceinline__ void arr_block_body(const double *__restrict__ lines, const double *lw, const double *sw, const double *bw, const int nL,
                                       const int n, const int bi, const int bj, const int bridles, double *C_out, double *F_out) {
    double C[36], F[6];
#pragma unroll
    for (int i = 0; i < 36; i++) C[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) F[i] = 0.0;
    for (int l = 0; l < nL; l++) {
        const double *row = lines + (size_t)l * RAFTX_ML_N;
        if (row[RAFTX_ML_CONT] != 0.0 || row[RAFTX_ML_LEG] != 0.0) continue;      // its head row's
        const int ub = (int)row[RAFTX_ML_UNIT_B], ua = (int)row[RAFTX_ML_UNIT_A] - 1;
        const double *q = lw + (size_t)l * MOOR_LW_N;
        if (ua >= 0) {
            if ((bi == ub || bi == ua) && (bj == ub || bj == ua)) arr_shared_share(q, sw + (size_t)l * ARR_SW_N, bi == ub, bj == ub, C, F);
            continue;
        }
        if (bi != ub || bj != ub) continue;
        if (bridles && moor_bridle_rows(row, nL - 1 - l)) {
            moor_bridle_share(bw + (size_t)l * MOOR_BW_N, C, F);
            continue;
        }
        moor_line_share(q, C, F);
    }
    if (C_out)
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j < 6; j++) C_out[(size_t)(6 * bi + i) * n + 6 * bj + j] = C[6 * i + j];
    if (F_out && bi == bj)
#pragma unroll
        for (int i = 0; i < 6; i++) F_out[6 * bi + i] = F[i];
}

__device__ __noinline__ void arr_block_call(const double *__restrict__ lines, const double *lw, const double *sw, const double *bw, const int nL,
                                           const int n, const int bi, const int bj, const int bridles, double *C_out, double *F_out) {
    arr_block_body(lines, lw, sw, bw, nL, n, bi, bj, bridles, C_out, F_out);
}
template <bool CALL>
__device__ __forceinline__ void arr_block(const double *__restrict__ lines, const double *lw, const double *sw, const double *bw, const int nL,
                                          const int n, const int bi, const int bj, double *C_out, double *F_out) {
    if (CALL) arr_block_call(lines, lw, sw, bw, nL, n, bi, bj, 1, C_out, F_out);
    else arr_block_body(lines, lw, sw, bw, nL, n, bi, bj, 0, C_out, F_out);
}

// The six columns of unit u in every row of J [2 nL,n] of ONE array, and (T not null: the lane of unit 0) T [2 nL].  A row that
// does not touch unit u has exact zeros there.  One source for both kernels, as arr_block.
__device__ __forceinline__ void arr_unit_TJ_body(const double *__restrict__ lines, const double *lw, const double *sw, const double *bw, const int nL,
                                         const int n, const int u, const int bridles, double *T, double *J) {
    int ub = 0, left = 0;                                        // the unit of the current head row; rows of its bridle still to come
    for (int l = 0; l < nL; l++) {
        const double *row = lines + (size_t)l * RAFTX_ML_N;
        int ua = -1;
        if (row[RAFTX_ML_CONT] == 0.0 && row[RAFTX_ML_LEG] == 0.0) {
            ub = (int)row[RAFTX_ML_UNIT_B];
            ua = (int)row[RAFTX_ML_UNIT_A] - 1;
            left = (bridles && ua < 0) ? moor_bridle_rows(row, nL - 1 - l) : 0;
        }
        double t2[2], j12[12];
        const double *q = lw + (size_t)l * MOOR_LW_N;
        if (left > 0) {
            moor_bridle_TJ(bw + (size_t)l * MOOR_BW_N, 0, 1, t2, j12);
            left--;
        } else
            moor_line_TJ(q, 0, 1, t2, j12);
        if (ua == u) {                                           // end A of a shared row on this unit: -g at the arm r_A
            const double *s = sw + (size_t)l * ARR_SW_N;
            double qa[MOOR_LW_N];
#pragma unroll
            for (int k = 0; k < MOOR_LW_N; k++) qa[k] = 0.0;
            qa[3] = s[0]; qa[4] = s[1]; qa[5] = s[2];
#pragma unroll
            for (int k = 15; k < 21; k++) qa[k] = -q[k];
            double ta[2];
            moor_line_TJ(qa, 0, 1, ta, j12);
        }
        const bool on = ub == u || ua == u;
        if (T) { T[l] = t2[0]; T[nL + l] = t2[1]; }
        if (J)
#pragma unroll
            for (int e = 0; e < 2; e++)
#pragma unroll
                for (int k = 0; k < 6; k++) J[(size_t)(e * nL + l) * n + 6 * u + k] = on ? j12[6 * e + k] : 0.0;
    }
}

__device__ __noinline__ void arr_unit_TJ_call(const double *__restrict__ lines, const double *lw, const double *sw, const double *bw, const int nL,
                                             const int n, const int u, const int bridles, double *T, double *J) {
    arr_unit_TJ_body(lines, lw, sw, bw, nL, n, u, bridles, T, J);
}
template <bool CALL>
__device__ __forceinline__ void arr_unit_TJ(const double *__restrict__ lines, const double *lw, const double *sw, const double *bw, const int nL,
                                            const int n, const int u, double *T, double *J) {
    if (CALL) arr_unit_TJ_call(lines, lw, sw, bw, nL, n, u, 1, T, J);
    else arr_unit_TJ_body(lines, lw, sw, bw, nL, n, u, 0, T, J);
}

template <bool CHAINS, bool BRIDLES>
__global__ void __launch_bounds__(MOOR_THREADS) k_array_moor_line(ArrayMoorArgs A) {
    const long long t = (long long)blockIdx.x * MOOR_THREADS + threadIdx.x;
    if (t >= (long long)A.nArray * A.nLine) return;
    const int a = (int)(t / A.nLine), l = (int)(t % A.nLine);
    arr_row_record<CHAINS, BRIDLES>(A.lines + (size_t)t * RAFTX_ML_N, A.nLine - 1 - l, A.pose + (size_t)a * 6 * A.nUnit, A.depth,
                                    A.lw + (size_t)t * MOOR_LW_N, A.sw + (size_t)t * ARR_SW_N,
                                    BRIDLES ? A.bw + (size_t)t * MOOR_BW_N : nullptr,
                                    A.line_out ? A.line_out + (size_t)t * MOOR_LO_N : nullptr);
}

template <bool BRIDLES>
__global__ void __launch_bounds__(MOOR_THREADS) k_array_moor_design(ArrayMoorArgs A) {
    const int N = A.nUnit, n = 6 * N, nL = A.nLine;
    const long long t = (long long)blockIdx.x * MOOR_THREADS + threadIdx.x;
    if (t >= (long long)A.nArray * N * N) return;
    const size_t a = (size_t)(t / (N * N));
    const int b = (int)(t % (N * N)), bi = b / N, bj = b % N;
    const double *lw0 = A.lw + a * nL * MOOR_LW_N;
    int flag = 0;
    for (int l = 0; l < nL; l++) flag |= (int)lw0[(size_t)l * MOOR_LW_N + 23];
    if (b == 0) A.flags[a] = flag;
    double *C = A.C ? A.C + a * n * n : nullptr, *F = A.F ? A.F + a * n : nullptr;
    double *T = A.T ? A.T + a * 2 * nL : nullptr, *J = A.J ? A.J + a * 2 * nL * n : nullptr;
    if (flag) {                                                  // a flagged array: NaN, in its own entries only
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        if (C)
            for (int i = 0; i < 36; i++) C[(size_t)(6 * bi + i / 6) * n + 6 * bj + i % 6] = nan;
        if (F && bi == bj)
            for (int i = 0; i < 6; i++) F[6 * bi + i] = nan;
        if (J && bj == 0)
            for (int r = 0; r < 2 * nL; r++)
                for (int k = 0; k < 6; k++) J[(size_t)r * n + 6 * bi + k] = nan;
        if (T && b == 0)
            for (int i = 0; i < 2 * nL; i++) T[i] = nan;
        if (A.line_out && b == 0)
            for (int i = 0; i < nL * MOOR_LO_N; i++) A.line_out[a * nL * MOOR_LO_N + i] = nan;
        return;
    }
    const double *lines = A.lines + a * nL * RAFTX_ML_N, *sw0 = A.sw + a * nL * ARR_SW_N;
    const double *bw0 = BRIDLES ? A.bw + a * nL * MOOR_BW_N : nullptr;
    if (C || (F && bi == bj)) arr_block<BRIDLES>(lines, lw0, sw0, bw0, nL, n, bi, bj, C, F);
    if (bj == 0 && (J || (T && bi == 0))) arr_unit_TJ<BRIDLES>(lines, lw0, sw0, bw0, nL, n, bi, bi == 0 ? T : nullptr, J);
}

// dX = K^-1 Y by the wave: [K | Y] (n rows of ARR_LDA doubles, Y in column n) is copied from sK to sA and eliminated there with
// partial pivoting; the solution lands in sdx.  Every lane of the workgroup calls it; returns (to every lane) false for a zero
// or non-finite pivot or a non-finite solution, as mp_solve.
__device__ __forceinline__ bool arr_solve(double *sA, const double *sK, double *sdx, const int n, const int lane) {
    for (int e = lane; e < n * ARR_LDA; e += ARR_THREADS) sA[e] = sK[e];
    __syncthreads();
    bool ok = true;
    for (int k = 0; k < n; k++) {
        int p = k;
        double best = fabs(sA[k * ARR_LDA + k]);
        for (int i = k + 1; i < n; i++) {
            const double v = fabs(sA[i * ARR_LDA + k]);
            if (v > best) { best = v; p = i; }
        }
        __syncthreads();                                         // every lane has read column k
        if (p != k && lane >= k && lane <= n) {
            const double u = sA[k * ARR_LDA + lane], v = sA[p * ARR_LDA + lane];
            sA[k * ARR_LDA + lane] = v;
            sA[p * ARR_LDA + lane] = u;
        }
        __syncthreads();
        ok = ok && best > 0.0 && isfinite(best);
        if (lane > k && lane < n) {
            const double m = sA[lane * ARR_LDA + k] / sA[k * ARR_LDA + k];
            for (int j = k + 1; j <= n; j++) sA[lane * ARR_LDA + j] = sA[lane * ARR_LDA + j] - m * sA[k * ARR_LDA + j];
        }
        __syncthreads();
    }
    for (int i = n - 1; i >= 0; i--) {
        if (lane == i) {
            double s = sA[i * ARR_LDA + n];
            for (int j = i + 1; j < n; j++) s = s - sA[i * ARR_LDA + j] * sdx[j];
            sdx[i] = s / sA[i * ARR_LDA + i];
        }
        __syncthreads();
    }
    for (int i = 0; i < n; i++) ok = ok && isfinite(sdx[i]);
    return ok;
}

template <bool CHAINS, bool BRIDLES>
__global__ void __launch_bounds__(ARR_THREADS) k_array_mean_pose(ArrayPoseArgs A) {
    __shared__ double sA[ARR_MAX_N * ARR_LDA], sK[ARR_MAX_N * ARR_LDA], sx[ARR_MAX_N], sxr[ARR_MAX_N], sdx[ARR_MAX_N];
    const int N = A.nUnit, n = 6 * N, nL = A.nLine, lane = (int)threadIdx.x;
    const size_t a = blockIdx.x;
    const double *lines = A.lines + a * nL * RAFTX_ML_N;
    double *lw0 = A.lw + a * nL * MOOR_LW_N, *sw0 = A.sw + a * nL * ARR_SW_N, *bw0 = BRIDLES ? A.bw + a * nL * MOOR_BW_N : nullptr;
    double *Cg = A.C + a * n * n, *Fg = A.F + a * n;
    if (lane < n) sx[lane] = sxr[lane] = A.x_ref[a * n + lane];
    __syncthreads();
    int it = 0, flag = 0;
    bool final = false;
    for (;;) {
        for (int l = lane; l < nL; l += ARR_THREADS)
            arr_row_record<CHAINS, BRIDLES>(lines + (size_t)l * RAFTX_ML_N, nL - 1 - l, sx, A.depth, lw0 + (size_t)l * MOOR_LW_N,
                                            sw0 + (size_t)l * ARR_SW_N, BRIDLES ? bw0 + (size_t)l * MOOR_BW_N : nullptr, nullptr);
        __syncthreads();                                         // the array's records are in memory
        int mf = 0;
        for (int l = 0; l < nL; l++) mf |= (int)lw0[(size_t)l * MOOR_LW_N + 23];
        if (mf) {
            flag |= mf;
            break;
        }
        if (lane < N * N) arr_block<BRIDLES>(lines, lw0, sw0, bw0, nL, n, lane / N, lane % N, Cg, Fg);
        if (final && lane < N && (A.T || A.J))
            arr_unit_TJ<BRIDLES>(lines, lw0, sw0, bw0, nL, n, lane, (A.T && lane == 0) ? A.T + a * 2 * nL : nullptr,
                        A.J ? A.J + a * 2 * nL * n : nullptr);
        __syncthreads();                                         // C and F are in memory
        for (int e = lane; e < n * n; e += ARR_THREADS) {
            const int r = e / n, c = e % n;
            double v = Cg[e];
            if (r / 6 == c / 6) v = A.K_hs[(a * N + r / 6) * 36 + 6 * (r % 6) + c % 6] + v;
            sK[r * ARR_LDA + c] = v;
        }
        if (lane < n) {
            const double *Kh = A.K_hs + (a * N + lane / 6) * 36 + 6 * (lane % 6);
            const int u0 = 6 * (lane / 6);
            double acc = 0.0;
            for (int j = 0; j < 6; j++) acc = acc + Kh[j] * (sx[u0 + j] - sxr[u0 + j]);
            const double base = A.F0[a * n + lane] + (A.F_env ? A.F_env[a * n + lane] : 0.0);
            const double Y = (base - acc) + Fg[lane];
            sK[lane * ARR_LDA + n] = Y;
            if (final) {                                         // the outputs at the returned pose (C, F, T, J are in place)
                if (A.pose) A.pose[a * n + lane] = sx[lane];
                if (A.Fres) A.Fres[a * n + lane] = Y;
            }
        }
        if (final) break;
        __syncthreads();
        double kmean = 0.0;
        for (int i = 0; i < n; i++) kmean = kmean + sK[i * ARR_LDA + i];
        kmean = kmean / (double)n;
        __syncthreads();
        if (lane < n && sK[lane * ARR_LDA + lane] == 0.0) sK[lane * ARR_LDA + lane] = kmean;
        __syncthreads();
        bool ok = arr_solve(sA, sK, sdx, n, lane);
        for (int tries = 0; tries < 10 && ok; tries++) {
            double dot = 0.0;
            for (int i = 0; i < n; i++) dot = dot + sdx[i] * sK[i * ARR_LDA + n];
            if (!(dot < 0.0)) break;
            __syncthreads();
            if (lane < n) sK[lane * ARR_LDA + lane] = sK[lane * ARR_LDA + lane] + 0.1 * fabs(sK[lane * ARR_LDA + lane]);
            __syncthreads();
            ok = arr_solve(sA, sK, sdx, n, lane);
        }
        if (!ok) {
            flag |= RAFTX_STATICS_SINGULAR;
            break;
        }
        double s = 1.0;
        for (int i = 0; i < n; i++) {
            const double cap = (i % 6) < 2 ? 30.0 : ((i % 6) == 2 ? 5.0 : 0.1);
            if (fabs(sdx[i]) * s > cap) s = cap / fabs(sdx[i]);
        }
        bool conv = true;
        for (int i = 0; i < n; i++) conv = conv && fabs(sdx[i] * s) <= ((i % 6) < 3 ? A.tolT : A.tolR);
        __syncthreads();                                         // every lane has read the step
        if (lane < n) sx[lane] = sx[lane] + sdx[lane] * s;
        __syncthreads();
        it++;
        if (conv) final = true;
        else if (it >= A.maxIter) {
            flag |= RAFTX_STATICS_POSE_CAP;
            break;
        }
    }
    __syncthreads();
    if (lane == 0) {
        A.flags[a] = flag;
        if (A.iterations) A.iterations[a] = it;
    }
    if (flag) {                                                  // a flagged array: NaN, in its own entries only
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        if (lane < n) {
            if (A.pose) A.pose[a * n + lane] = nan;
            A.F[a * n + lane] = nan;
            if (A.Fres) A.Fres[a * n + lane] = nan;
        }
        for (int e = lane; e < n * n; e += ARR_THREADS) Cg[e] = nan;
        if (A.T) for (int e = lane; e < 2 * nL; e += ARR_THREADS) A.T[a * 2 * nL + e] = nan;
        if (A.J) for (int e = lane; e < 2 * nL * n; e += ARR_THREADS) A.J[a * 2 * nL * n + e] = nan;
    }
}
