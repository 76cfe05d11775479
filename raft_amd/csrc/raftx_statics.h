// raftx_statics.h -- the mean equilibrium pose of every design (included by raftx_hip.hip; entry point in
// include/raftx_statics.h): Model.solveStatics for staticsMod 0 / forcingMod 0, rigid 6-DOF units with lines of their own.
//
//   Y(x) = F0 + F_env - K_hs (x - x_ref) + F_moor(x) = 0         K = K_hs + C_moor(x)         x <- x + K^-1 Y
//
// with the safeguards of raft_model.py:824-861 (a zero diagonal takes the mean diagonal; LU with partial pivoting; while
// dX.Y < 0 the diagonal grows by 10 %, at most ten times) and the step bounds of :667 by one common factor.
//
// Work decomposition: k_mean_pose is ONE launch for the whole iteration of the whole batch.  A design has a group of G lanes
// (G = the power of two at or above nLine, at most 64; a workgroup is one wavefront of 64 / G designs).  Per step the lanes of
// a group solve the design's lines in parallel -- moor_line_record, the body of k_moor_line, cold start -- into the records lw
// in global memory; after a workgroup barrier EVERY lane of the group gathers the records in line order (moor_design_sums, the
// walk and the sums of k_moor_design: the same bits), forms Y and K and takes the step, so the group needs no broadcast: its lanes hold the
// same x, bit for bit.  The records cross the barrier through memory, as between k_moor_line and k_moor_design, so no
// multiply-add is contracted across the two halves that those kernels could not contract either: C_moor, F_moor, T, J are what
// raftx_mooring_lines returns at the returned pose.  The loop is uniform over the workgroup (__syncthreads_or): a finished
// design idles and its state is frozen, so a design's bits depend on its own inputs only -- not on its neighbours, the batch or
// the grid.  No atomics; the only LDS is the 256 B behind __syncthreads_or.
#pragma once

#define MP_THREADS 64
#define MP_MAX_IT 40

struct MeanPoseArgs {
    int nDesign, nLine, G, maxIter;
    const double *__restrict__ lines;   // [nDesign,nLine,RAFTX_ML_N]
    const double *__restrict__ K_hs;    // [nDesign,36]
    const double *__restrict__ F0;      // [nDesign,6]
    const double *__restrict__ F_env;   // [nDesign,6] or null
    const double *__restrict__ x_ref;   // [nDesign,6] or null
    double depth, tolT, tolR;
    double *__restrict__ lw;            // [nDesign,nLine,MOOR_LW_N]
    double *__restrict__ pose, *__restrict__ C, *__restrict__ F, *__restrict__ T, *__restrict__ J, *__restrict__ Fres;   // each or null
    int *__restrict__ iterations;       // [nDesign] or null
    int *__restrict__ flags;            // [nDesign]
    int chains;                         // host side only: 1 a continuation row among the records, so k_mean_pose<true> runs; 2 a leg row
    double *__restrict__ bw;            // [nDesign,nLine,MOOR_BW_N], only with bridles
};

// dX = K^-1 Y by Gaussian elimination of [K | Y] with partial pivoting (the first row of the largest |a|, as LAPACK's gesv
// behind np.linalg.solve).  Rows are exchanged by selects so that every register index is static.  Returns false for a zero or
// non-finite pivot or a non-finite solution.
__device__ __forceinline__ bool mp_solve(const double K[36], const double Y[6], double dX[6]) {
    double A[6][7];
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = 0; j < 6; j++) A[i][j] = K[6 * i + j];
        A[i][6] = Y[i];
    }
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        int p = k;
        double best = fabs(A[k][k]);
#pragma unroll
        for (int i = k + 1; i < 6; i++) {
            const double a = fabs(A[i][k]);
            if (a > best) { best = a; p = i; }
        }
#pragma unroll
        for (int i = k + 1; i < 6; i++) {
            const bool sw = p == i;
#pragma unroll
            for (int j = k; j < 7; j++) {
                const double u = A[k][j], v = A[i][j];
                A[k][j] = sw ? v : u;
                A[i][j] = sw ? u : v;
            }
        }
        ok = ok && best > 0.0 && isfinite(best);
#pragma unroll
        for (int i = k + 1; i < 6; i++) {
            const double m = A[i][k] / A[k][k];
#pragma unroll
            for (int j = k + 1; j < 7; j++) A[i][j] = A[i][j] - m * A[k][j];
        }
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double s = A[i][6];
#pragma unroll
        for (int j = i + 1; j < 6; j++) s = s - A[i][j] * dX[j];
        dX[i] = s / A[i][i];
    }
#pragma unroll
    for (int i = 0; i < 6; i++) ok = ok && isfinite(dX[i]);
    return ok;
}

template <bool CHAINS, bool BRIDLES = false>
__global__ void __launch_bounds__(MP_THREADS) k_mean_pose(MeanPoseArgs A) {
    const int G = A.G, nL = A.nLine;
    const int d = blockIdx.x * (MP_THREADS / G) + (int)threadIdx.x / G, g = (int)threadIdx.x % G;
    const bool live = d < A.nDesign;
    const size_t dd = live ? (size_t)d : 0;
    double x[6], xr[6];
#pragma unroll
    for (int i = 0; i < 6; i++) x[i] = xr[i] = (live && A.x_ref) ? A.x_ref[dd * 6 + i] : 0.0;
    double *lw0 = A.lw + dd * nL * MOOR_LW_N;
    const double *lines = A.lines + dd * nL * RAFTX_ML_N, *bw0 = BRIDLES ? A.bw + dd * nL * MOOR_BW_N : nullptr;
    int it = 0, flag = 0;
    int phase = live ? 0 : 2;                                    // 0 iterating, 1 converged: the outputs at x are due, 2 finished
    for (;;) {
        if (phase < 2)
            for (int l = g; l < nL; l += G) {
                double lo[MOOR_LO_N];
                moor_line_record<CHAINS, BRIDLES>(A.lines + (dd * nL + l) * RAFTX_ML_N, nL - 1 - l, x, A.depth, lw0 + (size_t)l * MOOR_LW_N,
                                                  lo, nullptr, BRIDLES ? A.bw + (dd * nL + l) * MOOR_BW_N : nullptr);
            }
        __syncthreads();                                         // the group's records are in memory
        if (phase < 2) {
            int mf = 0;
            for (int l = 0; l < nL; l++) mf |= (int)lw0[(size_t)l * MOOR_LW_N + 23];
            if (mf) {
                flag |= mf;
                phase = 2;
            } else {
                double C[36], F[6], Y[6];
                moor_design_sums<BRIDLES>(lines, lw0, bw0, nL, C, F);       // k_moor_design's walk: a bridle from its head row, once
                const double *Kh = A.K_hs + dd * 36;
#pragma unroll
                for (int i = 0; i < 6; i++) {
                    double acc = 0.0;
#pragma unroll
                    for (int j = 0; j < 6; j++) acc = acc + Kh[6 * i + j] * (x[j] - xr[j]);
                    const double base = A.F0[dd * 6 + i] + (A.F_env ? A.F_env[dd * 6 + i] : 0.0);
                    Y[i] = (base - acc) + F[i];
                }
                if (phase == 1) {                                // the outputs at the returned pose; lane 0 of the group writes
                    if (g == 0) {
#pragma unroll
                        for (int i = 0; i < 6; i++) {
                            if (A.pose) A.pose[dd * 6 + i] = x[i];
                            if (A.F) A.F[dd * 6 + i] = F[i];
                            if (A.Fres) A.Fres[dd * 6 + i] = Y[i];
                        }
                        if (A.C)
#pragma unroll
                            for (int i = 0; i < 36; i++) A.C[dd * 36 + i] = C[i];
                        if (A.T || A.J)
                            moor_design_TJ<BRIDLES>(lines, lw0, bw0, nL, A.T ? A.T + dd * 2 * nL : nullptr, A.J ? A.J + dd * 12 * nL : nullptr);
                    }
                    phase = 2;
                } else {                                         // (the step: mp_newton_step below is this text once more, for k_mean_pose_nl -- keep them alike)
                    double K[36], dX[6];
#pragma unroll
                    for (int i = 0; i < 36; i++) K[i] = Kh[i] + C[i];
                    double kmean = 0.0;
#pragma unroll
                    for (int i = 0; i < 6; i++) kmean = kmean + K[7 * i];
                    kmean = kmean / 6.0;
#pragma unroll
                    for (int i = 0; i < 6; i++)
                        if (K[7 * i] == 0.0) K[7 * i] = kmean;
                    bool ok = mp_solve(K, Y, dX);
                    for (int tries = 0; tries < 10 && ok; tries++) {
                        double dot = 0.0;
#pragma unroll
                        for (int i = 0; i < 6; i++) dot = dot + dX[i] * Y[i];
                        if (!(dot < 0.0)) break;
#pragma unroll
                        for (int i = 0; i < 6; i++) K[7 * i] = K[7 * i] + 0.1 * fabs(K[7 * i]);
                        ok = mp_solve(K, Y, dX);
                    }
                    if (!ok) {
                        flag |= RAFTX_STATICS_SINGULAR;
                        phase = 2;
                    } else {
                        const double cap[6] = {30.0, 30.0, 5.0, 0.1, 0.1, 0.1};
                        double s = 1.0;
#pragma unroll
                        for (int i = 0; i < 6; i++)
                            if (fabs(dX[i]) * s > cap[i]) s = cap[i] / fabs(dX[i]);
                        bool conv = true;
#pragma unroll
                        for (int i = 0; i < 6; i++) {
                            dX[i] = dX[i] * s;
                            conv = conv && fabs(dX[i]) <= (i < 3 ? A.tolT : A.tolR);
                            x[i] = x[i] + dX[i];
                        }
                        it++;
                        if (conv) phase = 1;
                        else if (it >= A.maxIter) {
                            flag |= RAFTX_STATICS_POSE_CAP;
                            phase = 2;
                        }
                    }
                }
            }
        }
        if (!__syncthreads_or(phase < 2)) break;                 // (also: every lane has read the records before they are rewritten)
    }
    if (!live || g != 0) return;
    A.flags[d] = flag;
    if (A.iterations) A.iterations[d] = it;
    if (flag) {                                                  // a flagged design: NaN, in its own rows only
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        for (int i = 0; i < 6; i++) {
            if (A.pose) A.pose[dd * 6 + i] = nan;
            if (A.F) A.F[dd * 6 + i] = nan;
            if (A.Fres) A.Fres[dd * 6 + i] = nan;
        }
        if (A.C) for (int i = 0; i < 36; i++) A.C[dd * 36 + i] = nan;
        if (A.T) for (int i = 0; i < 2 * nL; i++) A.T[dd * 2 * nL + i] = nan;
        if (A.J) for (int i = 0; i < 12 * nL; i++) A.J[dd * 12 * nL + i] = nan;
    }
}

// ---- staticsMod 1 (raftx_mean_pose_nonlinear): buoyancy and weight re-evaluated at every iterate (raft_model.py:705-712, :797-800)
//
//   Y(x) = W_struc(x) + W_hydro(x) + W_pm(x) + F_extra - C_extra (x - x_ref) + F_env + F_moor(x)
//   K(x) = C_struc(x) + C_hydro(x) + C_pm(x) + C_extra + C_moor(x)
//
// k_mean_pose_nl is ONE launch for the whole iteration of the whole batch, in the layout of k_mean_pose: a design has a group
// of G lanes (mean_pose_nl_group: the power of two at or above max(members of a design, nLine), at most NL_MAX_G; a workgroup
// is one wavefront of 64 / G designs).  Per iterate
//   1. the lanes of a group take the design's members in parallel -- geom_member_body at the iterate, the body of
//      k_geom_member, then geom_member_inertia with the ballast-density correction where drho is given, the body of
//      k_geom_reinertia -- into the records mw (mp | mh | mi per member) and mflag in global memory, and its lines as
//      k_mean_pose does, into lw;
//   2. after a barrier, lanes 0 and 1 of the group do the member -> platform reductions of k_geom_reduce for its roles 0
//      (C_hydro, W_hydro) and 1 (C_struc, W_struc) -- nl_reduce: the same member order, the same sums, the same
//      symmetrisation -- into red;
//   3. after a second barrier EVERY lane of the group reads red, gathers the line records, adds the point masses and the
//      extras, and takes the step of k_mean_pose (mp_newton_step), so the group needs no broadcast.
// Records cross each barrier through memory, as between k_geom_member, k_geom_reduce and the mooring kernels, and the geometry
// runs with contraction off: K_hs and F0 at the returned pose are the bits of raftx_build_designs at that pose, C_moor,
// F_moor, T, J those of raftx_mooring_lines.  The loop is uniform over the workgroup; a finished or flagged design idles with
// its state frozen.  A non-finite iterate is flagged (RAFTX_STATICS_SINGULAR) BEFORE the member pass: geom_member_body never
// sees one.  No atomics; no LDS but the 256 B behind __syncthreads_or.
#define NL_MAX_G 32
#define NL_RED_N 84               // C_hydro 0:36 | W_hydro 36:42 | C_struc 42:78 | W_struc 78:84

struct MeanPoseNlArgs {
    MeanPoseArgs P;                     // the lines, F_env, x_ref, the settings, lw / bw and the outputs of k_mean_pose; P.K_hs and P.F0 are not read
    int nM;                             // rows of the program: members of every design; else 0
    const int64_t *memberOff;           // [nDesign+1]; rows of the program: null (design d has members d nM ...)
    const int64_t *stationOff, *capOff; // [nMember+1] (capOff or null); rows of the program: the base unit's, [nM+1]
    const double *gm, *gs, *gc;         // the caller's rows; rows of the program: null
    VariantView prog;                   // rows of the program: prog.params [nDesign,nP] on the device
    double rho, g;
    const double *drho;                 // [nDesign] or null
    int nPM, nX;                        // point masses per design; 0: no pm / Cx / Fx, 1: shared, nDesign: one set each
    const double *pm, *Cx, *Fx;         // [nX,nPM,4] [nX,36] [nX,6], each or null
    double *mw;                         // [nMember,FR_N]
    int *mflag;                         // [nMember]
    double *red;                        // [nDesign,NL_RED_N]
    double *K_out, *F0_out;             // [nDesign,36] [nDesign,6], each or null
};

// one member of design d at the iterate x: record wm of mw / mflag
template <class Rows>
__device__ __forceinline__ void nl_member_run(const MeanPoseNlArgs &A, const Rows &rows, const int n, const int ncap, const int d,
                                              const size_t wm, const double *x) {
    GEOM_NOFMA
    double *mp = A.mw + wm * FR_N, *mh = mp + MP_N, *mi = mh + MH_N;
    const GMember R = geom_member_body(rows, n, ncap, x, A.rho, A.g, A.drho != nullptr, true, mp, mh, mi);
    int bad = (R.rej | R.code) != 0;
    if (!bad && A.drho && !((int)rows.mcol(RAFTX_GM_FLAGS) & RAFTX_GM_FLAG_NOSTATIC))
        bad = geom_member_inertia(rows, n, ncap, mp + 3, mp + 6, mp + 9, mp + 12, A.g, true, A.drho[d], mi) != 0;
    A.mflag[wm] = bad;
}
template <class Rows>
__device__ __forceinline__ void nl_member(const MeanPoseNlArgs &A, const int d, const int k, const size_t wm, const double *x) {
    if constexpr (std::is_same<Rows, GeomRowsProg>::value) {
        const int s0 = (int)A.stationOff[k], c0 = A.capOff ? (int)A.capOff[k] : 0;
        const int n = (int)A.stationOff[k + 1] - s0, ncap = A.capOff ? (int)A.capOff[k + 1] - c0 : 0;
        const GeomRowsProg rows(A.prog, k, s0, c0, d);
        nl_member_run(A, rows, n, ncap, d, wm, x);
    } else {
        const int64_t s0 = A.stationOff[wm], c0 = A.capOff ? A.capOff[wm] : 0;
        const int n = (int)(A.stationOff[wm + 1] - s0), ncap = A.capOff ? (int)(A.capOff[wm + 1] - c0) : 0;
        const GeomRowsPlain rows{A.gm + wm * RAFTX_GM_N, A.gs + (size_t)s0 * RAFTX_GS_N, A.capOff ? A.gc + (size_t)c0 * RAFTX_GC_N : nullptr};
        nl_member_run(A, rows, n, ncap, d, wm, x);
    }
}
// role 0 | 1 of k_geom_reduce over the nM records at mw, at the pose x: dst[0:36] the symmetrised matrix, dst[36:42] the vector
__device__ inline void nl_reduce(const double *mw, const int nM, const int role, const double (&x)[6], double *dst) {
    GEOM_NOFMA
    const double th[3] = {x[3], x[4], x[5]}, rP[3] = {x[0], x[1], x[2]};
    double out[36], Wv[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 36; i++) out[i] = 0.0;
    for (int m = 0; m < nM; m++) {
        const double *mp = mw + (size_t)m * FR_N, *mh = mp + MP_N, *mi = mh + MH_N;
        const double a[3] = {mp[3] - rP[0], mp[4] - rP[1], mp[5] - rP[2]};
        double C[36];
        if (role == 1) {
            for (int i = 0; i < 36; i++) C[i] = 0.0;
            C[3 * 6 + 3] = C[4 * 6 + 4] = mi[46];
        } else {
            for (int i = 0; i < 36; i++) C[i] = mh[i];
        }
        geom_reduce_matrix(C, a, out);
        geom_reduce_vector(role == 0 ? mh + 36 : mi + 40, a, mp, th, Wv, out);
    }
    for (int i = 0; i < 6; i++)
        for (int j = i + 1; j < 6; j++) {
            const double s = (out[i * 6 + j] + out[j * 6 + i]) / 2;
            out[i * 6 + j] = out[j * 6 + i] = s;
        }
    for (int i = 0; i < 36; i++) dst[i] = out[i];
    for (int i = 0; i < 6; i++) dst[36 + i] = Wv[i];
}
// The point masses pm [nPM,4] = (mass, x, y, z about the PRP, in the unit's frame) at the pose x: every one a node that
// carries the force (0, 0, -m g) and no stiffness, reduced with geom_reduce_vector from the arm R_p r (R_p: the platform
// rotation of geom_pose) and the undisplaced arm r; the geometric stiffness symmetrised as a member's is.
__device__ inline void nl_point_masses(const double *pm, const int nPM, const double (&x)[6], const double g, double (&W)[6], double (&C)[36]) {
    GEOM_NOFMA
    const double sy = sin(x[5]), cy = cos(x[5]), sp = sin(x[4]), cp = cos(x[4]), sr = sin(x[3]), cr = cos(x[3]);
    const double Rp[3][3] = {{cy * cp, cy * sp * sr - cr * sy, sy * sr + cy * cr * sp},
                             {cp * sy, cy * cr + sy * sp * sr, cr * sy * sp - cy * sr},
                             {-sp, cp * sr, cp * cr}};
    const double th[3] = {x[3], x[4], x[5]};
    for (int i = 0; i < 6; i++) W[i] = 0.0;
    for (int i = 0; i < 36; i++) C[i] = 0.0;
    for (int p = 0; p < nPM; p++) {
        const double *r = pm + 4 * p + 1;
        const double a[3] = {Rp[0][0] * r[0] + Rp[0][1] * r[1] + Rp[0][2] * r[2], Rp[1][0] * r[0] + Rp[1][1] * r[1] + Rp[1][2] * r[2],
                             Rp[2][0] * r[0] + Rp[2][1] * r[1] + Rp[2][2] * r[2]};
        const double Wn[6] = {0.0, 0.0, -(pm[4 * p] * g), 0.0, 0.0, 0.0};
        geom_reduce_vector(Wn, a, r, th, W, C);
    }
    for (int i = 0; i < 6; i++)
        for (int j = i + 1; j < 6; j++) {
            const double s = (C[i * 6 + j] + C[j * 6 + i]) / 2;
            C[i * 6 + j] = C[j * 6 + i] = s;
        }
}
// The step of k_mean_pose on K (modified in place) and Y: the repaired diagonal, the solve, the diagonal growth while
// dX.Y < 0, the caps by one factor; x <- x + dX.  false: singular.  conv: that step was within the tolerances.
__device__ __forceinline__ bool mp_newton_step(double (&K)[36], const double (&Y)[6], double (&x)[6], const double tolT, const double tolR,
                                               bool &conv) {
    double dX[6], kmean = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) kmean = kmean + K[7 * i];
    kmean = kmean / 6.0;
#pragma unroll
    for (int i = 0; i < 6; i++)
        if (K[7 * i] == 0.0) K[7 * i] = kmean;
    bool ok = mp_solve(K, Y, dX);
    for (int tries = 0; tries < 10 && ok; tries++) {
        double dot = 0.0;
#pragma unroll
        for (int i = 0; i < 6; i++) dot = dot + dX[i] * Y[i];
        if (!(dot < 0.0)) break;
#pragma unroll
        for (int i = 0; i < 6; i++) K[7 * i] = K[7 * i] + 0.1 * fabs(K[7 * i]);
        ok = mp_solve(K, Y, dX);
    }
    if (!ok) return false;
    const double cap[6] = {30.0, 30.0, 5.0, 0.1, 0.1, 0.1};
    double s = 1.0;
#pragma unroll
    for (int i = 0; i < 6; i++)
        if (fabs(dX[i]) * s > cap[i]) s = cap[i] / fabs(dX[i]);
    conv = true;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        dX[i] = dX[i] * s;
        conv = conv && fabs(dX[i]) <= (i < 3 ? tolT : tolR);
        x[i] = x[i] + dX[i];
    }
    return true;
}

template <class Rows, bool CHAINS, bool BRIDLES>
__global__ void __launch_bounds__(MP_THREADS) k_mean_pose_nl(MeanPoseNlArgs N) {
    const MeanPoseArgs &A = N.P;
    const int G = A.G, nL = A.nLine;
    const int d = blockIdx.x * (MP_THREADS / G) + (int)threadIdx.x / G, g = (int)threadIdx.x % G;
    const bool live = d < A.nDesign;
    const size_t dd = live ? (size_t)d : 0;
    constexpr bool PROG = std::is_same<Rows, GeomRowsProg>::value;
    const size_t m0 = PROG ? dd * (size_t)N.nM : (size_t)N.memberOff[dd];
    const int nM = PROG ? N.nM : (int)((size_t)N.memberOff[dd + 1] - m0);
    double x[6], xr[6];
#pragma unroll
    for (int i = 0; i < 6; i++) x[i] = xr[i] = (live && A.x_ref) ? A.x_ref[dd * 6 + i] : 0.0;
    double *lw0 = A.lw + dd * nL * MOOR_LW_N, *red = N.red + dd * NL_RED_N;
    const double *mw0 = N.mw + m0 * FR_N;
    const double *lines = A.lines + dd * nL * RAFTX_ML_N, *bw0 = BRIDLES ? A.bw + dd * nL * MOOR_BW_N : nullptr;
    const size_t xi = N.nX > 1 ? dd : 0;
    const double *pm = (N.nX && N.nPM) ? N.pm + xi * 4 * N.nPM : nullptr, *Cx = (N.nX && N.Cx) ? N.Cx + xi * 36 : nullptr,
                 *Fx = (N.nX && N.Fx) ? N.Fx + xi * 6 : nullptr;
    int it = 0, flag = 0;
    int phase = live ? 0 : 2;                                    // 0 iterating, 1 converged: the outputs at x are due, 2 finished
    for (;;) {
        if (phase < 2) {
            bool fin = true;
#pragma unroll
            for (int i = 0; i < 6; i++) fin = fin && isfinite(x[i]);
            if (!fin) {                                          // (every lane of the group holds the same x)
                flag |= RAFTX_STATICS_SINGULAR;
                phase = 2;
            }
        }
        if (phase < 2) {
            for (int k = g; k < nM; k += G) nl_member<Rows>(N, d, k, m0 + k, x);
            for (int l = g; l < nL; l += G) {
                double lo[MOOR_LO_N];
                moor_line_record<CHAINS, BRIDLES>(A.lines + (dd * nL + l) * RAFTX_ML_N, nL - 1 - l, x, A.depth, lw0 + (size_t)l * MOOR_LW_N,
                                                  lo, nullptr, BRIDLES ? A.bw + (dd * nL + l) * MOOR_BW_N : nullptr);
            }
        }
        __syncthreads();                                         // the group's member and line records are in memory
        if (phase < 2) {
            int mf = 0;
            for (int l = 0; l < nL; l++) mf |= (int)lw0[(size_t)l * MOOR_LW_N + 23];
            for (int k = 0; k < nM; k++) mf |= N.mflag[m0 + k] ? RAFTX_STATICS_BAD_MEMBER : 0;
            if (mf) {
                flag |= mf;
                phase = 2;
            } else
                for (int role = g; role < 2; role += G) nl_reduce(mw0, nM, role, x, red + role * 42);
        }
        __syncthreads();                                         // ... and its two reductions
        if (phase < 2) {
            double C[36], F[6], Y[6], Kh[36], W0[6];
            moor_design_sums<BRIDLES>(lines, lw0, bw0, nL, C, F);
#pragma unroll
            for (int i = 0; i < 36; i++) Kh[i] = red[42 + i] + red[i];                          // C_struc + C_hydro
#pragma unroll
            for (int i = 0; i < 6; i++) W0[i] = red[78 + i] + red[36 + i];                      // W_struc + W_hydro
            if (pm) {
                double Wp[6], Cp[36];
                nl_point_masses(pm, N.nPM, x, N.g, Wp, Cp);
#pragma unroll
                for (int i = 0; i < 36; i++) Kh[i] = Kh[i] + Cp[i];
#pragma unroll
                for (int i = 0; i < 6; i++) W0[i] = W0[i] + Wp[i];
            }
            if (Cx)
#pragma unroll
                for (int i = 0; i < 36; i++) Kh[i] = Kh[i] + Cx[i];
            if (Fx)
#pragma unroll
                for (int i = 0; i < 6; i++) W0[i] = W0[i] + Fx[i];
#pragma unroll
            for (int i = 0; i < 6; i++) {
                double acc = 0.0;
                if (Cx)
#pragma unroll
                    for (int j = 0; j < 6; j++) acc = acc + Cx[6 * i + j] * (x[j] - xr[j]);
                Y[i] = ((W0[i] - acc) + (A.F_env ? A.F_env[dd * 6 + i] : 0.0)) + F[i];
            }
            if (phase == 1) {                                    // the outputs at the returned pose; lane 0 of the group writes
                if (g == 0) {
#pragma unroll
                    for (int i = 0; i < 6; i++) {
                        if (A.pose) A.pose[dd * 6 + i] = x[i];
                        if (A.F) A.F[dd * 6 + i] = F[i];
                        if (A.Fres) A.Fres[dd * 6 + i] = Y[i];
                        if (N.F0_out) N.F0_out[dd * 6 + i] = W0[i];
                    }
                    if (A.C)
#pragma unroll
                        for (int i = 0; i < 36; i++) A.C[dd * 36 + i] = C[i];
                    if (N.K_out)
#pragma unroll
                        for (int i = 0; i < 36; i++) N.K_out[dd * 36 + i] = Kh[i];
                    if (A.T || A.J)
                        moor_design_TJ<BRIDLES>(lines, lw0, bw0, nL, A.T ? A.T + dd * 2 * nL : nullptr, A.J ? A.J + dd * 12 * nL : nullptr);
                }
                phase = 2;
            } else {
                double K[36];
#pragma unroll
                for (int i = 0; i < 36; i++) K[i] = Kh[i] + C[i];
                bool conv = false;
                if (!mp_newton_step(K, Y, x, A.tolT, A.tolR, conv)) {
                    flag |= RAFTX_STATICS_SINGULAR;
                    phase = 2;
                } else {
                    it++;
                    if (conv) phase = 1;
                    else if (it >= A.maxIter) {
                        flag |= RAFTX_STATICS_POSE_CAP;
                        phase = 2;
                    }
                }
            }
        }
        if (!__syncthreads_or(phase < 2)) break;                 // (also: every lane has read the records before they are rewritten)
    }
    if (!live || g != 0) return;
    A.flags[d] = flag;
    if (A.iterations) A.iterations[d] = it;
    if (flag) {                                                  // a flagged design: NaN, in its own rows only
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        for (int i = 0; i < 6; i++) {
            if (A.pose) A.pose[dd * 6 + i] = nan;
            if (A.F) A.F[dd * 6 + i] = nan;
            if (A.Fres) A.Fres[dd * 6 + i] = nan;
            if (N.F0_out) N.F0_out[dd * 6 + i] = nan;
        }
        if (A.C) for (int i = 0; i < 36; i++) A.C[dd * 36 + i] = nan;
        if (N.K_out) for (int i = 0; i < 36; i++) N.K_out[dd * 36 + i] = nan;
        if (A.T) for (int i = 0; i < 2 * nL; i++) A.T[dd * 2 * nL + i] = nan;
        if (A.J) for (int i = 0; i < 12 * nL; i++) A.J[dd * 12 * nL + i] = nan;
    }
}
static inline int mean_pose_nl_group(int maxMember, int nLine) {
    const int want = maxMember > nLine ? maxMember : nLine;
    int G = 1;
    while (G < want && G < NL_MAX_G) G *= 2;
    return G;
}

// ---- the solve inside a sweep crossing (raftx_sweep_mean_pose): two small kernels around k_mean_pose, per block of the crossing.
// k_pose_assemble forms the solve's inputs from what the member -> platform reductions left at the reference pose,
//   K_hs = (C_struc + C_hydro) + C_extra          F0 = (W_struc + W_hydro) + F_extra
// in the association of raft_amd/statics.py hydrostatics(): sums only, nothing to contract, so the bits are NumPy's.  An absent
// extra adds nothing (not even a zero: -0 stays -0).  strideC / strideF: 36 / 6 for per-design extras, 0 for shared ones.
struct PoseAssembleArgs {
    int n;
    const double *__restrict__ Cs, *__restrict__ Ch, *__restrict__ Ws, *__restrict__ Wh;   // [n,36] [n,36] [n,6] [n,6]
    const double *__restrict__ Cx, *__restrict__ Fx;                                       // at the block's first design, or null
    size_t strideC, strideF;
    double *__restrict__ K, *__restrict__ F0;                                              // [n,36] [n,6]
};
__global__ void __launch_bounds__(256) k_pose_assemble(PoseAssembleArgs A) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nK = (size_t)A.n * 36, nF = (size_t)A.n * 6;
    if (t < nK) {
        double v = A.Cs[t] + A.Ch[t];
        if (A.Cx) v = v + A.Cx[(t / 36) * A.strideC + t % 36];
        A.K[t] = v;
    } else if (t < nK + nF) {
        const size_t u = t - nK;
        double v = A.Ws[u] + A.Wh[u];
        if (A.Fx) v = v + A.Fx[(u / 6) * A.strideF + u % 6];
        A.F0[u] = v;
    }
}
// k_pose_place, one lane per design: the pose the block's second member pass runs at -- the solved one, or the reference pose
// for a flagged design (its solved pose is NaN, and a NaN pose must never reach geom_member_body: its rejections abort a whole
// batch) -- and the solve's outputs straight into the slot's page-locked landing area (no small D2H copy to queue on the DMA
// engine), the flagged design's as NaN as k_mean_pose left them.
struct PosePlaceArgs {
    int n;
    const double *__restrict__ solved, *__restrict__ x_ref, *__restrict__ Fres;            // [n,6]; x_ref or null (zero)
    const int *__restrict__ iterations, *__restrict__ flags;                               // [n]
    double *__restrict__ placed;                                                           // [n,6] device
    double *__restrict__ hPose, *__restrict__ hFres;                                       // [n,6] page-locked
    int *__restrict__ hIter, *__restrict__ hFlags;                                         // [n] page-locked
};
__global__ void __launch_bounds__(64) k_pose_place(PosePlaceArgs A) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= A.n) return;
    const int fl = A.flags[d];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const double xs = A.solved[(size_t)d * 6 + i];
        A.placed[(size_t)d * 6 + i] = fl ? (A.x_ref ? A.x_ref[(size_t)d * 6 + i] : 0.0) : xs;
        A.hPose[(size_t)d * 6 + i] = xs;
        A.hFres[(size_t)d * 6 + i] = A.Fres[(size_t)d * 6 + i];
    }
    A.hIter[d] = A.iterations[d];
    A.hFlags[d] = fl;
}

static inline int mean_pose_group(int nLine) {
    int G = 1;
    while (G < nLine && G < MP_THREADS) G *= 2;
    return G;
}
