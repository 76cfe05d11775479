// raftx_mooring.h -- quasi-static mooring lines of every design at its pose (included by raftx_hip.hip; entry points in
// include/raftx_mooring.h).
//
// Per line (one elastic catenary segment, fixed anchor -> point on the vessel; Jonkman 2007 eqs. 2-35 .. 2-38), with
// vF = VF/HF, vA = (VF - wL)/HF, s. = sqrt(1 + v.^2):
//   no contact   XF = HF/w (asinh vF - asinh vA) + HF L/EA         ZF = HF/w (sF - sA) + (VF L - w L^2/2)/EA
//   contact      XF = L_B + HF/w asinh vF + HF L/EA                ZF = HF/w (sF - 1) + VF^2/(2 EA w)     L_B = L - VF/w, CB = 0
// solved for (HF, VF) by a damped Newton iteration with the analytic Jacobian (symmetric: dXF/dVF = dZF/dHF); the branch is
// chosen anew at every evaluation (contact: VF < wL with the anchor on the seabed).  The differences sF - 1, sF - sA and
// 1/sF - 1/sA are written as quotients that do not cancel.
//
// A composite line (include/raftx_mooring.h: a head row and up to RAFTX_MOOR_MAX_SEG - 1 continuation rows, segments joined
// at free points that may carry a weight or a buoy) has the same two unknowns: on a frictionless seabed HF is common to
// every segment, and the vertical force at the top of segment i is VF minus the weight hanging above it, so X = sum X_i,
// Z = sum Z_i and the Jacobian is the sum of the segments' (moor_chain_eval).  The lane of the head row solves the chain and
// writes the records of all its rows; the lanes of continuation rows do nothing.  The chain code exists only in the
// CHAINS instantiations, which the host picks when a batch holds a continuation row: single-row batches run the code and
// give the bits they always did.
//
// Work decomposition: k_moor_line, one lane per (design, line), solves the line and leaves a record of MOOR_LW_N doubles
// (force, arm, 3 x 3 stiffness at the fairlead, the gradients of both end tensions); k_moor_design, one lane per design,
// adds the lines' shares of C_moor / F_moor in line order and writes T and J.  No atomics, no LDS: a design's bits
// depend on its own lines and pose only -- not on the batch or the grid.
#pragma once

#define MOOR_THREADS 256
#define MOOR_MAX_IT 60
#define MOOR_TIGHT 1e-10          // max(|dX|, |dZ|) / L below which a step that does not improve ends the iteration
#define MOOR_LW_N 24              // f 0:3 | r 3:6 | K 6:15 | gA 15:18 | gB 18:21 | TA 21 | TB 22 | flag 23
#define MOOR_LO_N 8               // HF, VF, HA, VA, L_B, iterations, branch, 0

struct MoorArgs {
    int nDesign, nLine;
    const double *__restrict__ lines;   // [nDesign,nLine,RAFTX_ML_N]
    const double *__restrict__ pose;    // [nDesign,6] or null (zero)
    double depth;
    double *__restrict__ lw;            // [nDesign,nLine,MOOR_LW_N]
    double *__restrict__ line_out;      // [nDesign,nLine,MOOR_LO_N] or null
    double *__restrict__ C, *__restrict__ F, *__restrict__ T, *__restrict__ J;      // [nDesign,36] [.,6] [.,2 nLine] [.,2 nLine,6], each or null
    int *__restrict__ flags;            // [nDesign]
    int chains;                         // host side only: a continuation row among the records, so the CHAINS kernels run
    double *__restrict__ Lr;            // [nDesign,2 nLine,3,6] or null: J as rows of k_sweep_channels (plane 0 = J, the other two zero)
};

struct MoorEval {
    double X, Z, a11, a12, a22;
    int contact;
};
__device__ __forceinline__ void moor_eval(const double H, const double V, const double L, const double EA, const double w,
                                          const bool seabed, MoorEval &e) {
    const double W = w * L;
    const double vF = V / H, sF = sqrt(1.0 + vF * vF), aF = asinh(vF);
    if (seabed && V < W) {
        e.contact = 1;
        e.X = (L - V / w) + (H / w) * aF + H * L / EA;
        e.Z = (H / w) * (vF * vF / (sF + 1.0)) + V * V / (2.0 * EA * w);
        e.a11 = (aF - vF / sF) / w + L / EA;
        e.a12 = -(vF * vF / (sF * (sF + 1.0))) / w;
        e.a22 = vF / sF / w + V / (EA * w);
    } else {
        e.contact = 0;
        const double vA = (V - W) / H, sA = sqrt(1.0 + vA * vA), aA = asinh(vA);
        const double q = (W / H) * (vF + vA) / (sF + sA);          // sF - sA
        e.X = (H / w) * (aF - aA) + H * L / EA;
        e.Z = (H / w) * q + (V * L - 0.5 * W * L) / EA;
        e.a11 = ((aF - aA) - (vF / sF - vA / sA)) / w + L / EA;
        e.a12 = -(q / (sF * sA)) / w;
        e.a22 = (vF / sF - vA / sA) / w + L / EA;
    }
}

// The arm R r_f of the fairlead rec[3:6] with the rotation of geom_pose: the fairlead as end A of a unit vertical member, the
// unit turned but not displaced; the displacement is added afterwards
__device__ __forceinline__ void moor_arm(const double rec[RAFTX_ML_N], const double ps[6], double (&r)[3]) {
    double gm[RAFTX_GM_N];
    for (int i = 0; i < RAFTX_GM_N; i++) gm[i] = 0.0;
    gm[RAFTX_GM_RA] = rec[3]; gm[RAFTX_GM_RA + 1] = rec[4]; gm[RAFTX_GM_RA + 2] = rec[5];
    gm[RAFTX_GM_RB] = rec[3]; gm[RAFTX_GM_RB + 1] = rec[4]; gm[RAFTX_GM_RB + 2] = rec[5] + 1.0;
    gm[RAFTX_GM_L] = 1.0;
    const double pr[6] = {0.0, 0.0, 0.0, ps[3], ps[4], ps[5]};
    double rA0[3], q[3], p1[3], p2[3], rB[3], R2[2][2];
    geom_pose(gm, pr, rA0, q, p1, p2, r, rB, R2);
}

// ---- composite lines.  The segments of a chain, anchor side first; Wj is the net weight of the point at a segment's lower
// end (0 for the anchor-side one).  Every loop over them is unrolled to RAFTX_MOOR_MAX_SEG so that they stay in registers.
struct MoorChain {
    int n;
    double L[RAFTX_MOOR_MAX_SEG], EA[RAFTX_MOOR_MAX_SEG], w[RAFTX_MOOR_MAX_SEG], Wj[RAFTX_MOOR_MAX_SEG];
};
// X, Z and the Jacobian of the whole chain at the fairlead's (H, V): the sums of the segments', marching from the fairlead
// down with V at the top of a segment = V less the segments and joints hanging above it.  Only the anchor-side segment may rest
// on the seabed (moor_eval's contact branch with its own V); where all of it rests (V at its top <= 0) it is a straight
// stretched length on the bed, which the contact branch approaches with a continuous Jacobian.  Vtop [n]: each segment's V.
__device__ __forceinline__ void moor_chain_eval(const double H, const double V, const MoorChain &c, const bool seabed, MoorEval &e,
                                                double Vtop[RAFTX_MOOR_MAX_SEG]) {
    e.X = 0.0; e.Z = 0.0; e.a11 = 0.0; e.a12 = 0.0; e.a22 = 0.0; e.contact = 0;
    double Vt = V;
#pragma unroll
    for (int i = RAFTX_MOOR_MAX_SEG - 1; i >= 0; i--) {
        if (i >= c.n) continue;
        Vtop[i] = Vt;
        if (i == 0 && seabed && Vt <= 0.0) {
            e.X += c.L[0] + H * c.L[0] / c.EA[0];
            e.a11 += c.L[0] / c.EA[0];
            e.contact = 1;
        } else {
            MoorEval s;
            moor_eval(H, Vt, c.L[i], c.EA[i], c.w[i], seabed && i == 0, s);
            e.X += s.X; e.Z += s.Z; e.a11 += s.a11; e.a12 += s.a12; e.a22 += s.a22;
            if (i == 0) e.contact = s.contact;
        }
        Vt = (Vt - c.w[i] * c.L[i]) - c.Wj[i];
    }
}

// A chain at the pose ps: the head row `line` and the nc continuation rows after it.  The records lw of all its rows and, where
// lo_out is not null and the chain is not flagged, their line_out rows.  NOT inlined, and every argument a scalar or a pointer
// to global memory: k_moor_line and k_mean_pose call one body, so the records of a chain are the same bits from both (for a
// single line the two kernels' inlined copies of one source have always agreed; nothing promises that of a second, larger body).
struct MoorPose { double v[6]; };
__device__ __noinline__ void moor_chain_record(const double *__restrict__ line, const int nc, const MoorPose pose, const double depth,
                                               double *__restrict__ lw, double *__restrict__ lo_out) {
    double rec[RAFTX_ML_N], ps[6];
#pragma unroll
    for (int i = 0; i < RAFTX_ML_N; i++) rec[i] = line[i];
#pragma unroll
    for (int i = 0; i < 6; i++) ps[i] = pose.v[i];
    MoorChain c;
    c.n = nc + 1;
    c.L[0] = rec[6]; c.EA[0] = rec[7]; c.w[0] = rec[8]; c.Wj[0] = 0.0;
    bool fin = true;
    for (int i = 0; i < 10; i++) fin = fin && isfinite(rec[i]);
    for (int i = 0; i < 6; i++) fin = fin && isfinite(ps[i]);
    bool pos = c.L[0] > 0.0 && c.EA[0] > 0.0 && c.w[0] > 0.0;
    double Lt = c.L[0], Wt = c.w[0] * c.L[0];
#pragma unroll
    for (int i = 1; i < RAFTX_MOOR_MAX_SEG; i++) {
        c.L[i] = 1.0; c.EA[i] = 1.0; c.w[i] = 1.0; c.Wj[i] = 0.0;
        if (i >= c.n) continue;
        const double *p = line + (size_t)i * RAFTX_ML_N;
        c.L[i] = p[6]; c.EA[i] = p[7]; c.w[i] = p[8]; c.Wj[i] = p[RAFTX_ML_WJOINT];
        fin = fin && isfinite(c.L[i]) && isfinite(c.EA[i]) && isfinite(c.w[i]) && isfinite(p[9]) && isfinite(c.Wj[i]);
        pos = pos && c.L[i] > 0.0 && c.EA[i] > 0.0 && c.w[i] > 0.0;
        Lt += c.L[i];
        Wt += c.w[i] * c.L[i] + c.Wj[i];
    }
    const double az = rec[2];
    int flag = 0;
    double r[3] = {0, 0, 0}, XF = 0.0, ZF = 0.0, ux = 0.0, uy = 0.0;
    if (!fin || !pos || !(Wt > 0.0) || az < -depth - 1e-6 * depth) flag = RAFTX_MOOR_BAD_LINE;
    if (!flag) {
        moor_arm(rec, ps, r);
        const double dx = (ps[0] + r[0]) - rec[0], dy = (ps[1] + r[1]) - rec[1];
        XF = sqrt(dx * dx + dy * dy);
        ZF = (ps[2] + r[2]) - az;
        ux = dx / XF;
        uy = dy / XF;
        if (!(ZF > 0.0)) flag = RAFTX_MOOR_BAD_LINE;
        else if (XF <= 1e-9 * Lt) flag = RAFTX_MOOR_VERTICAL;
        else if (Lt >= XF + ZF) flag = RAFTX_MOOR_SLACK;
    }
    double H = 0.0, V = 0.0, Vtop[RAFTX_MOOR_MAX_SEG] = {0, 0, 0, 0};
    MoorEval e;
    int it = 0;
    if (!flag) {
        const bool seabed = fabs(az + depth) <= 1e-6 * depth;
        const double we = Wt / Lt;                                // the effective weight per length of the guess
        const double lam = (Lt * Lt <= XF * XF + ZF * ZF) ? 0.2 : sqrt(3.0 * ((Lt * Lt - ZF * ZF) / (XF * XF) - 1.0));
        H = fabs(we * XF / (2.0 * lam));
        V = 0.5 * we * (ZF / tanh(lam) + Lt);
        moor_chain_eval(H, V, c, seabed, e, Vtop);
        double eX = e.X - XF, eZ = e.Z - ZF, res = fmax(fabs(eX), fabs(eZ)) / Lt, a = 1.0;
        bool conv = res == 0.0;
        while (!conv && it < MOOR_MAX_IT) {
            it++;
            const double det = e.a11 * e.a22 - e.a12 * e.a12;
            const double dH = -(e.a22 * eX - e.a12 * eZ) / det, dV = -(e.a11 * eZ - e.a12 * eX) / det;
            double s = a;
            if (H + s * dH <= 0.0) s = -0.5 * H / dH;
            const double Ht = H + s * dH, Vt = V + s * dV;
            MoorEval n;
            double Vn[RAFTX_MOOR_MAX_SEG] = {0, 0, 0, 0};
            moor_chain_eval(Ht, Vt, c, seabed, n, Vn);
            const double nX = n.X - XF, nZ = n.Z - ZF, rn = fmax(fabs(nX), fabs(nZ)) / Lt;
            if (rn < res) {
                H = Ht; V = Vt; e = n; eX = nX; eZ = nZ; res = rn; a = 1.0;
#pragma unroll
                for (int i = 0; i < RAFTX_MOOR_MAX_SEG; i++) Vtop[i] = Vn[i];
                conv = res == 0.0;
            } else if (res <= MOOR_TIGHT) {
                conv = true;
            } else {
                a *= 0.5;
                if (a < 0x1p-40) break;
            }
        }
        if (!conv) flag = RAFTX_MOOR_NO_CONVERGENCE;
        else if (seabed && Vtop[0] <= 0.0) flag = RAFTX_MOOR_GROUNDED;      // the anchor-side segment rests wholly: so would its upper joint
        else {
            // the joints and the sags (where V changes sign inside a segment) against the seabed, from the anchor up
            const double floor = -depth - 1e-6 * depth;
            double z = az;
#pragma unroll
            for (int i = 0; i < RAFTX_MOOR_MAX_SEG; i++) {
                if (i >= c.n) continue;
                const double Vb = Vtop[i] - c.w[i] * c.L[i];
                if (!(i == 0 && e.contact) && Vb < 0.0 && Vtop[i] > 0.0) {
                    const double vb = Vb / H, sb = sqrt(1.0 + vb * vb);
                    const double drop = (H / c.w[i]) * (vb * vb / (sb + 1.0)) + Vb * Vb / (2.0 * c.EA[i] * c.w[i]);
                    if (z - drop < floor) flag = RAFTX_MOOR_GROUNDED;
                }
                MoorEval s;
                moor_eval(H, Vtop[i], c.L[i], c.EA[i], c.w[i], seabed && i == 0, s);
                z += s.Z;
                if (i + 1 < c.n && z < floor) flag = RAFTX_MOOR_GROUNDED;
            }
        }
    }
    if (!flag) {
        const double det = e.a11 * e.a22 - e.a12 * e.a12;
        const double k11 = e.a22 / det, k12 = -e.a12 / det, k22 = e.a11 / det;
        const double th = H / XF;
#pragma unroll
        for (int i = 0; i < RAFTX_MOOR_MAX_SEG; i++) {
            if (i >= c.n) continue;
            double *q = lw + (size_t)i * MOOR_LW_N;
            const bool ct = i == 0 && e.contact;
            const double VB = Vtop[i], VA = ct ? 0.0 : VB - c.w[i] * c.L[i];
            const double TB = sqrt(H * H + VB * VB), TA = sqrt(H * H + VA * VA);
            if (i == 0) {
                q[0] = -H * ux; q[1] = -H * uy; q[2] = -V;
                q[6] = k11 * ux * ux + th * (1.0 - ux * ux);
                q[7] = k11 * ux * uy - th * (ux * uy);
                q[8] = k12 * ux;
                q[9] = q[7];
                q[10] = k11 * uy * uy + th * (1.0 - uy * uy);
                q[11] = k12 * uy;
                q[12] = q[8];
                q[13] = q[11];
                q[14] = k22;
            } else {
                q[0] = 0.0; q[1] = 0.0; q[2] = 0.0;
                for (int k = 6; k < 15; k++) q[k] = 0.0;
            }
            q[3] = r[0]; q[4] = r[1]; q[5] = r[2];
            const double gAX = (H * k11 + VA * k12) / TA, gAZ = (H * k12 + VA * k22) / TA;
            const double gBX = (H * k11 + VB * k12) / TB, gBZ = (H * k12 + VB * k22) / TB;
            q[15] = gAX * ux; q[16] = gAX * uy; q[17] = gAZ;
            q[18] = gBX * ux; q[19] = gBX * uy; q[20] = gBZ;
            q[21] = TA;
            q[22] = TB;
            double *o = lo_out ? lo_out + (size_t)i * MOOR_LO_N : nullptr;
            if (o) {
                o[0] = H; o[1] = VB; o[2] = H; o[3] = VA;
                o[4] = ct ? c.L[0] - VB / c.w[0] : 0.0;
                o[5] = (double)it;
                o[6] = ct ? 1.0 : 0.0;
                o[7] = 0.0;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < RAFTX_MOOR_MAX_SEG; i++)
        if (i < c.n) lw[(size_t)i * MOOR_LW_N + 23] = (double)flag;
}

// One line at the pose ps: the record lw [MOOR_LW_N] (in global memory) and lo [MOOR_LO_N].  The body of k_moor_line, shared
// with k_mean_pose (raftx_statics.h).  Returns true: lo is this row's line_out.  CHAINS: `line` may be the head row of a
// composite line, with its continuation rows among the nAfter rows of the design that follow it -- then the records of all of
// them are written, and their line_out rows at lo_out (this row's place in global memory, or null) unless the chain is flagged
// -- or a continuation row itself, for which nothing is written; false is returned in both cases.
template <bool CHAINS>
__device__ __forceinline__ bool moor_line_record(const double *__restrict__ line, const int nAfter, const double ps[6],
                                                 const double depth, double *__restrict__ lw, double lo[MOOR_LO_N],
                                                 double *__restrict__ lo_out) {
    double rec[RAFTX_ML_N];
    {
        const double2 *p = reinterpret_cast<const double2 *>(line);
#pragma unroll
        for (int k = 0; k < RAFTX_ML_N / 2; k++) {
            const double2 v = p[k];
            rec[2 * k] = v.x;
            rec[2 * k + 1] = v.y;
        }
    }
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int i = 0; i < MOOR_LO_N; i++) lo[i] = nan;
    if (CHAINS) {
        if (rec[RAFTX_ML_CONT] != 0.0) return false;
        int nc = 0;
        while (nc < nAfter && nc < RAFTX_MOOR_MAX_SEG - 1 && line[(size_t)(nc + 1) * RAFTX_ML_N + RAFTX_ML_CONT] != 0.0) nc++;
        if (nc) {
            MoorPose pose;
#pragma unroll
            for (int i = 0; i < 6; i++) pose.v[i] = ps[i];
            moor_chain_record(line, nc, pose, depth, lw, lo_out);
            return false;
        }
    }
    int flag = 0;
    bool fin = true;
    for (int i = 0; i < 10; i++) fin = fin && isfinite(rec[i]);
    for (int i = 0; i < 6; i++) fin = fin && isfinite(ps[i]);
    const double L = rec[6], EA = rec[7], w = rec[8], az = rec[2];
    double r[3] = {0, 0, 0}, XF = 0.0, ZF = 0.0, ux = 0.0, uy = 0.0;
    if (!fin || !(L > 0.0) || !(EA > 0.0) || !(w > 0.0) || az < -depth - 1e-6 * depth) flag = RAFTX_MOOR_BAD_LINE;
    if (!flag) {
        moor_arm(rec, ps, r);
        const double dx = (ps[0] + r[0]) - rec[0], dy = (ps[1] + r[1]) - rec[1];
        XF = sqrt(dx * dx + dy * dy);
        ZF = (ps[2] + r[2]) - az;
        ux = dx / XF;
        uy = dy / XF;
        if (!(ZF > 0.0)) flag = RAFTX_MOOR_BAD_LINE;
        else if (XF <= 1e-9 * L) flag = RAFTX_MOOR_VERTICAL;
        else if (L >= XF + ZF) flag = RAFTX_MOOR_SLACK;
    }
    if (!flag) {
        const bool seabed = fabs(az + depth) <= 1e-6 * depth;
        const double lam = (L * L <= XF * XF + ZF * ZF) ? 0.2 : sqrt(3.0 * ((L * L - ZF * ZF) / (XF * XF) - 1.0));
        double H = fabs(w * XF / (2.0 * lam)), V = 0.5 * w * (ZF / tanh(lam) + L);
        MoorEval e;
        moor_eval(H, V, L, EA, w, seabed, e);
        double eX = e.X - XF, eZ = e.Z - ZF, res = fmax(fabs(eX), fabs(eZ)) / L, a = 1.0;
        int it = 0;
        bool conv = res == 0.0;
        while (!conv && it < MOOR_MAX_IT) {
            it++;
            const double det = e.a11 * e.a22 - e.a12 * e.a12;
            const double dH = -(e.a22 * eX - e.a12 * eZ) / det, dV = -(e.a11 * eZ - e.a12 * eX) / det;
            double s = a;
            if (H + s * dH <= 0.0) s = -0.5 * H / dH;             // keep HF > 0: at most half way to zero
            const double Ht = H + s * dH, Vt = V + s * dV;
            MoorEval n;
            moor_eval(Ht, Vt, L, EA, w, seabed, n);
            const double nX = n.X - XF, nZ = n.Z - ZF, rn = fmax(fabs(nX), fabs(nZ)) / L;
            if (rn < res) {
                H = Ht; V = Vt; e = n; eX = nX; eZ = nZ; res = rn; a = 1.0;
                conv = res == 0.0;
            } else if (res <= MOOR_TIGHT) {
                conv = true;                                     // stagnation: the step no longer improves the residual
            } else {
                a *= 0.5;                                        // (a NaN residual lands here too)
                if (a < 0x1p-40) break;
            }
        }
        if (!conv) flag = RAFTX_MOOR_NO_CONVERGENCE;
        else {
            const double det = e.a11 * e.a22 - e.a12 * e.a12;
            const double k11 = e.a22 / det, k12 = -e.a12 / det, k22 = e.a11 / det;
            const double VA = e.contact ? 0.0 : V - w * L;
            const double TB = sqrt(H * H + V * V), TA = sqrt(H * H + VA * VA);
            const double th = H / XF;
            lw[0] = -H * ux; lw[1] = -H * uy; lw[2] = -V;
            lw[3] = r[0]; lw[4] = r[1]; lw[5] = r[2];
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
            lo[0] = H; lo[1] = V; lo[2] = H; lo[3] = VA;
            lo[4] = e.contact ? L - V / w : 0.0;
            lo[5] = (double)it;
            lo[6] = (double)e.contact;
            lo[7] = 0.0;
        }
    }
    lw[23] = (double)flag;
    return true;
}

template <bool CHAINS>
__global__ void __launch_bounds__(MOOR_THREADS) k_moor_line(MoorArgs A) {
    const long long t = (long long)blockIdx.x * MOOR_THREADS + threadIdx.x;
    if (t >= (long long)A.nDesign * A.nLine) return;
    const int d = (int)(t / A.nLine);
    double ps[6] = {0, 0, 0, 0, 0, 0};
    if (A.pose)
        for (int i = 0; i < 6; i++) ps[i] = A.pose[(size_t)d * 6 + i];
    double lo[MOOR_LO_N];
    const bool mine = moor_line_record<CHAINS>(A.lines + (size_t)t * RAFTX_ML_N, A.nLine - 1 - (int)(t % A.nLine), ps, A.depth,
                                               A.lw + (size_t)t * MOOR_LW_N, lo,
                                               A.line_out ? A.line_out + (size_t)t * MOOR_LO_N : nullptr);
    if (A.line_out && mine)
        for (int i = 0; i < MOOR_LO_N; i++) A.line_out[(size_t)t * MOOR_LO_N + i] = lo[i];
}

// The share of one line record q in C_moor [36] and F_moor [6], and its rows of T and J: the sums of k_moor_design, shared with
// k_mean_pose (raftx_statics.h).
__device__ __forceinline__ void moor_line_share(const double *__restrict__ q, double C[36], double F[6]) {
    const double f[3] = {q[0], q[1], q[2]}, r[3] = {q[3], q[4], q[5]};
    double K[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) K[i][j] = q[6 + 3 * i + j];
    // [r x] and [f x]
    const double RX[3][3] = {{0.0, -r[2], r[1]}, {r[2], 0.0, -r[0]}, {-r[1], r[0], 0.0}};
    const double FX[3][3] = {{0.0, -f[2], f[1]}, {f[2], 0.0, -f[0]}, {-f[1], f[0], 0.0}};
    double KR[3][3], RK[3][3];                                // K [r x], [r x] K
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            KR[i][j] = K[i][0] * RX[0][j] + K[i][1] * RX[1][j] + K[i][2] * RX[2][j];
            RK[i][j] = RX[i][0] * K[0][j] + RX[i][1] * K[1][j] + RX[i][2] * K[2][j];
        }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double rkr = RX[i][0] * KR[0][j] + RX[i][1] * KR[1][j] + RX[i][2] * KR[2][j];
            const double fr = FX[i][0] * RX[0][j] + FX[i][1] * RX[1][j] + FX[i][2] * RX[2][j];     // the arm turning under a fixed force
            C[6 * i + j] += K[i][j];
            C[6 * i + 3 + j] += -KR[i][j];
            C[6 * (3 + i) + j] += RK[i][j];
            C[6 * (3 + i) + 3 + j] += -rkr - fr;
        }
    F[0] += f[0]; F[1] += f[1]; F[2] += f[2];
    F[3] += r[1] * f[2] - r[2] * f[1];
    F[4] += r[2] * f[0] - r[0] * f[2];
    F[5] += r[0] * f[1] - r[1] * f[0];
}
__device__ __forceinline__ void moor_line_TJ(const double *__restrict__ q, const int l, const int nL, double *__restrict__ T,
                                             double *__restrict__ J) {
    const double r[3] = {q[3], q[4], q[5]};
    if (T) { T[l] = q[21]; T[nL + l] = q[22]; }
    if (J)
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const double *g = q + 15 + 3 * e;
            double *o = J + (size_t)(e * nL + l) * 6;
            o[0] = g[0]; o[1] = g[1]; o[2] = g[2];
            o[3] = r[1] * g[2] - r[2] * g[1];
            o[4] = r[2] * g[0] - r[0] * g[2];
            o[5] = r[0] * g[1] - r[1] * g[0];
        }
}

__global__ void __launch_bounds__(MOOR_THREADS) k_moor_design(MoorArgs A) {
    const int d = blockIdx.x * MOOR_THREADS + threadIdx.x;
    if (d >= A.nDesign) return;
    const int nL = A.nLine;
    const double *lw0 = A.lw + (size_t)d * nL * MOOR_LW_N;
    int flag = 0;
    for (int l = 0; l < nL; l++) flag |= (int)lw0[(size_t)l * MOOR_LW_N + 23];
    A.flags[d] = flag;
    double *T = A.T ? A.T + (size_t)d * 2 * nL : nullptr, *J = A.J ? A.J + (size_t)d * 2 * nL * 6 : nullptr;
    if (flag) {                                                  // a flagged design: NaN, in its own rows only
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        if (A.C) for (int i = 0; i < 36; i++) A.C[(size_t)d * 36 + i] = nan;
        if (A.F) for (int i = 0; i < 6; i++) A.F[(size_t)d * 6 + i] = nan;
        if (T) for (int i = 0; i < 2 * nL; i++) T[i] = nan;
        if (J) for (int i = 0; i < 12 * nL; i++) J[i] = nan;
        if (A.line_out) for (int i = 0; i < nL * MOOR_LO_N; i++) A.line_out[(size_t)d * nL * MOOR_LO_N + i] = nan;
        if (A.Lr) for (int i = 0; i < 36 * nL; i++) A.Lr[(size_t)d * 36 * nL + i] = (i % 18) < 6 ? nan : 0.0;
        return;
    }
    double C[36], F[6];
#pragma unroll
    for (int i = 0; i < 36; i++) C[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) F[i] = 0.0;
    for (int l = 0; l < nL; l++) {
        const double *q = lw0 + (size_t)l * MOOR_LW_N;
        moor_line_share(q, C, F);
        const double r[3] = {q[3], q[4], q[5]};
        moor_line_TJ(q, l, nL, T, J);
        if (A.Lr)
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const double *g = q + 15 + 3 * e;
                double *o = A.Lr + ((size_t)d * 2 * nL + (e * nL + l)) * 18;
                o[0] = g[0]; o[1] = g[1]; o[2] = g[2];
                o[3] = r[1] * g[2] - r[2] * g[1];
                o[4] = r[2] * g[0] - r[0] * g[2];
                o[5] = r[0] * g[1] - r[1] * g[0];
#pragma unroll
                for (int i = 6; i < 18; i++) o[i] = 0.0;
            }
    }
    if (A.C)
#pragma unroll
        for (int i = 0; i < 36; i++) A.C[(size_t)d * 36 + i] = C[i];
    if (A.F)
#pragma unroll
        for (int i = 0; i < 6; i++) A.F[(size_t)d * 6 + i] = F[i];
}

// The line records of the variants of a mooring program (raftx_mooring_program): the base records with the anchor /
// fairlead coordinates of the edited lines evaluated as affine_eval does for the member ends -- left to right, no fused
// multiply-adds.  One lane per (design, line).
struct MoorExpandArgs {
    int nDesign, nLine, nP;
    const double *__restrict__ base;    // [nLine,RAFTX_ML_N]
    const double *__restrict__ coef;    // [nLine,6,nP+1]
    const int *__restrict__ edit;       // [nLine]
    const double *__restrict__ params;  // [nDesign,nP]
    double *__restrict__ out;           // [nDesign,nLine,RAFTX_ML_N]
};
__global__ void __launch_bounds__(MOOR_THREADS) k_moor_expand(MoorExpandArgs E) {
    const long long t = (long long)blockIdx.x * MOOR_THREADS + threadIdx.x;
    if (t >= (long long)E.nDesign * E.nLine) return;
    const int d = (int)(t / E.nLine), l = (int)(t % E.nLine);
    const double *b = E.base + (size_t)l * RAFTX_ML_N;
    double *o = E.out + (size_t)t * RAFTX_ML_N;
    const bool ed = E.edit[l] != 0;
    for (int i = 0; i < RAFTX_ML_N; i++)
        o[i] = (ed && i < 6) ? affine_eval(E.coef + ((size_t)l * 6 + i) * (E.nP + 1), E.params + (size_t)d * E.nP, E.nP) : b[i];
}

// C0 [n,36] += C_moor [n,36] of a block of a crossing (raftx_sweep_mooring with add_stiffness), ahead of the add-up
__global__ void __launch_bounds__(MOOR_THREADS) k_moor_add(double *__restrict__ C0, const double *__restrict__ Cm, long long n) {
    const long long t = (long long)blockIdx.x * MOOR_THREADS + threadIdx.x;
    if (t < n) C0[t] += Cm[t];
}

static inline unsigned moor_grid(long long n) { return (unsigned)((n + MOOR_THREADS - 1) / MOOR_THREADS); }
