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
// A bridle (stem rows, then leg rows with field 14 set) has the junction's three coordinates as unknowns and fairleads that are
// coupled through it: moor_bridle_record below, a record array of its own (MOOR_BW_N per row), and third instantiations
// (BRIDLES) that the host picks when a batch holds a leg row.
//
// Work decomposition: k_moor_line, one lane per (design, line), solves the line and leaves a record of MOOR_LW_N doubles
// (force, arm, 3 x 3 stiffness at the fairlead, the gradients of both end tensions); k_moor_design, one lane per design,
// adds the lines' shares of C_moor / F_moor in line order and writes T and J.  No atomics, no LDS: a design's bits
// depend on its own lines and pose only -- not on the batch or the grid.
//
// Shared steps: moor_chain_load / moor_chain_grounded (a chain, a bridle's stem), moor_end_set / moor_end_grad / moor_lo_write (a
// chain, a stem, a leg), moor_design_walk (k_moor_design, k_mean_pose).  NOT shared, on purpose: the Newton loops of the single row
// and of the chain stay beside moor_shoot, and the single row keeps its own record writer -- through the helpers the compiler fuses
// the other product of K3's k11 u u + th (1 - u u) and C_moor moves in the last bit (profiles/mooring_one_solve_ab.txt) --, and the
// shared rows of an array (raftx_array_mooring.h) keep their copy under a lexical `fp contract(off)` that a helper here would escape.
#pragma once

#define MOOR_THREADS 256
#define MOOR_MAX_IT 60
#define MOOR_TIGHT 1e-10          // max(|dX|, |dZ|) / L below which a step that does not improve ends the iteration
#define MOOR_LW_N 24              // f 0:3 | r 3:6 | K 6:15 | gA 15:18 | gB 18:21 | TA 21 | TB 22 | flag 23
#define MOOR_LO_N 8               // HF, VF, HA, VA, L_B, iterations, branch, 0
#define MOOR_BW_N 56              // a bridle's row: C share 0:36 | F 36:42 (head row only) | TA 42 | TB 43 | JA 44:50 | JB 50:56
#define MOOR_BR_MAX_IT 60         // steps of the junction iteration, at most
#define MOOR_BR_GROW 1e3          // ... and the growth of its residual that ONE step may bring, when the step before brought none

struct MoorArgs {
    int nDesign, nLine;
    const double *__restrict__ lines;   // [nDesign,nLine,RAFTX_ML_N]
    const double *__restrict__ pose;    // [nDesign,6] or null (zero)
    double depth;
    double *__restrict__ lw;            // [nDesign,nLine,MOOR_LW_N]
    double *__restrict__ line_out;      // [nDesign,nLine,MOOR_LO_N] or null
    double *__restrict__ C, *__restrict__ F, *__restrict__ T, *__restrict__ J;      // [nDesign,36] [.,6] [.,2 nLine] [.,2 nLine,6], each or null
    int *__restrict__ flags;            // [nDesign]
    int chains;                         // host side only: 1 a continuation row among the records, so the CHAINS kernels run; 2 a leg row: BRIDLES
    double *__restrict__ Lr;            // [nDesign,2 nLine,3,6] or null: J as rows of k_sweep_channels (plane 0 = J, the other two zero)
    double *__restrict__ bw;            // [nDesign,nLine,MOOR_BW_N], only with bridles
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

// ---- one element between its ends, XF apart horizontally and ZF vertically: the Newton iteration of moor_line_record /
// moor_chain_record, cold start.  KIND 0: the chain c; 1: one suspended segment (c.L[0], c.EA[0], c.w[0]; no seabed); 2: the
// chain c with the suspended segment top = (L, EA, w, weight of the point at its lower end) above it -- (H, V) at the top of
// that segment, Vtop the chain's own.
template <int KIND>
__device__ __forceinline__ void moor_shoot_eval(const double H, const double V, const MoorChain &c, const bool seabed, const double top[4],
                                                MoorEval &e, double Vtop[RAFTX_MOOR_MAX_SEG]) {
    if (KIND == 1) moor_eval(H, V, c.L[0], c.EA[0], c.w[0], false, e);
    else if (KIND == 0) moor_chain_eval(H, V, c, seabed, e, Vtop);
    else {
        MoorEval t;
        moor_eval(H, V, top[0], top[1], top[2], false, t);
        moor_chain_eval(H, (V - top[2] * top[0]) - top[3], c, seabed, e, Vtop);
        e.X = t.X + e.X; e.Z = t.Z + e.Z; e.a11 = t.a11 + e.a11; e.a12 = t.a12 + e.a12; e.a22 = t.a22 + e.a22;
    }
}
template <int KIND>
__device__ __forceinline__ bool moor_shoot(const MoorChain &c, const bool seabed, const double top[4], const double Lt, const double we,
                                           const double XF, const double ZF, double &H, double &V, MoorEval &e,
                                           double Vtop[RAFTX_MOOR_MAX_SEG]) {
    const double lam = (Lt * Lt <= XF * XF + ZF * ZF) ? 0.2 : sqrt(3.0 * ((Lt * Lt - ZF * ZF) / (XF * XF) - 1.0));
    H = fabs(we * XF / (2.0 * lam));
    V = 0.5 * we * (ZF / tanh(lam) + Lt);
    moor_shoot_eval<KIND>(H, V, c, seabed, top, e, Vtop);
    double eX = e.X - XF, eZ = e.Z - ZF, res = fmax(fabs(eX), fabs(eZ)) / Lt, a = 1.0;
    bool conv = res == 0.0;
    int it = 0;
    while (!conv && it < MOOR_MAX_IT) {
        it++;
        const double det = e.a11 * e.a22 - e.a12 * e.a12;
        const double dH = -(e.a22 * eX - e.a12 * eZ) / det, dV = -(e.a11 * eZ - e.a12 * eX) / det;
        double s = a;
        if (H + s * dH <= 0.0) s = -0.5 * H / dH;
        const double Ht = H + s * dH, Vt = V + s * dV;
        MoorEval n;
        double Vn[RAFTX_MOOR_MAX_SEG] = {0, 0, 0, 0};
        moor_shoot_eval<KIND>(Ht, Vt, c, seabed, top, n, Vn);
        const double nX = n.X - XF, nZ = n.Z - ZF, rn = fmax(fabs(nX), fabs(nZ)) / Lt;
        if (rn < res) {
            H = Ht; V = Vt; e = n; eX = nX; eZ = nZ; res = rn; a = 1.0;
            if (KIND != 1)
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
    return conv;
}

// A solved element: its end force pieces, (k) the inverse of its catenary Jacobian and the 3 x 3 end stiffness
// K = [k11 u u' + HF/XF (I_h - u u'), k12 u; k12 u', k22] (xx xy xz yy yz zz): a chain, a bridle's stem and its legs.
struct MoorEnd {
    double H, V, ux, uy, k11, k12, k22, K[6];
};
__device__ __forceinline__ void moor_end_set(MoorEnd &m, const double H, const double V, const MoorEval &e, const double ux,
                                             const double uy, const double XF) {
    const double det = e.a11 * e.a22 - e.a12 * e.a12;
    m.H = H; m.V = V; m.ux = ux; m.uy = uy;
    m.k11 = e.a22 / det; m.k12 = -e.a12 / det; m.k22 = e.a11 / det;
    const double th = H / XF;
    m.K[0] = m.k11 * ux * ux + th * (1.0 - ux * ux);
    m.K[1] = m.k11 * ux * uy - th * (ux * uy);
    m.K[2] = m.k12 * ux;
    m.K[3] = m.k11 * uy * uy + th * (1.0 - uy * uy);
    m.K[4] = m.k12 * uy;
    m.K[5] = m.k22;
}
// The gradient g3 of the tension Tx = |(H, Vx)| at a point of the element where the vertical force is Vx, for a displacement
// of its upper end
__device__ __forceinline__ void moor_end_grad(const MoorEnd &m, const double Vx, const double Tx, double g3[3]) {
    const double gX = (m.H * m.k11 + Vx * m.k12) / Tx, gZ = (m.H * m.k12 + Vx * m.k22) / Tx;
    g3[0] = gX * m.ux; g3[1] = gX * m.uy; g3[2] = gZ;
}
// The record q [0:23] of one row of the solved element m, between VA at its lower and VB at its upper end, with the arm r.
// head: the row that carries the element's force and K3 (the anchor-side row of a chain); the others have zeros.
__device__ __forceinline__ void moor_row_write(double *__restrict__ q, const MoorEnd &m, const double r[3], const bool head, const double VA,
                                               const double VB) {
    const double TB = sqrt(m.H * m.H + VB * VB), TA = sqrt(m.H * m.H + VA * VA);
    if (head) {
        q[0] = -m.H * m.ux; q[1] = -m.H * m.uy; q[2] = -m.V;
        q[6] = m.K[0]; q[7] = m.K[1]; q[8] = m.K[2];
        q[9] = m.K[1]; q[10] = m.K[3]; q[11] = m.K[4];
        q[12] = m.K[2]; q[13] = m.K[4]; q[14] = m.K[5];
    } else {
        q[0] = 0.0; q[1] = 0.0; q[2] = 0.0;
        for (int k = 6; k < 15; k++) q[k] = 0.0;
    }
    q[3] = r[0]; q[4] = r[1]; q[5] = r[2];
    double gA[3], gB[3];
    moor_end_grad(m, VA, TA, gA);
    moor_end_grad(m, VB, TB, gB);
    q[15] = gA[0]; q[16] = gA[1]; q[17] = gA[2];
    q[18] = gB[0]; q[19] = gB[1]; q[20] = gB[2];
    q[21] = TA;
    q[22] = TB;
}
// A line_out row: LB the length on the seabed (ct: the row rests there in part), it the steps of the row's iteration
__device__ __forceinline__ void moor_lo_write(double *o, const double H, const double VB, const double VA, const double LB, const int it,
                                              const bool ct) {
    o[0] = H; o[1] = VB; o[2] = H; o[3] = VA; o[4] = LB;
    o[5] = (double)it; o[6] = ct ? 1.0 : 0.0; o[7] = 0.0;
}
// How far a segment (EA, w) sags below its lower end, where the vertical force is Vb < 0 (V changes sign inside the segment)
__device__ __forceinline__ double moor_sag_drop(const double H, const double Vb, const double EA, const double w) {
    const double vb = Vb / H, sb = sqrt(1.0 + vb * vb);
    return (H / w) * (vb * vb / (sb + 1.0)) + Vb * Vb / (2.0 * EA * w);
}
// The head row `line` (into rec) and its nc continuation rows as the chain c, with the pose (into ps).  fin: every number read is
// finite; pos: every L, EA, w is positive; Lt, Wt: the sums of the lengths and of the weights (segments and joints).
struct MoorPose { double v[6]; };
__device__ __forceinline__ void moor_chain_load(const double *__restrict__ line, const int nc, const MoorPose &pose, double rec[RAFTX_ML_N],
                                                double ps[6], MoorChain &c, bool &fin, bool &pos, double &Lt, double &Wt) {
#pragma unroll
    for (int i = 0; i < RAFTX_ML_N; i++) rec[i] = line[i];
#pragma unroll
    for (int i = 0; i < 6; i++) ps[i] = pose.v[i];
    c.n = nc + 1;
    c.L[0] = rec[6]; c.EA[0] = rec[7]; c.w[0] = rec[8]; c.Wj[0] = 0.0;
    fin = true;
    for (int i = 0; i < 10; i++) fin = fin && isfinite(rec[i]);
    for (int i = 0; i < 6; i++) fin = fin && isfinite(ps[i]);
    pos = c.L[0] > 0.0 && c.EA[0] > 0.0 && c.w[0] > 0.0;
    Lt = c.L[0];
    Wt = c.w[0] * c.L[0];
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
}
// The solved chain c (H, its segments' Vtop, the anchor-side segment's contact) against the seabed, anchor at az: true where the
// anchor-side segment rests wholly (so would its upper joint), or a joint or a sag lies below the floor
__device__ __forceinline__ bool moor_chain_grounded(const MoorChain &c, const double H, const double Vtop[RAFTX_MOOR_MAX_SEG], const int contact,
                                                    const bool seabed, const double az, const double depth) {
    if (seabed && Vtop[0] <= 0.0) return true;
    // the joints and the sags (where V changes sign inside a segment) against the seabed, from the anchor up
    const double floor = -depth - 1e-6 * depth;
    bool grounded = false;
    double z = az;
#pragma unroll
    for (int i = 0; i < RAFTX_MOOR_MAX_SEG; i++) {
        if (i >= c.n) continue;
        const double Vb = Vtop[i] - c.w[i] * c.L[i];
        if (!(i == 0 && contact) && Vb < 0.0 && Vtop[i] > 0.0) {
            const double drop = moor_sag_drop(H, Vb, c.EA[i], c.w[i]);
            if (z - drop < floor) grounded = true;
        }
        MoorEval s;
        moor_eval(H, Vtop[i], c.L[i], c.EA[i], c.w[i], seabed && i == 0, s);
        z += s.Z;
        if (i + 1 < c.n && z < floor) grounded = true;
    }
    return grounded;
}
// A chain at the pose ps: the head row `line` and the nc continuation rows after it.  The records lw of all its rows and, where
// lo_out is not null and the chain is not flagged, their line_out rows.  NOT inlined, and every argument a scalar or a pointer
// to global memory: k_moor_line and k_mean_pose call one body, so the records of a chain are the same bits from both (for a
// single line the two kernels' inlined copies of one source have always agreed; nothing promises that of a second, larger body).
__device__ __noinline__ void moor_chain_record(const double *__restrict__ line, const int nc, const MoorPose pose, const double depth,
                                               double *__restrict__ lw, double *__restrict__ lo_out) {
    double rec[RAFTX_ML_N], ps[6], Lt, Wt;
    MoorChain c;
    bool fin, pos;
    moor_chain_load(line, nc, pose, rec, ps, c, fin, pos, Lt, Wt);
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
        else if (moor_chain_grounded(c, H, Vtop, e.contact, seabed, az, depth)) flag = RAFTX_MOOR_GROUNDED;
    }
    if (!flag) {
        MoorEnd m;
        moor_end_set(m, H, V, e, ux, uy, XF);
#pragma unroll
        for (int i = 0; i < RAFTX_MOOR_MAX_SEG; i++) {
            if (i >= c.n) continue;
            const bool ct = i == 0 && e.contact;
            const double VB = Vtop[i], VA = ct ? 0.0 : VB - c.w[i] * c.L[i];
            moor_row_write(lw + (size_t)i * MOOR_LW_N, m, r, i == 0, VA, VB);
            if (lo_out) moor_lo_write(lo_out + (size_t)i * MOOR_LO_N, H, VB, VA, ct ? c.L[0] - VB / c.w[0] : 0.0, it, ct);
        }
    }
#pragma unroll
    for (int i = 0; i < RAFTX_MOOR_MAX_SEG; i++)
        if (i < c.n) lw[(size_t)i * MOOR_LW_N + 23] = (double)flag;
}

// ---- bridles (include/raftx_mooring.h: stem rows anchor -> junction, then 2 .. RAFTX_MOOR_MAX_LEG leg rows junction ->
// fairlead).  The unknown is the junction P; at every P the stem is shot in the vertical plane through the anchor and P
// (moor_chain_eval) and every leg, a suspended catenary, in its own plane (moor_eval without a seabed), and
//     R(P) = f_stem + sum f_leg,lower end - (0, 0, W_junction) = 0,       dR/dP = -K_PP = -(K_stem + sum K_leg)
// with the 3 x 3 end stiffness K = [k11 u u' + HF/XF (I_h - u u'), k12 u; k12 u', k22] of an element, (k) the inverse of its
// catenary Jacobian.  At the solution the fairleads see K_ij = K_i d_ij - K_i K_PP^-1 K_j, and dP/dx6 = K_PP^-1 sum K_j [I, -[r_j x]].
// The legs of the rows after a head row `line` and its nc continuation rows (0: no bridle), within the nAfter rows that follow
__device__ __forceinline__ int moor_bridle_legs(const double *__restrict__ line, const int nAfter, const int nc) {
    int n = 0;
    while (nc + n < nAfter && n < RAFTX_MOOR_MAX_LEG && line[(size_t)(nc + n + 1) * RAFTX_ML_N + RAFTX_ML_LEG] != 0.0) n++;
    return n;
}
// The rows of the bridle whose head row is `line` (0: `line` is no head row of a bridle)
__device__ __forceinline__ int moor_bridle_rows(const double *__restrict__ line, const int nAfter) {
    if (line[RAFTX_ML_CONT] != 0.0 || line[RAFTX_ML_LEG] != 0.0) return 0;
    int nc = 0;
    while (nc < nAfter && nc < RAFTX_MOOR_MAX_SEG - 1 && line[(size_t)(nc + 1) * RAFTX_ML_N + RAFTX_ML_CONT] != 0.0) nc++;
    const int nleg = moor_bridle_legs(line, nAfter, nc);
    return nleg ? nc + 1 + nleg : 0;
}

// y = S x with S symmetric (xx xy xz yy yz zz)
__device__ __forceinline__ void moor_sym_mul(const double S[6], const double x[3], double y[3]) {
    y[0] = S[0] * x[0] + S[1] * x[1] + S[2] * x[2];
    y[1] = S[1] * x[0] + S[3] * x[1] + S[4] * x[2];
    y[2] = S[2] * x[0] + S[4] * x[1] + S[5] * x[2];
}
__device__ __forceinline__ double moor_sym_at(const double S[6], const int i, const int j) {
    const int a = i < j ? i : j, b = i < j ? j : i;
    return S[a == 0 ? b : (a == 1 ? 2 + b : 5)];
}

// A bridle at the pose: the head row `line`, its nc continuation rows and the nleg leg rows after them.  The lw records of all
// its rows carry the flag only; its share of C_moor / F_moor and every row end's T and J go to the bw records (MOOR_BW_N per
// row, bw at the head row's); line_out rows at lo_out unless flagged.  NOT inlined, for the reason moor_chain_record gives.
__device__ __noinline__ void moor_bridle_record(const double *__restrict__ line, const int nc, const int nleg, const MoorPose pose,
                                                const double depth, double *__restrict__ lw, double *__restrict__ bw,
                                                double *__restrict__ lo_out) {
    const int nrow = nc + 1 + nleg;
    double rec[RAFTX_ML_N], ps[6], Ls, Ws;
    MoorChain c;                                                 // the stem
    bool fin, pos;
    moor_chain_load(line, nc, pose, rec, ps, c, fin, pos, Ls, Ws);
    MoorChain g[RAFTX_MOOR_MAX_LEG];                             // the legs, one segment each
    double rl[RAFTX_MOOR_MAX_LEG][3], pf[RAFTX_MOOR_MAX_LEG][3];  // arms R r_f and fairlead positions
    double Wj = 0.0, Wl = 0.0;
#pragma unroll
    for (int i = 0; i < RAFTX_MOOR_MAX_LEG; i++) {
        g[i].n = 1; g[i].L[0] = 1.0; g[i].EA[0] = 1.0; g[i].w[0] = 1.0; g[i].Wj[0] = 0.0;
        rl[i][0] = rl[i][1] = rl[i][2] = 0.0;
        pf[i][0] = pf[i][1] = pf[i][2] = 0.0;
        if (i >= nleg) continue;
        const double *p = line + (size_t)(nc + 1 + i) * RAFTX_ML_N;
        double lr[RAFTX_ML_N];
#pragma unroll
        for (int k = 0; k < RAFTX_ML_N; k++) lr[k] = p[k];
        for (int k = 3; k < 11; k++) fin = fin && isfinite(lr[k]);
        g[i].L[0] = lr[6]; g[i].EA[0] = lr[7]; g[i].w[0] = lr[8];
        pos = pos && lr[6] > 0.0 && lr[7] > 0.0 && lr[8] > 0.0;
        if (i == 0) Wj = lr[RAFTX_ML_WJOINT];
        Wl += lr[8] * lr[6];
        if (fin) {
            moor_arm(lr, ps, rl[i]);
#pragma unroll
            for (int k = 0; k < 3; k++) pf[i][k] = ps[k] + rl[i][k];
        }
    }
    const double az = rec[2];
    const double Wt = Ws + Wl;                                   // the scale of the force balance
    int flag = 0;
    if (!fin || !pos || !(Ws > 0.0) || !(Wt + Wj > 0.0) || az < -depth - 1e-6 * depth) flag = RAFTX_MOOR_BAD_LINE;
    if (!flag) {
        bool slack = true;
#pragma unroll
        for (int i = 0; i < RAFTX_MOOR_MAX_LEG; i++) {
            if (i >= nleg) continue;
            const double dx = pf[i][0] - rec[0], dy = pf[i][1] - rec[1], XFi = sqrt(dx * dx + dy * dy), ZFi = pf[i][2] - az;
            if (!(ZFi > 0.0)) flag = RAFTX_MOOR_BAD_LINE;
            slack = slack && (Ls + g[i].L[0] >= XFi + ZFi);
        }
        if (!flag && slack) flag = RAFTX_MOOR_SLACK;
    }
    const bool seabed = fabs(az + depth) <= 1e-6 * depth;
    const double wes = Ws / Ls;
    // the accepted state: junction, residual, elements
    double P[3] = {0, 0, 0}, R[3] = {0, 0, 0}, d[3] = {0, 0, 0}, Ki[6] = {0, 0, 0, 0, 0, 0}, res = 0.0, a = 1.0;
    MoorEnd S, G[RAFTX_MOOR_MAX_LEG];
    MoorEval es;
    double Vtop[RAFTX_MOOR_MAX_SEG] = {0, 0, 0, 0}, XFs = 0.0;
    int it = 0;
    bool have = false, conv = false, up = false;
    if (!flag) {
        // the start: the stem with ONE equivalent leg above it (the legs' summed EA and weight, their mean length along the axis)
        // to the centroid of the fairleads, shot as a composite line; the junction is that leg's span below the centroid.  Where
        // this plane problem has no solution: on the straight line from the anchor to the centroid.
        double cf[3] = {0, 0, 0};
#pragma unroll
        for (int i = 0; i < RAFTX_MOOR_MAX_LEG; i++)
            if (i < nleg)
                for (int k = 0; k < 3; k++) cf[k] += pf[i][k];
        for (int k = 0; k < 3; k++) cf[k] = cf[k] / (double)nleg;
        double Le = 0.0, EAe = 0.0;
#pragma unroll
        for (int i = 0; i < RAFTX_MOOR_MAX_LEG; i++) {
            if (i >= nleg) continue;
            const double ox = pf[i][0] - cf[0], oy = pf[i][1] - cf[1], oz = pf[i][2] - cf[2], Li = g[i].L[0];
            Le += sqrt(fmax(Li * Li - (ox * ox + oy * oy + oz * oz), 0.25 * Li * Li));
            EAe += g[i].EA[0];
        }
        Le = Le / (double)nleg;
        double Pt[3];
#pragma unroll
        for (int k = 0; k < 3; k++) Pt[k] = rec[k] + (Ls / (Ls + Le)) * (cf[k] - rec[k]);
        {
            const double dxc = cf[0] - rec[0], dyc = cf[1] - rec[1], ZFc = cf[2] - az, XFc = sqrt(dxc * dxc + dyc * dyc);
            if (XFc > 1e-9 * (Ls + Le) && (!seabed || Ls + Le < XFc + ZFc)) {
                const double top[4] = {Le, EAe, Wl / Le, Wj};
                double H0, V0, V4[RAFTX_MOOR_MAX_SEG] = {0, 0, 0, 0};
                MoorEval e0;
                if (moor_shoot<2>(c, seabed, top, Ls + Le, (Wt + Wj) / (Ls + Le), XFc, ZFc, H0, V0, e0, V4)) {
                    MoorEval t;
                    moor_eval(H0, V0, top[0], top[1], top[2], false, t);
                    Pt[0] = cf[0] - t.X * (dxc / XFc);
                    Pt[1] = cf[1] - t.X * (dyc / XFc);
                    Pt[2] = cf[2] - t.Z;
                }
            }
        }
        for (;;) {
            // everything at the trial junction Pt
            bool ok = true;
            MoorEnd St, Gt[RAFTX_MOOR_MAX_LEG];
            MoorEval et;
            double Vt[RAFTX_MOOR_MAX_SEG] = {0, 0, 0, 0}, Rt[3], Kt[6], XFt = 0.0;
            {
                const double dx = Pt[0] - rec[0], dy = Pt[1] - rec[1], ZF = Pt[2] - az;
                XFt = sqrt(dx * dx + dy * dy);
                ok = XFt > 1e-9 * Ls && (!seabed || (ZF > 0.0 && Ls < XFt + ZF));      // (a stem on the seabed: no fully slack profile)
                if (ok) {
                    double H, V;
                    ok = moor_shoot<0>(c, seabed, nullptr, Ls, wes, XFt, ZF, H, V, et, Vt);
                    moor_end_set(St, H, V, et, dx / XFt, dy / XFt, XFt);
                    Rt[0] = -H * St.ux; Rt[1] = -H * St.uy; Rt[2] = -V - Wj;
#pragma unroll
                    for (int k = 0; k < 6; k++) Kt[k] = St.K[k];
                }
            }
#pragma unroll
            for (int i = 0; i < RAFTX_MOOR_MAX_LEG; i++) {
                if (i >= nleg || !ok) continue;
                const double dx = pf[i][0] - Pt[0], dy = pf[i][1] - Pt[1], ZF = pf[i][2] - Pt[2];
                const double XF = sqrt(dx * dx + dy * dy);
                ok = XF > 1e-9 * g[i].L[0];
                if (!ok) continue;
                double H, V, Vn[RAFTX_MOOR_MAX_SEG];
                MoorEval el;
                ok = moor_shoot<1>(g[i], false, nullptr, g[i].L[0], g[i].w[0], XF, ZF, H, V, el, Vn);
                moor_end_set(Gt[i], H, V, el, dx / XF, dy / XF, XF);
                Rt[0] += H * Gt[i].ux; Rt[1] += H * Gt[i].uy; Rt[2] += V - g[i].w[0] * g[i].L[0];
#pragma unroll
                for (int k = 0; k < 6; k++) Kt[k] += Gt[i].K[k];
            }
            const double rt = ok ? fmax(fmax(fabs(Rt[0]), fabs(Rt[1])), fabs(Rt[2])) / Wt : 0.0;
            bool take = false;
            if (!have) {
                if (!ok) break;                                  // no start: NO_CONVERGENCE
                take = true;
            } else if (ok && rt < res) {
                take = true;
                up = false;
            } else if (res <= MOOR_TIGHT) {
                conv = true;
                break;
            } else if (ok && !up && a == 1.0 && rt <= MOOR_BR_GROW * res) {
                take = true;                                     // a full step from the soft side lands on the stiff side: Newton's way in
                up = true;
            } else {
                a *= 0.5;
                if (a < 0x1p-40) break;
            }
            if (take) {
                have = true;
#pragma unroll
                for (int k = 0; k < 3; k++) { P[k] = Pt[k]; R[k] = Rt[k]; }
                res = rt; a = 1.0;
                S = St; es = et; XFs = XFt;
#pragma unroll
                for (int i = 0; i < RAFTX_MOOR_MAX_SEG; i++) Vtop[i] = Vt[i];
#pragma unroll
                for (int i = 0; i < RAFTX_MOOR_MAX_LEG; i++) G[i] = Gt[i];
                // K_PP^-1 (symmetric) by cofactors, and the Newton step d = K_PP^-1 R
                const double c0 = Kt[3] * Kt[5] - Kt[4] * Kt[4], c1 = Kt[2] * Kt[4] - Kt[1] * Kt[5], c2 = Kt[1] * Kt[4] - Kt[2] * Kt[3];
                const double det = Kt[0] * c0 + Kt[1] * c1 + Kt[2] * c2;
                Ki[0] = c0 / det; Ki[1] = c1 / det; Ki[2] = c2 / det;
                Ki[3] = (Kt[0] * Kt[5] - Kt[2] * Kt[2]) / det;
                Ki[4] = (Kt[1] * Kt[2] - Kt[0] * Kt[4]) / det;
                Ki[5] = (Kt[0] * Kt[3] - Kt[1] * Kt[1]) / det;
                moor_sym_mul(Ki, R, d);
                if (res == 0.0) { conv = true; break; }
            }
            if (it >= MOOR_BR_MAX_IT) break;
            it++;
#pragma unroll
            for (int k = 0; k < 3; k++) Pt[k] = P[k] + a * d[k];
        }
        if (!conv) flag = RAFTX_MOOR_NO_CONVERGENCE;
    }
    if (!flag) {
        // the seabed: the stem by the chain's rule, then the junction and the sags of the legs
        const double floor = -depth - 1e-6 * depth;
        if (moor_chain_grounded(c, S.H, Vtop, es.contact, seabed, az, depth)) flag = RAFTX_MOOR_GROUNDED;
        if (P[2] < floor) flag = RAFTX_MOOR_GROUNDED;
#pragma unroll
        for (int i = 0; i < RAFTX_MOOR_MAX_LEG; i++) {
            if (i >= nleg) continue;
            const double Vb = G[i].V - g[i].w[0] * g[i].L[0];
            if (Vb < 0.0 && G[i].V > 0.0) {
                const double drop = moor_sag_drop(G[i].H, Vb, g[i].EA[0], g[i].w[0]);
                if (P[2] - drop < floor) flag = RAFTX_MOOR_GROUNDED;
            }
        }
    }
    if (!flag) {
        // D_j = K_PP^-1 K_j, and dP/dx6 = sum_j D_j [I, -[r_j x]]
        double D[RAFTX_MOOR_MAX_LEG][3][3], DP[3][6];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 6; j++) DP[i][j] = 0.0;
#pragma unroll
        for (int j = 0; j < RAFTX_MOOR_MAX_LEG; j++) {
            if (j >= nleg) continue;
            const double *r = rl[j];
            const double RX[3][3] = {{0.0, -r[2], r[1]}, {r[2], 0.0, -r[0]}, {-r[1], r[0], 0.0}};
#pragma unroll
            for (int i = 0; i < 3; i++) {
#pragma unroll
                for (int k = 0; k < 3; k++)
                    D[j][i][k] = moor_sym_at(Ki, i, 0) * moor_sym_at(G[j].K, 0, k) + moor_sym_at(Ki, i, 1) * moor_sym_at(G[j].K, 1, k) +
                                 moor_sym_at(Ki, i, 2) * moor_sym_at(G[j].K, 2, k);
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    DP[i][k] += D[j][i][k];
                    DP[i][3 + k] += -(D[j][i][0] * RX[0][k] + D[j][i][1] * RX[1][k] + D[j][i][2] * RX[2][k]);
                }
            }
        }
        // the share of C_moor and F_moor: over the pairs of fairleads, then the arm turning of each
        double C[36], F[6];
#pragma unroll
        for (int i = 0; i < 36; i++) C[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 6; i++) F[i] = 0.0;
#pragma unroll
        for (int i = 0; i < RAFTX_MOOR_MAX_LEG; i++) {
            if (i >= nleg) continue;
            const double *ri = rl[i];
            const double RI[3][3] = {{0.0, -ri[2], ri[1]}, {ri[2], 0.0, -ri[0]}, {-ri[1], ri[0], 0.0}};
            const double f[3] = {-G[i].H * G[i].ux, -G[i].H * G[i].uy, -G[i].V};
            const double FX[3][3] = {{0.0, -f[2], f[1]}, {f[2], 0.0, -f[0]}, {-f[1], f[0], 0.0}};
#pragma unroll
            for (int j = 0; j < RAFTX_MOOR_MAX_LEG; j++) {
                if (j >= nleg) continue;
                const double *rj = rl[j];
                const double RJ[3][3] = {{0.0, -rj[2], rj[1]}, {rj[2], 0.0, -rj[0]}, {-rj[1], rj[0], 0.0}};
                double M[3][3], MR[3][3], RM[3][3];                 // K_ij, K_ij [r_j x], [r_i x] K_ij
#pragma unroll
                for (int p = 0; p < 3; p++)
#pragma unroll
                    for (int q = 0; q < 3; q++) {
                        const double kd = moor_sym_at(G[i].K, p, 0) * D[j][0][q] + moor_sym_at(G[i].K, p, 1) * D[j][1][q] +
                                          moor_sym_at(G[i].K, p, 2) * D[j][2][q];
                        M[p][q] = (i == j ? moor_sym_at(G[i].K, p, q) : 0.0) - kd;
                    }
#pragma unroll
                for (int p = 0; p < 3; p++)
#pragma unroll
                    for (int q = 0; q < 3; q++) {
                        MR[p][q] = M[p][0] * RJ[0][q] + M[p][1] * RJ[1][q] + M[p][2] * RJ[2][q];
                        RM[p][q] = RI[p][0] * M[0][q] + RI[p][1] * M[1][q] + RI[p][2] * M[2][q];
                    }
#pragma unroll
                for (int p = 0; p < 3; p++)
#pragma unroll
                    for (int q = 0; q < 3; q++) {
                        const double rmr = RI[p][0] * MR[0][q] + RI[p][1] * MR[1][q] + RI[p][2] * MR[2][q];
                        C[6 * p + q] += M[p][q];
                        C[6 * p + 3 + q] += -MR[p][q];
                        C[6 * (3 + p) + q] += RM[p][q];
                        C[6 * (3 + p) + 3 + q] += -rmr;
                    }
            }
#pragma unroll
            for (int p = 0; p < 3; p++)
#pragma unroll
                for (int q = 0; q < 3; q++)
                    C[6 * (3 + p) + 3 + q] += -(FX[p][0] * RI[0][q] + FX[p][1] * RI[1][q] + FX[p][2] * RI[2][q]);
            F[0] += f[0]; F[1] += f[1]; F[2] += f[2];
            F[3] += ri[1] * f[2] - ri[2] * f[1];
            F[4] += ri[2] * f[0] - ri[0] * f[2];
            F[5] += ri[0] * f[1] - ri[1] * f[0];
        }
#pragma unroll
        for (int i = 0; i < 36; i++) bw[i] = C[i];
#pragma unroll
        for (int i = 0; i < 6; i++) bw[36 + i] = F[i];
        // the stem's rows: T and its gradient for a junction displacement, through dP/dx6
#pragma unroll
        for (int i = 0; i < RAFTX_MOOR_MAX_SEG; i++) {
            if (i >= c.n) continue;
            double *b = bw + (size_t)i * MOOR_BW_N;
            const bool ct = i == 0 && es.contact;
            const double VB = Vtop[i], VA = ct ? 0.0 : VB - c.w[i] * c.L[i];
            const double TB = sqrt(S.H * S.H + VB * VB), TA = sqrt(S.H * S.H + VA * VA);
            b[42] = TA; b[43] = TB;
#pragma unroll
            for (int e = 0; e < 2; e++) {
                double g3[3];
                moor_end_grad(S, e ? VB : VA, e ? TB : TA, g3);
#pragma unroll
                for (int k = 0; k < 6; k++) b[44 + 6 * e + k] = g3[0] * DP[0][k] + g3[1] * DP[1][k] + g3[2] * DP[2][k];
            }
            if (lo_out) moor_lo_write(lo_out + (size_t)i * MOOR_LO_N, S.H, VB, VA, ct ? c.L[0] - VB / c.w[0] : 0.0, it, ct);
        }
        // the legs' rows: the relative displacement of their ends is [I, -[r_i x]] - dP/dx6
#pragma unroll
        for (int i = 0; i < RAFTX_MOOR_MAX_LEG; i++) {
            if (i >= nleg) continue;
            double *b = bw + (size_t)(c.n + i) * MOOR_BW_N;
            const double *r = rl[i];
            const double RX[3][3] = {{0.0, -r[2], r[1]}, {r[2], 0.0, -r[0]}, {-r[1], r[0], 0.0}};
            const double H = G[i].H, VB = G[i].V, VA = VB - g[i].w[0] * g[i].L[0];
            const double TB = sqrt(H * H + VB * VB), TA = sqrt(H * H + VA * VA);
            b[42] = TA; b[43] = TB;
#pragma unroll
            for (int e = 0; e < 2; e++) {
                double g3[3];
                moor_end_grad(G[i], e ? VB : VA, e ? TB : TA, g3);
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    b[44 + 6 * e + k] = (g3[k] - g3[0] * DP[0][k]) - g3[1] * DP[1][k] - g3[2] * DP[2][k];
                    const double gr = -(g3[0] * RX[0][k] + g3[1] * RX[1][k] + g3[2] * RX[2][k]);
                    b[44 + 6 * e + 3 + k] = (gr - g3[0] * DP[0][3 + k]) - g3[1] * DP[1][3 + k] - g3[2] * DP[2][3 + k];
                }
            }
            if (lo_out) moor_lo_write(lo_out + (size_t)(c.n + i) * MOOR_LO_N, H, VB, VA, 0.0, it, false);
        }
    }
    for (int i = 0; i < nrow; i++) {
        double *q = lw + (size_t)i * MOOR_LW_N;
        for (int k = 0; k < 23; k++) q[k] = 0.0;
        q[23] = (double)flag;
    }
}

// The share of a bridle (the bw record of its head row) in C_moor and F_moor, and a row's T, J and Lr (J as rows of
// k_sweep_channels: plane 0 = J, the other two zero), each or null: k_moor_design's part
__device__ __forceinline__ void moor_bridle_share(const double *__restrict__ b, double C[36], double F[6]) {
#pragma unroll
    for (int i = 0; i < 36; i++) C[i] += b[i];
#pragma unroll
    for (int i = 0; i < 6; i++) F[i] += b[36 + i];
}
__device__ __forceinline__ void moor_bridle_TJ(const double *__restrict__ b, const int l, const int nL, double *__restrict__ T,
                                               double *__restrict__ J, double *__restrict__ Lr = nullptr) {
    if (T) { T[l] = b[42]; T[nL + l] = b[43]; }
    if (J)
#pragma unroll
        for (int e = 0; e < 2; e++)
#pragma unroll
            for (int k = 0; k < 6; k++) J[(size_t)(e * nL + l) * 6 + k] = b[44 + 6 * e + k];
    if (Lr)
#pragma unroll
        for (int e = 0; e < 2; e++)
#pragma unroll
            for (int i = 0; i < 18; i++) Lr[(size_t)(e * nL + l) * 18 + i] = i < 6 ? b[44 + 6 * e + i] : 0.0;
}

// One line at the pose ps: the record lw [MOOR_LW_N] (in global memory) and lo [MOOR_LO_N].  The body of k_moor_line, shared
// with k_mean_pose (raftx_statics.h).  Returns true: lo is this row's line_out.  CHAINS: `line` may be the head row of a
// composite line, with its continuation rows among the nAfter rows of the design that follow it -- then the records of all of
// them are written, and their line_out rows at lo_out (this row's place in global memory, or null) unless the chain is flagged
// -- or a continuation row itself, for which nothing is written; false is returned in both cases.
template <bool CHAINS, bool BRIDLES = false>
__device__ __forceinline__ bool moor_line_record(const double *__restrict__ line, const int nAfter, const double ps[6],
                                                 const double depth, double *__restrict__ lw, double lo[MOOR_LO_N],
                                                 double *__restrict__ lo_out, double *__restrict__ bw = nullptr) {
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
        if (BRIDLES && rec[RAFTX_ML_LEG] != 0.0) return false;
        int nc = 0;
        while (nc < nAfter && nc < RAFTX_MOOR_MAX_SEG - 1 && line[(size_t)(nc + 1) * RAFTX_ML_N + RAFTX_ML_CONT] != 0.0) nc++;
        if (BRIDLES) {
            const int nleg = moor_bridle_legs(line, nAfter, nc);
            if (nleg) {
                MoorPose pose;
#pragma unroll
                for (int i = 0; i < 6; i++) pose.v[i] = ps[i];
                moor_bridle_record(line, nc, nleg, pose, depth, lw, bw, lo_out);
                return false;
            }
        }
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

template <bool CHAINS, bool BRIDLES = false>
__global__ void __launch_bounds__(MOOR_THREADS) k_moor_line(MoorArgs A) {
    const long long t = (long long)blockIdx.x * MOOR_THREADS + threadIdx.x;
    if (t >= (long long)A.nDesign * A.nLine) return;
    const int d = (int)(t / A.nLine);
    double ps[6] = {0, 0, 0, 0, 0, 0};
    if (A.pose)
        for (int i = 0; i < 6; i++) ps[i] = A.pose[(size_t)d * 6 + i];
    double lo[MOOR_LO_N];
    const bool mine = moor_line_record<CHAINS, BRIDLES>(A.lines + (size_t)t * RAFTX_ML_N, A.nLine - 1 - (int)(t % A.nLine), ps, A.depth,
                                                        A.lw + (size_t)t * MOOR_LW_N, lo,
                                                        A.line_out ? A.line_out + (size_t)t * MOOR_LO_N : nullptr,
                                                        BRIDLES ? A.bw + (size_t)t * MOOR_BW_N : nullptr);
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
// The six J values of end e (0: A, 1: B) of a row from its record q: (g, r x g)
__device__ __forceinline__ void moor_row_J(const double *__restrict__ q, const int e, double *o) {
    const double r[3] = {q[3], q[4], q[5]};
    const double *g = q + 15 + 3 * e;
    o[0] = g[0]; o[1] = g[1]; o[2] = g[2];
    o[3] = r[1] * g[2] - r[2] * g[1];
    o[4] = r[2] * g[0] - r[0] * g[2];
    o[5] = r[0] * g[1] - r[1] * g[0];
}
__device__ __forceinline__ void moor_line_TJ(const double *__restrict__ q, const int l, const int nL, double *__restrict__ T,
                                             double *__restrict__ J, double *__restrict__ Lr = nullptr) {
    if (T) { T[l] = q[21]; T[nL + l] = q[22]; }
    if (J)
#pragma unroll
        for (int e = 0; e < 2; e++) moor_row_J(q, e, J + (size_t)(e * nL + l) * 6);
    if (Lr)
#pragma unroll
        for (int e = 0; e < 2; e++) {
            double *o = Lr + (size_t)(e * nL + l) * 18;
            moor_row_J(q, e, o);
#pragma unroll
            for (int i = 6; i < 18; i++) o[i] = 0.0;
        }
}

// The walk over the nL rows of ONE design (its lines, its records lw and, with BRIDLES, bw): a bridle from its head row once,
// else the line's own.  SUMS: the shares in C_moor [36] and F_moor [6], added in row order from zero; ROWS: T [2 nL],
// J [2 nL,6] and Lr [2 nL,3,6] (each or null) of every row.  k_moor_design does both in one pass; k_mean_pose
// (raftx_statics.h) the sums at every step and the rows once, through the two functions below.
template <bool BRIDLES, bool SUMS, bool ROWS>
__device__ __forceinline__ void moor_design_walk(const double *__restrict__ lines, const double *lw, const double *bw, const int nL,
                                                 double *C, double *F, double *__restrict__ T, double *__restrict__ J,
                                                 double *__restrict__ Lr) {
    if (SUMS) {
#pragma unroll
        for (int i = 0; i < 36; i++) C[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 6; i++) F[i] = 0.0;
    }
    for (int l = 0; l < nL; l++) {
        if (BRIDLES) {
            const int nb = moor_bridle_rows(lines + (size_t)l * RAFTX_ML_N, nL - 1 - l);
            if (nb) {                                            // a bridle, from its head row: the share once, T and J of all its rows
                const double *b = bw + (size_t)l * MOOR_BW_N;
                if (SUMS) moor_bridle_share(b, C, F);
                if (ROWS)
                    for (int k = 0; k < nb; k++) moor_bridle_TJ(b + (size_t)k * MOOR_BW_N, l + k, nL, T, J, Lr);
                l += nb - 1;
                continue;
            }
        }
        if (SUMS) moor_line_share(lw + (size_t)l * MOOR_LW_N, C, F);
        if (ROWS) moor_line_TJ(lw + (size_t)l * MOOR_LW_N, l, nL, T, J, Lr);
    }
}
template <bool BRIDLES>
__device__ __forceinline__ void moor_design_sums(const double *__restrict__ lines, const double *lw, const double *bw, const int nL,
                                                 double C[36], double F[6]) {
    moor_design_walk<BRIDLES, true, false>(lines, lw, bw, nL, C, F, nullptr, nullptr, nullptr);
}
template <bool BRIDLES>
__device__ __forceinline__ void moor_design_TJ(const double *__restrict__ lines, const double *lw, const double *bw, const int nL,
                                               double *__restrict__ T, double *__restrict__ J) {
    moor_design_walk<BRIDLES, false, true>(lines, lw, bw, nL, nullptr, nullptr, T, J, nullptr);
}

template <bool BRIDLES>
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
    const double *lines = A.lines + (size_t)d * nL * RAFTX_ML_N, *bw0 = BRIDLES ? A.bw + (size_t)d * nL * MOOR_BW_N : nullptr;
    double C[36], F[6];
    moor_design_walk<BRIDLES, true, true>(A.lines + (size_t)d * nL * RAFTX_ML_N, lw0, BRIDLES ? A.bw + (size_t)d * nL * MOOR_BW_N : nullptr, nL,
                                          C, F, T, J, A.Lr ? A.Lr + (size_t)d * 36 * nL : nullptr);
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
