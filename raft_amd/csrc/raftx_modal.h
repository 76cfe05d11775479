// raftx_modal.h -- batched eigen analysis of rigid 6-DOF systems (included by raftx_hip.hip; entry points in
// include/raftx_modal.h).
//
// Per system (raft_fowt.py:1646-1729, raft_model.py:436-547 for one unit without an array mooring system):
//   M_tot, C_tot                    arrive summed (the caller's, or the resident M0 + dM, C0 + dC)
//   viability                       a diagonal below 1 sets SMALL_DIAG (the reference raises; here the numbers go on)
//   A = solve(M_tot, C_tot)         LU with partial pivoting, first index of the largest |a| as pivot (LAPACK gesv)
//   balance A                       exact power-of-two row / column scaling (EISPACK balanc, dgebal's scaling step)
//   Hessenberg                      Householder reduction with the transformations accumulated (orthes + ortran)
//   Schur form + eigenvectors       Francis double-shift QR, back-substitution of the real quasi-triangular form
//                                   (hqr2); at most 30 N QR steps in all, then NO_CONVERGENCE
//   undo the balancing, unit 2-norm columns, sign: largest |component| positive (first index on ties)
//   DOF order                       rows N-1 .. 0 each claim the unclaimed column of largest |v| (first on ties); the
//                                   list reversed: output column i is the column row i claimed
//
// modal_core_n<N> is this method for any N <= 36 as serial code: N = 6 is the rigid unit (modal_core, k_modal below); the
// larger sizes are the arrays of 6 nUnit DOFs, which raftx_array_modal.h runs with one wavefront per system and checks
// against this text on the host (tests/csrc/array_modal_driver.cpp).
//
// Data layout: one system per lane.  Everything indexed at run time (H, Z and the small vectors: the deflation
// window and the pivot rows have run-time bounds) lives in LDS as [entry][lane] -- 8-byte words of consecutive lanes
// are consecutive, no bank conflicts -- so the kernel has no private segment.  The block's input matrices are read
// with coalesced loads straight into that layout.
#pragma once

#ifndef RAFTX_MODAL_HD
#define RAFTX_MODAL_HD __host__ __device__
#endif

#define MODAL_N 6
#define MODAL_V_D 0              // d[6]: real parts of the eigenvalues
#define MODAL_V_E 6              // e[6]: imaginary parts
#define MODAL_V_SC 12            // scale[6]: balancing
#define MODAL_V_ORT 18           // ort[6]: Householder vectors
#define MODAL_NV 24
#define MODAL_NE (2 * 36 + MODAL_NV)   // LDS words per lane: H, Z (M before the solve), the vectors

// The claim mask of the DOF order: 32 bits up to 32 DOFs (the rigid unit's instance stays what it was), 64 above.
template <bool WIDE> struct ModalMask { typedef unsigned type; };
template <> struct ModalMask<true> { typedef unsigned long long type; };

// S: H(i, j), Z(i, j), V(k) -- references into the system's storage.  On entry Z holds M_tot and H holds C_tot.
// N DOFs (6 for one rigid unit, 6 nUnit <= 36 for an array: V holds 4 N words, d | e | scale | ort, at MODAL_V_* scaled
// by N / 6).  fn [N], modes [N*N] (row-major, column i = DOF i's mode).  Returns the RAFTX_MODAL_* flags.
template <int N, class S>
RAFTX_MODAL_HD inline int modal_core_n(S &s, double *fn, double *modes) {
#pragma clang fp contract(off)
    const int n = N;
    const int VD = 0, VE = N, VSC = 2 * N, VORT = 3 * N;      // d, e, scale, ort in V (MODAL_V_* at N = 6)
    const double eps = 2.220446049250313e-16;            // 2^-52
    int flags = 0;
    for (int i = 0; i < n; i++)
        if (s.Z(i, i) < 1.0 || s.H(i, i) < 1.0) flags |= RAFTX_MODAL_SMALL_DIAG;
    // ---- LU of M (in Z) with partial pivoting, applied to the six right-hand sides in H
    for (int k = 0; k < n; k++) {
        int p = k;
        double amax = fabs(s.Z(k, k));
        for (int i = k + 1; i < n; i++) {
            const double a = fabs(s.Z(i, k));
            if (a > amax) { amax = a; p = i; }
        }
        if (amax == 0.0) { flags |= RAFTX_MODAL_SINGULAR_M; break; }
        if (p != k) {
            for (int j = 0; j < n; j++) {
                const double t = s.Z(k, j); s.Z(k, j) = s.Z(p, j); s.Z(p, j) = t;
                const double u = s.H(k, j); s.H(k, j) = s.H(p, j); s.H(p, j) = u;
            }
        }
        const double piv = s.Z(k, k);
        for (int i = k + 1; i < n; i++) {
            const double l = s.Z(i, k) / piv;
            s.Z(i, k) = l;
            for (int j = k + 1; j < n; j++) s.Z(i, j) = s.Z(i, j) - l * s.Z(k, j);
            for (int j = 0; j < n; j++) s.H(i, j) = s.H(i, j) - l * s.H(k, j);
        }
    }
    if (!(flags & RAFTX_MODAL_SINGULAR_M)) {
        for (int i = n - 1; i >= 0; i--)              // back substitution, column by column of the right-hand sides
            for (int j = 0; j < n; j++) {
                double t = s.H(i, j);
                for (int k = i + 1; k < n; k++) t = t - s.Z(i, k) * s.H(k, j);
                s.H(i, j) = t / s.Z(i, i);
            }
        // ---- balancing: powers of two only, so the scaled matrix is exactly similar
        for (int i = 0; i < n; i++) s.V(VSC + i) = 1.0;
        for (int sweep = 0; sweep < 64; sweep++) {
            bool noconv = false;
            for (int i = 0; i < n; i++) {
                double c = 0.0, r = 0.0;
                for (int j = 0; j < n; j++)
                    if (j != i) { c = c + fabs(s.H(j, i)); r = r + fabs(s.H(i, j)); }
                if (c == 0.0 || r == 0.0) continue;
                double g = r / 2.0, f = 1.0;
                const double tot = c + r;
                while (c < g) { f = f * 2.0; c = c * 4.0; }
                g = r * 2.0;
                while (c >= g) { f = f / 2.0; c = c / 4.0; }
                if ((c + r) / f < 0.95 * tot) {
                    const double gi = 1.0 / f;
                    s.V(VSC + i) = s.V(VSC + i) * f;
                    noconv = true;
                    for (int j = 0; j < n; j++) s.H(i, j) = s.H(i, j) * gi;
                    for (int j = 0; j < n; j++) s.H(j, i) = s.H(j, i) * f;
                }
            }
            if (!noconv) break;
        }
        // ---- Householder reduction to upper Hessenberg form
        for (int m = 1; m <= n - 2; m++) {
            double scale = 0.0;
            for (int i = m; i < n; i++) scale = scale + fabs(s.H(i, m - 1));
            if (scale != 0.0) {
                double h = 0.0;
                for (int i = n - 1; i >= m; i--) {
                    const double o = s.H(i, m - 1) / scale;
                    s.V(VORT + i) = o;
                    h = h + o * o;
                }
                double g = sqrt(h);
                if (s.V(VORT + m) > 0) g = -g;
                h = h - s.V(VORT + m) * g;
                s.V(VORT + m) = s.V(VORT + m) - g;
                for (int j = m; j < n; j++) {
                    double f = 0.0;
                    for (int i = n - 1; i >= m; i--) f = f + s.V(VORT + i) * s.H(i, j);
                    f = f / h;
                    for (int i = m; i < n; i++) s.H(i, j) = s.H(i, j) - f * s.V(VORT + i);
                }
                for (int i = 0; i < n; i++) {
                    double f = 0.0;
                    for (int j = n - 1; j >= m; j--) f = f + s.V(VORT + j) * s.H(i, j);
                    f = f / h;
                    for (int j = m; j < n; j++) s.H(i, j) = s.H(i, j) - f * s.V(VORT + j);
                }
                s.V(VORT + m) = scale * s.V(VORT + m);
                s.H(m, m - 1) = scale * g;
            }
        }
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) s.Z(i, j) = (i == j) ? 1.0 : 0.0;
        for (int m = n - 2; m >= 1; m--) {
            if (s.H(m, m - 1) != 0.0) {
                for (int i = m + 1; i < n; i++) s.V(VORT + i) = s.H(i, m - 1);
                for (int j = m; j < n; j++) {
                    double g = 0.0;
                    for (int i = m; i < n; i++) g = g + s.V(VORT + i) * s.Z(i, j);
                    g = (g / s.V(VORT + m)) / s.H(m, m - 1);
                    for (int i = m; i < n; i++) s.Z(i, j) = s.Z(i, j) + g * s.V(VORT + i);
                }
            }
        }
        for (int i = 2; i < n; i++)                        // the Householder vectors below the subdiagonal
            for (int j = 0; j < i - 1; j++) s.H(i, j) = 0.0;
        // ---- Francis double-shift QR on the Hessenberg form, transformations accumulated into Z
        double norm = 0.0;
        for (int i = 0; i < n; i++)
            for (int j = (i > 0 ? i - 1 : 0); j < n; j++) norm = norm + fabs(s.H(i, j));
        double exshift = 0.0, p = 0, q = 0, r = 0, sv = 0, z = 0, w, x, y;
        int iter = 0, total = 0;
        int nn = n - 1;
        while (nn >= 0) {
            int l = nn;
            while (l > 0) {
                sv = fabs(s.H(l - 1, l - 1)) + fabs(s.H(l, l));
                if (sv == 0.0) sv = norm;
                if (fabs(s.H(l, l - 1)) < eps * sv) break;
                l--;
            }
            if (l == nn) {                                // one root
                s.H(nn, nn) = s.H(nn, nn) + exshift;
                s.V(VD + nn) = s.H(nn, nn);
                s.V(VE + nn) = 0.0;
                nn--;
                iter = 0;
            } else if (l == nn - 1) {                     // two roots
                w = s.H(nn, nn - 1) * s.H(nn - 1, nn);
                p = (s.H(nn - 1, nn - 1) - s.H(nn, nn)) / 2.0;
                q = p * p + w;
                z = sqrt(fabs(q));
                s.H(nn, nn) = s.H(nn, nn) + exshift;
                s.H(nn - 1, nn - 1) = s.H(nn - 1, nn - 1) + exshift;
                x = s.H(nn, nn);
                if (q >= 0) {                             // a real pair: rotate it to triangular form
                    z = (p >= 0) ? p + z : p - z;
                    s.V(VD + nn - 1) = x + z;
                    s.V(VD + nn) = s.V(VD + nn - 1);
                    if (z != 0.0) s.V(VD + nn) = x - w / z;
                    s.V(VE + nn - 1) = 0.0;
                    s.V(VE + nn) = 0.0;
                    x = s.H(nn, nn - 1);
                    sv = fabs(x) + fabs(z);
                    p = x / sv;
                    q = z / sv;
                    r = sqrt(p * p + q * q);
                    p = p / r;
                    q = q / r;
                    for (int j = nn - 1; j < n; j++) {
                        z = s.H(nn - 1, j);
                        s.H(nn - 1, j) = q * z + p * s.H(nn, j);
                        s.H(nn, j) = q * s.H(nn, j) - p * z;
                    }
                    for (int i = 0; i <= nn; i++) {
                        z = s.H(i, nn - 1);
                        s.H(i, nn - 1) = q * z + p * s.H(i, nn);
                        s.H(i, nn) = q * s.H(i, nn) - p * z;
                    }
                    for (int i = 0; i < n; i++) {
                        z = s.Z(i, nn - 1);
                        s.Z(i, nn - 1) = q * z + p * s.Z(i, nn);
                        s.Z(i, nn) = q * s.Z(i, nn) - p * z;
                    }
                } else {                                  // a complex pair
                    s.V(VD + nn - 1) = x + p;
                    s.V(VD + nn) = x + p;
                    s.V(VE + nn - 1) = z;
                    s.V(VE + nn) = -z;
                    flags |= RAFTX_MODAL_COMPLEX;
                }
                nn -= 2;
                iter = 0;
            } else {                                      // no convergence yet: one more double-shift step
                if (++total > 30 * n) { flags |= RAFTX_MODAL_NO_CONVERGENCE; break; }
                x = s.H(nn, nn);
                y = 0.0;
                w = 0.0;
                if (l < nn) {
                    y = s.H(nn - 1, nn - 1);
                    w = s.H(nn, nn - 1) * s.H(nn - 1, nn);
                }
                if (iter == 10) {                         // Wilkinson's exceptional shift
                    exshift += x;
                    for (int i = 0; i <= nn; i++) s.H(i, i) = s.H(i, i) - x;
                    sv = fabs(s.H(nn, nn - 1)) + fabs(s.H(nn - 1, nn - 2));
                    x = y = 0.75 * sv;
                    w = -0.4375 * sv * sv;
                }
                if (iter == 30) {                         // a second exceptional shift
                    sv = (y - x) / 2.0;
                    sv = sv * sv + w;
                    if (sv > 0) {
                        sv = sqrt(sv);
                        if (y < x) sv = -sv;
                        sv = x - w / ((y - x) / 2.0 + sv);
                        for (int i = 0; i <= nn; i++) s.H(i, i) = s.H(i, i) - sv;
                        exshift += sv;
                        x = y = w = 0.964;
                    }
                }
                iter++;
                int m = nn - 2;                           // two consecutive small subdiagonal elements
                while (m >= l) {
                    z = s.H(m, m);
                    r = x - z;
                    sv = y - z;
                    p = (r * sv - w) / s.H(m + 1, m) + s.H(m, m + 1);
                    q = s.H(m + 1, m + 1) - z - r - sv;
                    r = s.H(m + 2, m + 1);
                    sv = fabs(p) + fabs(q) + fabs(r);
                    p = p / sv;
                    q = q / sv;
                    r = r / sv;
                    if (m == l) break;
                    if (fabs(s.H(m, m - 1)) * (fabs(q) + fabs(r)) <
                        eps * (fabs(p) * (fabs(s.H(m - 1, m - 1)) + fabs(z) + fabs(s.H(m + 1, m + 1)))))
                        break;
                    m--;
                }
                for (int i = m + 2; i <= nn; i++) {
                    s.H(i, i - 2) = 0.0;
                    if (i > m + 2) s.H(i, i - 3) = 0.0;
                }
                for (int k = m; k <= nn - 1; k++) {
                    const bool notlast = (k != nn - 1);
                    if (k != m) {
                        p = s.H(k, k - 1);
                        q = s.H(k + 1, k - 1);
                        r = notlast ? s.H(k + 2, k - 1) : 0.0;
                        x = fabs(p) + fabs(q) + fabs(r);
                        if (x == 0.0) continue;
                        p = p / x;
                        q = q / x;
                        r = r / x;
                    }
                    sv = sqrt(p * p + q * q + r * r);
                    if (p < 0) sv = -sv;
                    if (sv != 0) {
                        if (k != m) s.H(k, k - 1) = -sv * x;
                        else if (l != m) s.H(k, k - 1) = -s.H(k, k - 1);
                        p = p + sv;
                        x = p / sv;
                        y = q / sv;
                        z = r / sv;
                        q = q / p;
                        r = r / p;
                        for (int j = k; j < n; j++) {
                            p = s.H(k, j) + q * s.H(k + 1, j);
                            if (notlast) {
                                p = p + r * s.H(k + 2, j);
                                s.H(k + 2, j) = s.H(k + 2, j) - p * z;
                            }
                            s.H(k, j) = s.H(k, j) - p * x;
                            s.H(k + 1, j) = s.H(k + 1, j) - p * y;
                        }
                        const int ie = (nn < k + 3) ? nn : k + 3;
                        for (int i = 0; i <= ie; i++) {
                            p = x * s.H(i, k) + y * s.H(i, k + 1);
                            if (notlast) {
                                p = p + z * s.H(i, k + 2);
                                s.H(i, k + 2) = s.H(i, k + 2) - p * r;
                            }
                            s.H(i, k) = s.H(i, k) - p;
                            s.H(i, k + 1) = s.H(i, k + 1) - p * q;
                        }
                        for (int i = 0; i < n; i++) {
                            p = x * s.Z(i, k) + y * s.Z(i, k + 1);
                            if (notlast) {
                                p = p + z * s.Z(i, k + 2);
                                s.Z(i, k + 2) = s.Z(i, k + 2) - p * r;
                            }
                            s.Z(i, k) = s.Z(i, k) - p;
                            s.Z(i, k + 1) = s.Z(i, k + 1) - p * q;
                        }
                    }
                }
            }
        }
        if (!(flags & (RAFTX_MODAL_COMPLEX | RAFTX_MODAL_NO_CONVERGENCE))) {
            // ---- eigenvectors of the (now real upper triangular) Schur form, then back to A's basis
            if (norm != 0.0) {
                for (int k = n - 1; k >= 0; k--) {
                    const double lam = s.V(VD + k);
                    s.H(k, k) = 1.0;
                    for (int i = k - 1; i >= 0; i--) {
                        const double wd = s.H(i, i) - lam;
                        double acc = 0.0;
                        for (int j = i + 1; j <= k; j++) acc = acc + s.H(i, j) * s.H(j, k);
                        const double v = (wd != 0.0) ? -acc / wd : -acc / (eps * norm);
                        s.H(i, k) = v;
                        const double t = fabs(v);
                        if ((eps * t) * t > 1)
                            for (int j = i; j <= k; j++) s.H(j, k) = s.H(j, k) / t;
                    }
                }
                for (int j = n - 1; j >= 0; j--)
                    for (int i = 0; i < n; i++) {
                        double acc = 0.0;
                        for (int k = 0; k <= j; k++) acc = acc + s.Z(i, k) * s.H(k, j);
                        s.Z(i, j) = acc;
                    }
            }
            for (int i = 0; i < n; i++) {             // the balancing undone, unit 2-norm, the sign convention
                const double sc = s.V(VSC + i);
                for (int j = 0; j < n; j++) s.Z(i, j) = s.Z(i, j) * sc;
            }
            for (int j = 0; j < n; j++) {
                double ss = 0.0, big = -1.0;
                int ib = 0;
                for (int i = 0; i < n; i++) {
                    const double a = s.Z(i, j);
                    ss = ss + a * a;
                    if (fabs(a) > big) { big = fabs(a); ib = i; }
                }
                double f = 1.0 / sqrt(ss);
                if (s.Z(ib, j) < 0) f = -f;
                for (int i = 0; i < n; i++) s.Z(i, j) = s.Z(i, j) * f;
            }
            for (int j = 0; j < n; j++)
                if (!(s.V(VD + j) > 0.0)) flags |= RAFTX_MODAL_NONPOSITIVE;
        }
    }
    if (flags & ~RAFTX_MODAL_SMALL_DIAG) {
        const double nan = __builtin_nan("");
        for (int i = 0; i < n; i++) fn[i] = nan;
        for (int i = 0; i < n * n; i++) modes[i] = nan;
        return flags;
    }
    // ---- the reference's DOF order: row i (N-1 .. 0) claims the unclaimed column of largest |v[i, :]|
    typename ModalMask<(N > 32)>::type claimed = 0;
    const typename ModalMask<(N > 32)>::type one = 1;
    for (int i = n - 1; i >= 0; i--) {
        int best = -1;
        double bv = -1.0;
        for (int j = 0; j < n; j++) {
            if (claimed & (one << j)) continue;
            const double a = fabs(s.Z(i, j));
            if (a > bv) { bv = a; best = j; }
        }
        claimed |= one << best;
        fn[i] = sqrt(s.V(VD + best)) / 2.0 / 3.141592653589793;
        for (int r2 = 0; r2 < n; r2++) modes[r2 * n + i] = s.Z(r2, best);
    }
    return flags;
}

// The rigid unit's instance, what k_modal runs.
template <class S>
RAFTX_MODAL_HD inline int modal_core(S &s, double *fn, double *modes) { return modal_core_n<MODAL_N>(s, fn, modes); }

#ifdef __HIPCC__
// Storage of one lane's system in the block's LDS: word e of lane t at sm[e * BS + t].
template <int BS>
struct ModalLds {
    double *sm;
    int lane;
    __device__ double &H(int i, int j) { return sm[(i * MODAL_N + j) * BS + lane]; }
    __device__ double &Z(int i, int j) { return sm[(36 + i * MODAL_N + j) * BS + lane]; }
    __device__ double &V(int k) { return sm[(72 + k) * BS + lane]; }
};

struct ModalArgs {
    int n;                               // systems
    const double *M, *C;                 // [n,36]: M_tot, C_tot (or the resident M0, C0)
    const double *dM, *dC;               // [n,36] added to M, C, or null
    const double *props_in;              // [n,RAFTX_SP_N] copied to props_out, or null
    double *props_out;
    double *fn, *modes;                  // [n,6], [n,36]
    int32_t *flags;                      // [n]
};

#define MODAL_BS 32
// One system per lane, MODAL_BS lanes per workgroup.  The block's matrices are contiguous: read coalesced into the
// [entry][lane] layout (M into Z, C into H), each sum in the order M + dM.
__global__ void __launch_bounds__(MODAL_BS) k_modal(ModalArgs A) {
    __shared__ double sm[MODAL_NE * MODAL_BS];
    const int t = threadIdx.x;
    const size_t s0 = (size_t)blockIdx.x * MODAL_BS;
    const int nb = (int)(((size_t)A.n - s0) < (size_t)MODAL_BS ? (size_t)A.n - s0 : (size_t)MODAL_BS);
    for (int k = t; k < nb * 36; k += MODAL_BS) {
        const int l = k / 36, e = k - l * 36;
        const size_t g = s0 * 36 + (size_t)k;
        double m = A.M[g], c = A.C[g];
        if (A.dM) m = m + A.dM[g];
        if (A.dC) c = c + A.dC[g];
        sm[(36 + e) * MODAL_BS + l] = m;
        sm[e * MODAL_BS + l] = c;
    }
    if (A.props_in)
        for (int k = t; k < nb * RAFTX_SP_N; k += MODAL_BS) A.props_out[s0 * RAFTX_SP_N + k] = A.props_in[s0 * RAFTX_SP_N + k];
    __syncthreads();
    if (t >= nb) return;
    ModalLds<MODAL_BS> s{sm, t};
    const size_t d = s0 + (size_t)t;
    A.flags[d] = modal_core(s, A.fn + d * 6, A.modes + d * 36);
}
#endif
