// raftx_array_modal.h -- eigen analysis of moored arrays: N = 6 nUnit <= 36 DOFs per system, one wavefront per system
// (included by raftx_hip.hip after raftx_modal.h; entry points in include/raftx_array_modal.h).
//
// The numerical method is modal_core_n<N> of raftx_modal.h, step for step: raft_model.py:436-547 with the array's
// coupled stiffness already summed into C.  What changes is who does the work.  One lane per system does not scale to
// N = 36 (H and Z alone are 20.7 KB per system), so the 64 lanes of one wavefront share one system:
//   * a loop of the serial core over j with i fixed (a row operation: the LU row updates, the Householder row pass, the
//     three-row update of a Francis step) is done by lane j;
//   * a loop over i with j fixed (a column operation: the Householder column pass, the three-column updates on H and Z,
//     Z <- Z T row by row, the normalisation per column) is done by lane i;
//   * a dot product is the serial sum of the lane that owns the column or row, in the serial core's order: there is no
//     cross-lane reduction anywhere, so every entry receives exactly the serial core's arithmetic (fp contract off) and
//     the results are the serial core's bits;
//   * scalars (the pivot choice, the balancing factors, the shifts, p / q / r, the deflation tests, the DOF claim) are
//     computed by every lane from the same LDS words, so all control flow is uniform over the workgroup;
//   * hqr2's back-substitution overwrites columns of H that other eigenvectors still read: with one lane per eigenvector
//     it writes into a third matrix X instead.
// Every hand-over of an LDS word from one lane to another is ordered by a barrier (ARRAY_MODAL_SYNC), also where the
// workgroup is one wavefront: nothing relies on lockstep.
//
// LDS: H, Z, X with a row pitch of N + 1 doubles (odd: lane-per-row reads of one column with ds_read_b64 hit distinct
// banks; a pitch of 36 would be a 4-way conflict), d | scale | ort [3 N] and the claimed columns [N] as int.  N = 36:
// 3 * 36 * 37 * 8 + 3 * 36 * 8 + 36 * 4 = 32 976 B, so the 160 KB of a CU hold four systems.  A workgroup is ONE
// wavefront with one system: the LDS budget, not the wave count, bounds the residency (four waves per CU, one per SIMD,
// whatever the grouping), so grouping waves would buy no occupancy, while a one-wave workgroup makes the many barriers of
// the Francis sweep as cheap as they get and makes a system's bits independent of its neighbours by construction.
//
// The same text compiles for the host with the lane loops run one lane after the other (ARRAY_MODAL_LANES): that is how
// tests/csrc/array_modal_driver.cpp checks this schedule against modal_core_n bit for bit without a GPU.
#pragma once

#if defined(__HIP_DEVICE_COMPILE__)
#define ARRAY_MODAL_LANES(t, lo, hi) if (const int t = lane; t >= (lo) && t < (hi))
#define ARRAY_MODAL_SYNC() __syncthreads()
#else
#define ARRAY_MODAL_LANES(t, lo, hi) for (int t = (lo); t < (hi); t++)
#define ARRAY_MODAL_SYNC() ((void)0)
#endif

// S: H(i, j), Z(i, j), X(i, j), V(k) [3 N], P(k) [N] (int) -- the workgroup's storage of its system.  On entry Z holds
// M_tot and H holds C_tot (written before a barrier).  Called by every lane of the workgroup with its lane number;
// lane t writes fn[t] and column t of modes.  Returns the RAFTX_MODAL_* flags, the same in every lane.
template <int N, class S>
RAFTX_MODAL_HD inline int modal_wave(S &s, const int lane, double *fn, double *modes) {
#pragma clang fp contract(off)
    const int n = N;
    const int VD = 0, VSC = N, VORT = 2 * N;
    const double eps = 2.220446049250313e-16;            // 2^-52
    int flags = 0;
    (void)lane;
    for (int i = 0; i < n; i++)
        if (s.Z(i, i) < 1.0 || s.H(i, i) < 1.0) flags |= RAFTX_MODAL_SMALL_DIAG;
    // ---- LU of M (in Z) with partial pivoting, applied to the N right-hand sides in H: lane j owns column j
    for (int k = 0; k < n; k++) {
        int p = k;
        double amax = fabs(s.Z(k, k));
        for (int i = k + 1; i < n; i++) {
            const double a = fabs(s.Z(i, k));
            if (a > amax) { amax = a; p = i; }
        }
        if (amax == 0.0) { flags |= RAFTX_MODAL_SINGULAR_M; break; }
        ARRAY_MODAL_SYNC();                               // the scan of column k is over before anything is written
        if (p != k) {
            ARRAY_MODAL_LANES(j, 0, n) {
                const double t = s.Z(k, j); s.Z(k, j) = s.Z(p, j); s.Z(p, j) = t;
                const double u = s.H(k, j); s.H(k, j) = s.H(p, j); s.H(p, j) = u;
            }
            ARRAY_MODAL_SYNC();
        }
        const double piv = s.Z(k, k);
        ARRAY_MODAL_LANES(i, k + 1, n) s.Z(i, k) = s.Z(i, k) / piv;
        ARRAY_MODAL_SYNC();
        ARRAY_MODAL_LANES(j, 0, n)
            for (int i = k + 1; i < n; i++) {
                const double l = s.Z(i, k);
                if (j > k) s.Z(i, j) = s.Z(i, j) - l * s.Z(k, j);
                s.H(i, j) = s.H(i, j) - l * s.H(k, j);
            }
        ARRAY_MODAL_SYNC();
    }
    if (!(flags & RAFTX_MODAL_SINGULAR_M)) {
        ARRAY_MODAL_LANES(j, 0, n)                        // back substitution: lane j solves its right-hand side
            for (int i = n - 1; i >= 0; i--) {
                double t = s.H(i, j);
                for (int k = i + 1; k < n; k++) t = t - s.Z(i, k) * s.H(k, j);
                s.H(i, j) = t / s.Z(i, i);
            }
        ARRAY_MODAL_LANES(i, 0, n) s.V(VSC + i) = 1.0;
        ARRAY_MODAL_SYNC();
        // ---- balancing: the sweep over i is sequential; row i is scaled by lane j at (i, j), column i at (j, i)
        for (int sweep = 0; sweep < 64; sweep++) {
            bool noconv = false;
            for (int i = 0; i < n; i++) {
                double c = 0.0, r = 0.0;
                for (int j = 0; j < n; j++)
                    if (j != i) { c = c + fabs(s.H(j, i)); r = r + fabs(s.H(i, j)); }
                ARRAY_MODAL_SYNC();                       // every lane has its sums before a lane scales
                if (c == 0.0 || r == 0.0) continue;
                double g = r / 2.0, f = 1.0;
                const double tot = c + r;
                while (c < g) { f = f * 2.0; c = c * 4.0; }
                g = r * 2.0;
                while (c >= g) { f = f / 2.0; c = c / 4.0; }
                if ((c + r) / f < 0.95 * tot) {
                    const double gi = 1.0 / f;
                    noconv = true;
                    ARRAY_MODAL_LANES(j, 0, n) {
                        if (j == i) s.V(VSC + i) = s.V(VSC + i) * f;
                        s.H(i, j) = s.H(i, j) * gi;
                        s.H(j, i) = s.H(j, i) * f;
                    }
                    ARRAY_MODAL_SYNC();
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
                    h = h + o * o;
                }
                double g = sqrt(h);
                const double om = s.H(m, m - 1) / scale;
                if (om > 0) g = -g;
                h = h - om * g;
                ARRAY_MODAL_LANES(i, m, n) {
                    const double o = s.H(i, m - 1) / scale;
                    s.V(VORT + i) = (i == m) ? o - g : o;
                }
                ARRAY_MODAL_SYNC();
                ARRAY_MODAL_LANES(j, m, n) {              // the row pass: lane j owns column j
                    double f = 0.0;
                    for (int i = n - 1; i >= m; i--) f = f + s.V(VORT + i) * s.H(i, j);
                    f = f / h;
                    for (int i = m; i < n; i++) s.H(i, j) = s.H(i, j) - f * s.V(VORT + i);
                }
                ARRAY_MODAL_SYNC();
                ARRAY_MODAL_LANES(i, 0, n) {              // the column pass: lane i owns row i
                    double f = 0.0;
                    for (int j = n - 1; j >= m; j--) f = f + s.V(VORT + j) * s.H(i, j);
                    f = f / h;
                    for (int j = m; j < n; j++) s.H(i, j) = s.H(i, j) - f * s.V(VORT + j);
                }
                ARRAY_MODAL_SYNC();
                ARRAY_MODAL_LANES(t, m, m + 1) {
                    (void)t;
                    s.V(VORT + m) = scale * s.V(VORT + m);
                    s.H(m, m - 1) = scale * g;
                }
                ARRAY_MODAL_SYNC();
            }
        }
        ARRAY_MODAL_LANES(i, 0, n)
            for (int j = 0; j < n; j++) s.Z(i, j) = (i == j) ? 1.0 : 0.0;
        ARRAY_MODAL_SYNC();
        for (int m = n - 2; m >= 1; m--) {
            if (s.H(m, m - 1) != 0.0) {
                ARRAY_MODAL_LANES(i, m + 1, n) s.V(VORT + i) = s.H(i, m - 1);
                ARRAY_MODAL_SYNC();
                ARRAY_MODAL_LANES(j, m, n) {
                    double g = 0.0;
                    for (int i = m; i < n; i++) g = g + s.V(VORT + i) * s.Z(i, j);
                    g = (g / s.V(VORT + m)) / s.H(m, m - 1);
                    for (int i = m; i < n; i++) s.Z(i, j) = s.Z(i, j) + g * s.V(VORT + i);
                }
                ARRAY_MODAL_SYNC();
            }
        }
        ARRAY_MODAL_LANES(i, 2, n)                        // the Householder vectors below the subdiagonal
            for (int j = 0; j < i - 1; j++) s.H(i, j) = 0.0;
        ARRAY_MODAL_SYNC();
        // ---- Francis double-shift QR on the Hessenberg form, transformations accumulated into Z
        double norm = 0.0;
        for (int i = 0; i < n; i++)
            for (int j = (i > 0 ? i - 1 : 0); j < n; j++) norm = norm + fabs(s.H(i, j));
        double exshift = 0.0, p = 0, q = 0, r = 0, sv = 0, z = 0, w, x, y;
        int iter = 0, total = 0;
        int nn = n - 1;
        while (nn >= 0) {                                 // every pass starts behind a barrier
            int l = nn;
            while (l > 0) {
                sv = fabs(s.H(l - 1, l - 1)) + fabs(s.H(l, l));
                if (sv == 0.0) sv = norm;
                if (fabs(s.H(l, l - 1)) < eps * sv) break;
                l--;
            }
            if (l == nn) {                                // one root
                const double hnn = s.H(nn, nn) + exshift;
                ARRAY_MODAL_SYNC();
                ARRAY_MODAL_LANES(t, 0, 1) {
                    (void)t;
                    s.H(nn, nn) = hnn;
                    s.V(VD + nn) = hnn;
                }
                ARRAY_MODAL_SYNC();
                nn--;
                iter = 0;
            } else if (l == nn - 1) {                     // two roots
                w = s.H(nn, nn - 1) * s.H(nn - 1, nn);
                p = (s.H(nn - 1, nn - 1) - s.H(nn, nn)) / 2.0;
                q = p * p + w;
                z = sqrt(fabs(q));
                const double hnn = s.H(nn, nn) + exshift, hmm = s.H(nn - 1, nn - 1) + exshift;
                const double sub = s.H(nn, nn - 1);
                x = hnn;
                ARRAY_MODAL_SYNC();
                if (q >= 0) {                             // a real pair: rotate it to triangular form
                    z = (p >= 0) ? p + z : p - z;
                    const double d0 = x + z;
                    double d1 = d0;
                    if (z != 0.0) d1 = x - w / z;
                    ARRAY_MODAL_LANES(t, 0, 1) {
                        (void)t;
                        s.H(nn, nn) = hnn;
                        s.H(nn - 1, nn - 1) = hmm;
                        s.V(VD + nn - 1) = d0;
                        s.V(VD + nn) = d1;
                    }
                    x = sub;
                    sv = fabs(x) + fabs(z);
                    p = x / sv;
                    q = z / sv;
                    r = sqrt(p * p + q * q);
                    p = p / r;
                    q = q / r;
                    ARRAY_MODAL_SYNC();
                    ARRAY_MODAL_LANES(j, nn - 1, n) {
                        const double zz = s.H(nn - 1, j);
                        s.H(nn - 1, j) = q * zz + p * s.H(nn, j);
                        s.H(nn, j) = q * s.H(nn, j) - p * zz;
                    }
                    ARRAY_MODAL_SYNC();
                    ARRAY_MODAL_LANES(i, 0, n) {
                        if (i <= nn) {
                            const double zz = s.H(i, nn - 1);
                            s.H(i, nn - 1) = q * zz + p * s.H(i, nn);
                            s.H(i, nn) = q * s.H(i, nn) - p * zz;
                        }
                        const double zz = s.Z(i, nn - 1);
                        s.Z(i, nn - 1) = q * zz + p * s.Z(i, nn);
                        s.Z(i, nn) = q * s.Z(i, nn) - p * zz;
                    }
                    ARRAY_MODAL_SYNC();
                } else {                                  // a complex pair
                    flags |= RAFTX_MODAL_COMPLEX;
                }
                nn -= 2;
                iter = 0;
            } else {                                      // no convergence yet: one more double-shift step
                if (++total > 30 * n) { flags |= RAFTX_MODAL_NO_CONVERGENCE; break; }
                x = s.H(nn, nn);
                y = s.H(nn - 1, nn - 1);
                w = s.H(nn, nn - 1) * s.H(nn - 1, nn);
                if (iter == 10) {                         // Wilkinson's exceptional shift
                    exshift += x;
                    ARRAY_MODAL_SYNC();
                    ARRAY_MODAL_LANES(i, 0, nn + 1) s.H(i, i) = s.H(i, i) - x;
                    ARRAY_MODAL_SYNC();
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
                        ARRAY_MODAL_SYNC();
                        ARRAY_MODAL_LANES(i, 0, nn + 1) s.H(i, i) = s.H(i, i) - sv;
                        ARRAY_MODAL_SYNC();
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
                ARRAY_MODAL_LANES(i, m + 2, nn + 1) {     // entries the search above does not read
                    s.H(i, i - 2) = 0.0;
                    if (i > m + 2) s.H(i, i - 3) = 0.0;
                }
                ARRAY_MODAL_SYNC();
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
                        bool sub = false;                 // H(k, k-1): column k-1, written behind the next barrier
                        double hsub = 0.0;
                        if (k != m) { sub = true; hsub = -sv * x; }
                        else if (l != m) { sub = true; hsub = -s.H(k, k - 1); }
                        p = p + sv;
                        x = p / sv;
                        y = q / sv;
                        z = r / sv;
                        q = q / p;
                        r = r / p;
                        ARRAY_MODAL_LANES(j, k, n) {      // rows k, k+1, k+2: lane j owns column j
                            double pp = s.H(k, j) + q * s.H(k + 1, j);
                            if (notlast) {
                                pp = pp + r * s.H(k + 2, j);
                                s.H(k + 2, j) = s.H(k + 2, j) - pp * z;
                            }
                            s.H(k, j) = s.H(k, j) - pp * x;
                            s.H(k + 1, j) = s.H(k + 1, j) - pp * y;
                        }
                        ARRAY_MODAL_SYNC();
                        const int ie = (nn < k + 3) ? nn : k + 3;
                        ARRAY_MODAL_LANES(i, 0, n) {      // columns k, k+1, k+2 of H and Z: lane i owns row i
                            if (i == 0 && sub) s.H(k, k - 1) = hsub;
                            if (i <= ie) {
                                double pp = x * s.H(i, k) + y * s.H(i, k + 1);
                                if (notlast) {
                                    pp = pp + z * s.H(i, k + 2);
                                    s.H(i, k + 2) = s.H(i, k + 2) - pp * r;
                                }
                                s.H(i, k) = s.H(i, k) - pp;
                                s.H(i, k + 1) = s.H(i, k + 1) - pp * q;
                            }
                            double pp = x * s.Z(i, k) + y * s.Z(i, k + 1);
                            if (notlast) {
                                pp = pp + z * s.Z(i, k + 2);
                                s.Z(i, k + 2) = s.Z(i, k + 2) - pp * r;
                            }
                            s.Z(i, k) = s.Z(i, k) - pp;
                            s.Z(i, k + 1) = s.Z(i, k + 1) - pp * q;
                        }
                        ARRAY_MODAL_SYNC();
                    }
                }
            }
        }
        if (!(flags & (RAFTX_MODAL_COMPLEX | RAFTX_MODAL_NO_CONVERGENCE))) {
            // ---- eigenvectors of the (now real upper triangular) Schur form into X, lane k its own; then back to A's basis
            if (norm != 0.0) {
                ARRAY_MODAL_LANES(k, 0, n) {
                    const double lam = s.V(VD + k);
                    s.X(k, k) = 1.0;
                    for (int i = k - 1; i >= 0; i--) {
                        const double wd = s.H(i, i) - lam;
                        double acc = 0.0;
                        for (int j = i + 1; j <= k; j++) acc = acc + s.H(i, j) * s.X(j, k);
                        const double v = (wd != 0.0) ? -acc / wd : -acc / (eps * norm);
                        s.X(i, k) = v;
                        const double t = fabs(v);
                        if ((eps * t) * t > 1)
                            for (int j = i; j <= k; j++) s.X(j, k) = s.X(j, k) / t;
                    }
                }
                ARRAY_MODAL_SYNC();
                ARRAY_MODAL_LANES(i, 0, n)
                    for (int j = n - 1; j >= 0; j--) {
                        double acc = 0.0;
                        for (int k = 0; k <= j; k++) acc = acc + s.Z(i, k) * s.X(k, j);
                        s.Z(i, j) = acc;
                    }
            }
            ARRAY_MODAL_LANES(i, 0, n) {                  // the balancing undone, unit 2-norm, the sign convention
                const double sc = s.V(VSC + i);
                for (int j = 0; j < n; j++) s.Z(i, j) = s.Z(i, j) * sc;
            }
            ARRAY_MODAL_SYNC();
            ARRAY_MODAL_LANES(j, 0, n) {
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
            ARRAY_MODAL_SYNC();
            for (int j = 0; j < n; j++)
                if (!(s.V(VD + j) > 0.0)) flags |= RAFTX_MODAL_NONPOSITIVE;
        }
    }
    if (flags & ~RAFTX_MODAL_SMALL_DIAG) {
        const double nan = __builtin_nan("");
        ARRAY_MODAL_LANES(t, 0, n) {
            fn[t] = nan;
            for (int i = 0; i < n; i++) modes[i * n + t] = nan;
        }
        return flags;
    }
    // ---- the reference's DOF order: row i (N-1 .. 0) claims the unclaimed column of largest |v[i, :]|
    unsigned long long claimed = 0;
    for (int i = n - 1; i >= 0; i--) {
        int best = -1;
        double bv = -1.0;
        for (int j = 0; j < n; j++) {
            if (claimed & (1ull << j)) continue;
            const double a = fabs(s.Z(i, j));
            if (a > bv) { bv = a; best = j; }
        }
        claimed |= 1ull << best;
        ARRAY_MODAL_LANES(t, i, i + 1) s.P(t) = best;
    }
    ARRAY_MODAL_SYNC();
    ARRAY_MODAL_LANES(t, 0, n) {                          // lane t: DOF t's frequency and mode, rows of modes coalesced
        const int b = s.P(t);
        fn[t] = sqrt(s.V(VD + b)) / 2.0 / 3.141592653589793;
        for (int r2 = 0; r2 < n; r2++) modes[r2 * n + t] = s.Z(r2, b);
    }
    return flags;
}

#ifdef __HIPCC__
// One system in the workgroup's LDS: H | Z | X with a row pitch of N + 1 doubles, then d | scale | ort, then the claim.
template <int N>
struct ArrayModalLds {
    enum { PITCH = N + 1, MAT = N * (N + 1), WORDS = 3 * N * (N + 1) + 3 * N + (N + 1) / 2 };
    double *sm;
    __device__ double &H(int i, int j) { return sm[i * PITCH + j]; }
    __device__ double &Z(int i, int j) { return sm[MAT + i * PITCH + j]; }
    __device__ double &X(int i, int j) { return sm[2 * MAT + i * PITCH + j]; }
    __device__ double &V(int k) { return sm[3 * MAT + k]; }
    __device__ int &P(int k) { return reinterpret_cast<int *>(sm + 3 * MAT + 3 * N)[k]; }
};

struct ArrayModalArgs {
    int n;                               // systems
    const double *M, *C;                 // [n,N,N]
    double *fn, *modes;                  // [n,N], [n,N,N]
    int32_t *flags;                      // [n]
    const int32_t *moor_flags;           // [n] or null: a system with any bit set is NaN and carries flags = 0
};

struct ArrayModalAssembleArgs {
    int nArray, nUnit;
    const double *M_unit, *K_unit;       // [nArray,nUnit,6,6]
    const double *C_moor;                // [nArray,n,n]: the array stiffness of the line kernels
    const double *dC;                    // [nArray,n,n] added last, or null
    double *M, *C;                       // [nArray,n,n]: blockdiag(M_unit), blockdiag(K_unit) + C_moor (+ dC)
};

// One entry of M_tot and C_tot per thread.
__global__ void __launch_bounds__(256) k_array_modal_assemble(ArrayModalAssembleArgs A) {
#pragma clang fp contract(off)
    const size_t n = (size_t)6 * A.nUnit, nn = n * n;
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= (size_t)A.nArray * nn) return;
    const size_t a = g / nn, e = g - a * nn, i = e / n, j = e - i * n;
    const size_t ui = i / 6, uj = j / 6;
    double m = 0.0, k = 0.0;
    if (ui == uj) {
        const size_t u = (a * A.nUnit + ui) * 36 + (i - ui * 6) * 6 + (j - uj * 6);
        m = A.M_unit[u];
        k = A.K_unit[u];
    }
    double c = k + A.C_moor[g];                          // (outside the blocks too: 0 + C_moor, the sum of the dense matrices)
    if (A.dC) c = c + A.dC[g];
    A.M[g] = m;
    A.C[g] = c;
}

// One system per workgroup of one wavefront; the grid is the batch.  The matrices are read with coalesced loads.
template <int N>
__global__ void __launch_bounds__(64) k_array_modal(ArrayModalArgs A) {
    __shared__ double sm[ArrayModalLds<N>::WORDS];
    const int t = threadIdx.x;
    const size_t d = blockIdx.x;
    ArrayModalLds<N> s{sm};
    if (A.moor_flags && A.moor_flags[d]) {               // (uniform over the workgroup)
        const double nan = __builtin_nan("");
        if (t < N) A.fn[d * N + t] = nan;
        for (int k = t; k < N * N; k += 64) A.modes[d * (N * N) + k] = nan;
        if (t == 0) A.flags[d] = 0;
        return;
    }
    for (int k = t; k < N * N; k += 64) {
        const int i = k / N, j = k - i * N;
        s.Z(i, j) = A.M[d * (N * N) + k];
        s.H(i, j) = A.C[d * (N * N) + k];
    }
    __syncthreads();
    const int fl = modal_wave<N>(s, t, A.fn + d * N, A.modes + d * (N * N));
    if (t == 0) A.flags[d] = fl;
}
#endif
