// raftx_flex_modal.h -- eigen analysis of units with flexible members: n DOFs at run time, 6 <= n <= 256, one workgroup of
// 256 threads per system (included by raftx_hip.hip after raftx_array_modal.h; entry point in include/raftx_flex_modal.h).
//
// The numerical method is modal_core_n<N> of raftx_modal.h, step for step, up to and including the sign convention
// (raft_fowt.py:1705-1714 and raft_model.py:518-527 for nDOF != 6: eig(solve(M_tot, C_tot)), no DOF claim): an ascending
// stable order of the eigenvalues (ties by the QR's column index) takes the place of the DOF claim.  The schedule is the
// ownership rule of modal_wave<N> (raftx_array_modal.h) carried to up to 256 lanes:
//   * a loop of the serial core over j with i fixed is done by lane j, a loop over i with j fixed by lane i;
//   * a dot product is the serial sum of the owning lane in the serial order: no cross-lane reduction anywhere, fp contract
//     off, so every entry receives the serial core's arithmetic and the results are its bits;
//   * scalars (pivots, balancing factors, shifts, p / q / r, the deflation tests) are computed by every lane from the same
//     words, so all control flow is uniform over the workgroup;
//   * hqr2's back-substitution writes into a third matrix X, lane k its own eigenvector.
// Every hand-over of a word from one lane to another is ordered by a barrier (FLEX_MODAL_SYNC): nothing relies on lockstep.
// This text is a run-time-n twin of modal_wave<N>, which stays as it is; tests/csrc/flex_modal_driver.cpp pins the two (and
// modal_core_n) together bit for bit on the host, where the lane loops run one lane after the other.
//
// Storage.  Three n x n fp64 matrices are 540 KB at n = 150 and 1.38 MB at n = 240: they live in a global workspace PER
// WORKGROUP (the grid is min(nSys, FLEX_MODAL_WG_PER_CU per CU); a workgroup walks systems with a grid stride and reuses its
// workspace), with a pitch of n | 1 doubles.  The layouts follow the passes that dominate:
//   H   row-major: the row passes (LU updates, the Householder row pass, the three rows of a Francis step: lane j at (i, j))
//       are coalesced; the lane-per-row passes walk their own row, cache line by cache line
//   X   row-major: M_tot during the LU (lane j owns column j), later the eigenvectors of the Schur form, lane k at (j, k)
//   Z   COLUMN-major: the three-column update of a Francis step and Z <- Z X (lane i at (i, k)) are coalesced
// LDS holds d | scale | ort [3 n] and two int vectors (the order and the columns that are returned).
//
// Work whose results are not returned is skipped where the returned bits cannot depend on it: with nModes == 0 Z is never
// formed (H's arithmetic does not read Z); otherwise the back-substitution, Z <- Z X, the scaling and the normalisation run
// only for the nModes columns of the lowest eigenvalues (each column's arithmetic reads no other column's result).
#pragma once

#define FLEX_MODAL_THREADS 256
#define FLEX_MODAL_WG_PER_CU 2

#if defined(__HIP_DEVICE_COMPILE__)
#define FLEX_MODAL_LANES(t, lo, hi) if (const int t = lane; t >= (lo) && t < (hi))
#define FLEX_MODAL_SYNC() __syncthreads()
#else
#define FLEX_MODAL_LANES(t, lo, hi) for (int t = (lo); t < (hi); t++)
#define FLEX_MODAL_SYNC() ((void)0)
#endif

// S: H(i, j), Z(i, j), X(i, j), V(k) [3 n], P(k) [n] and W(k) [n] (int) -- the workgroup's storage of its system.  On entry
// X holds M_tot and H holds C_tot (written before a barrier).  Called by every lane of the workgroup with its lane number.
// fn [n] ascending; modes [n, nModes] row-major, column t the mode of fn[t].  Returns the RAFTX_MODAL_* flags, the same in
// every lane.
template <class S>
RAFTX_MODAL_HD inline int flex_modal_lanes(S &s, const int n, const int nModes, const int lane, double *fn, double *modes) {
#pragma clang fp contract(off)
    const int VD = 0, VSC = n, VORT = 2 * n;
    const double eps = 2.220446049250313e-16;            // 2^-52
    const bool wantZ = nModes > 0;
    int flags = 0;
    (void)lane;
    for (int i = 0; i < n; i++)
        if (s.X(i, i) < 1.0 || s.H(i, i) < 1.0) flags |= RAFTX_MODAL_SMALL_DIAG;
    // ---- LU of M (in X) with partial pivoting, applied to the n right-hand sides in H: lane j owns column j
    for (int k = 0; k < n; k++) {
        int p = k;
        double amax = fabs(s.X(k, k));
        for (int i = k + 1; i < n; i++) {
            const double a = fabs(s.X(i, k));
            if (a > amax) { amax = a; p = i; }
        }
        if (amax == 0.0) { flags |= RAFTX_MODAL_SINGULAR_M; break; }
        FLEX_MODAL_SYNC();                                // the scan of column k is over before anything is written
        if (p != k) {
            FLEX_MODAL_LANES(j, 0, n) {
                const double t = s.X(k, j); s.X(k, j) = s.X(p, j); s.X(p, j) = t;
                const double u = s.H(k, j); s.H(k, j) = s.H(p, j); s.H(p, j) = u;
            }
            FLEX_MODAL_SYNC();
        }
        const double piv = s.X(k, k);
        FLEX_MODAL_LANES(i, k + 1, n) s.X(i, k) = s.X(i, k) / piv;
        FLEX_MODAL_SYNC();
        FLEX_MODAL_LANES(j, 0, n) {
            const double xk = s.X(k, j), hk = s.H(k, j);
            for (int i = k + 1; i < n; i++) {
                const double l = s.X(i, k);
                if (j > k) s.X(i, j) = s.X(i, j) - l * xk;
                s.H(i, j) = s.H(i, j) - l * hk;
            }
        }
        FLEX_MODAL_SYNC();
    }
    if (!(flags & RAFTX_MODAL_SINGULAR_M)) {
        FLEX_MODAL_LANES(j, 0, n)                         // back substitution: lane j solves its right-hand side
            for (int i = n - 1; i >= 0; i--) {
                double t = s.H(i, j);
                for (int k = i + 1; k < n; k++) t = t - s.X(i, k) * s.H(k, j);
                s.H(i, j) = t / s.X(i, i);
            }
        FLEX_MODAL_LANES(i, 0, n) s.V(VSC + i) = 1.0;
        FLEX_MODAL_SYNC();
        // ---- balancing: the sweep over i is sequential; row i is scaled by lane j at (i, j), column i at (j, i)
        for (int sweep = 0; sweep < 64; sweep++) {
            bool noconv = false;
            for (int i = 0; i < n; i++) {
                double c = 0.0, r = 0.0;
                for (int j = 0; j < n; j++)
                    if (j != i) { c = c + fabs(s.H(j, i)); r = r + fabs(s.H(i, j)); }
                FLEX_MODAL_SYNC();                        // every lane has its sums before a lane scales
                if (c == 0.0 || r == 0.0) continue;
                double g = r / 2.0, f = 1.0;
                const double tot = c + r;
                while (c < g) { f = f * 2.0; c = c * 4.0; }
                g = r * 2.0;
                while (c >= g) { f = f / 2.0; c = c / 4.0; }
                if ((c + r) / f < 0.95 * tot) {
                    const double gi = 1.0 / f;
                    noconv = true;
                    FLEX_MODAL_LANES(j, 0, n) {
                        if (j == i) s.V(VSC + i) = s.V(VSC + i) * f;
                        s.H(i, j) = s.H(i, j) * gi;
                        s.H(j, i) = s.H(j, i) * f;
                    }
                    FLEX_MODAL_SYNC();
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
                FLEX_MODAL_LANES(i, m, n) {
                    const double o = s.H(i, m - 1) / scale;
                    s.V(VORT + i) = (i == m) ? o - g : o;
                }
                FLEX_MODAL_SYNC();
                FLEX_MODAL_LANES(j, m, n) {               // the row pass: lane j owns column j
                    double f = 0.0;
                    for (int i = n - 1; i >= m; i--) f = f + s.V(VORT + i) * s.H(i, j);
                    f = f / h;
                    for (int i = m; i < n; i++) s.H(i, j) = s.H(i, j) - f * s.V(VORT + i);
                }
                FLEX_MODAL_SYNC();
                FLEX_MODAL_LANES(i, 0, n) {               // the column pass: lane i owns row i
                    double f = 0.0;
                    for (int j = n - 1; j >= m; j--) f = f + s.V(VORT + j) * s.H(i, j);
                    f = f / h;
                    for (int j = m; j < n; j++) s.H(i, j) = s.H(i, j) - f * s.V(VORT + j);
                }
                FLEX_MODAL_SYNC();
                FLEX_MODAL_LANES(t, m, m + 1) {
                    (void)t;
                    s.V(VORT + m) = scale * s.V(VORT + m);
                    s.H(m, m - 1) = scale * g;
                }
                FLEX_MODAL_SYNC();
            }
        }
        if (wantZ) {
            FLEX_MODAL_LANES(i, 0, n)
                for (int j = 0; j < n; j++) s.Z(i, j) = (i == j) ? 1.0 : 0.0;
            FLEX_MODAL_SYNC();
            for (int m = n - 2; m >= 1; m--) {
                if (s.H(m, m - 1) != 0.0) {
                    FLEX_MODAL_LANES(i, m + 1, n) s.V(VORT + i) = s.H(i, m - 1);
                    FLEX_MODAL_SYNC();
                    FLEX_MODAL_LANES(j, m, n) {
                        double g = 0.0;
                        for (int i = m; i < n; i++) g = g + s.V(VORT + i) * s.Z(i, j);
                        g = (g / s.V(VORT + m)) / s.H(m, m - 1);
                        for (int i = m; i < n; i++) s.Z(i, j) = s.Z(i, j) + g * s.V(VORT + i);
                    }
                    FLEX_MODAL_SYNC();
                }
            }
        }
        FLEX_MODAL_LANES(i, 2, n)                         // the Householder vectors below the subdiagonal
            for (int j = 0; j < i - 1; j++) s.H(i, j) = 0.0;
        FLEX_MODAL_SYNC();
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
                FLEX_MODAL_SYNC();
                FLEX_MODAL_LANES(t, 0, 1) {
                    (void)t;
                    s.H(nn, nn) = hnn;
                    s.V(VD + nn) = hnn;
                }
                FLEX_MODAL_SYNC();
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
                FLEX_MODAL_SYNC();
                if (q >= 0) {                             // a real pair: rotate it to triangular form
                    z = (p >= 0) ? p + z : p - z;
                    const double d0 = x + z;
                    double d1 = d0;
                    if (z != 0.0) d1 = x - w / z;
                    FLEX_MODAL_LANES(t, 0, 1) {
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
                    FLEX_MODAL_SYNC();
                    FLEX_MODAL_LANES(j, nn - 1, n) {
                        const double zz = s.H(nn - 1, j);
                        s.H(nn - 1, j) = q * zz + p * s.H(nn, j);
                        s.H(nn, j) = q * s.H(nn, j) - p * zz;
                    }
                    FLEX_MODAL_SYNC();
                    FLEX_MODAL_LANES(i, 0, n) {
                        if (i <= nn) {
                            const double zz = s.H(i, nn - 1);
                            s.H(i, nn - 1) = q * zz + p * s.H(i, nn);
                            s.H(i, nn) = q * s.H(i, nn) - p * zz;
                        }
                        if (wantZ) {
                            const double zz = s.Z(i, nn - 1);
                            s.Z(i, nn - 1) = q * zz + p * s.Z(i, nn);
                            s.Z(i, nn) = q * s.Z(i, nn) - p * zz;
                        }
                    }
                    FLEX_MODAL_SYNC();
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
                    FLEX_MODAL_SYNC();
                    FLEX_MODAL_LANES(i, 0, nn + 1) s.H(i, i) = s.H(i, i) - x;
                    FLEX_MODAL_SYNC();
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
                        FLEX_MODAL_SYNC();
                        FLEX_MODAL_LANES(i, 0, nn + 1) s.H(i, i) = s.H(i, i) - sv;
                        FLEX_MODAL_SYNC();
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
                FLEX_MODAL_LANES(i, m + 2, nn + 1) {      // entries the searches above do not read
                    s.H(i, i - 2) = 0.0;
                    if (i > m + 2) s.H(i, i - 3) = 0.0;
                }
                FLEX_MODAL_SYNC();
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
                        FLEX_MODAL_LANES(j, k, n) {       // rows k, k+1, k+2: lane j owns column j
                            double pp = s.H(k, j) + q * s.H(k + 1, j);
                            if (notlast) {
                                pp = pp + r * s.H(k + 2, j);
                                s.H(k + 2, j) = s.H(k + 2, j) - pp * z;
                            }
                            s.H(k, j) = s.H(k, j) - pp * x;
                            s.H(k + 1, j) = s.H(k + 1, j) - pp * y;
                        }
                        FLEX_MODAL_SYNC();
                        const int ie = (nn < k + 3) ? nn : k + 3;
                        FLEX_MODAL_LANES(i, 0, n) {       // columns k, k+1, k+2 of H and Z: lane i owns row i
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
                            if (wantZ) {
                                double pp = x * s.Z(i, k) + y * s.Z(i, k + 1);
                                if (notlast) {
                                    pp = pp + z * s.Z(i, k + 2);
                                    s.Z(i, k + 2) = s.Z(i, k + 2) - pp * r;
                                }
                                s.Z(i, k) = s.Z(i, k) - pp;
                                s.Z(i, k + 1) = s.Z(i, k + 1) - pp * q;
                            }
                        }
                        FLEX_MODAL_SYNC();
                    }
                }
            }
        }
        if (!(flags & (RAFTX_MODAL_COMPLEX | RAFTX_MODAL_NO_CONVERGENCE))) {
            for (int j = 0; j < n; j++)
                if (!(s.V(VD + j) > 0.0)) flags |= RAFTX_MODAL_NONPOSITIVE;
        }
        if (!(flags & ~RAFTX_MODAL_SMALL_DIAG)) {
            // ---- the ascending stable order: lane k counts the eigenvalues ahead of its own (ties by column index)
            FLEX_MODAL_LANES(k, 0, n) {
                const double dk = s.V(VD + k);
                int rank = 0;
                for (int j = 0; j < n; j++) {
                    const double dj = s.V(VD + j);
                    if (dj < dk || (dj == dk && j < k)) rank++;
                }
                s.P(rank) = k;                            // rank -> column
                s.W(k) = rank < nModes;                   // column k is returned
            }
            FLEX_MODAL_SYNC();
            // ---- eigenvectors of the (now real upper triangular) Schur form into X, lane k its own; then back to A's basis
            if (wantZ && norm != 0.0) {
                FLEX_MODAL_LANES(k, 0, n) {
                    if (s.W(k)) {
                        const double lam = s.V(VD + k);
                        s.X(k, k) = 1.0;
                        for (int i = n - 2; i >= 0; i--) {   // (one i for all lanes at a time: row i of H is a broadcast)
                            if (i >= k) continue;
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
                }
                FLEX_MODAL_SYNC();
                FLEX_MODAL_LANES(i, 0, n)
                    for (int j = n - 1; j >= 0; j--) {
                        if (!s.W(j)) continue;
                        double acc = 0.0;
                        for (int k = 0; k <= j; k++) acc = acc + s.Z(i, k) * s.X(k, j);
                        s.Z(i, j) = acc;
                    }
            }
            if (wantZ) {
                FLEX_MODAL_LANES(i, 0, n) {               // the balancing undone, unit 2-norm, the sign convention
                    const double sc = s.V(VSC + i);
                    for (int j = 0; j < n; j++)
                        if (s.W(j)) s.Z(i, j) = s.Z(i, j) * sc;
                }
                FLEX_MODAL_SYNC();
                FLEX_MODAL_LANES(j, 0, n) {
                    if (s.W(j)) {
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
                }
                FLEX_MODAL_SYNC();
            }
        }
    }
    if (flags & ~RAFTX_MODAL_SMALL_DIAG) {
        const double nan = __builtin_nan("");
        FLEX_MODAL_LANES(t, 0, n) {
            fn[t] = nan;
            for (int j = 0; j < nModes; j++) modes[(size_t)t * nModes + j] = nan;
        }
        return flags;
    }
    FLEX_MODAL_LANES(t, 0, n) fn[t] = sqrt(s.V(VD + s.P(t))) / 2.0 / 3.141592653589793;
    FLEX_MODAL_LANES(i, 0, n)                             // lane i: row i of the returned modes
        for (int t = 0; t < nModes; t++) modes[(size_t)i * nModes + t] = s.Z(i, s.P(t));
    return flags;
}

#ifdef __HIPCC__
// The workgroup's storage: H | X row-major and Z column-major in its global workspace, the small vectors in LDS.
struct FlexModalStore {
    double *h, *x, *z, *v;
    int *pw;
    int n, pitch;
    __device__ double &H(int i, int j) { return h[(size_t)i * pitch + j]; }
    __device__ double &X(int i, int j) { return x[(size_t)i * pitch + j]; }
    __device__ double &Z(int i, int j) { return z[(size_t)j * pitch + i]; }
    __device__ double &V(int k) { return v[k]; }
    __device__ int &P(int k) { return pw[k]; }
    __device__ int &W(int k) { return pw[n + k]; }
};

struct FlexModalArgs {
    int nSys, n, nModes, pitch;
    const double *M, *C;                 // [nSys,n,n]
    double *fn, *modes;                  // [nSys,n], [nSys,n,nModes]
    int32_t *flags;                      // [nSys]
    double *work;                        // [grid, 3, n, pitch]
};

static inline int flex_modal_pitch(int n) { return n | 1; }

// One system at a time per workgroup, systems with a grid stride.  The matrices are read with coalesced loads.
__global__ void __launch_bounds__(FLEX_MODAL_THREADS) k_flex_modal(FlexModalArgs A) {
    __shared__ double sv[3 * RAFTX_FLEX_MODAL_MAX_N];
    __shared__ int sp[2 * RAFTX_FLEX_MODAL_MAX_N];
    const int t = threadIdx.x, n = A.n;
    const size_t mat = (size_t)n * A.pitch, nn = (size_t)n * n;
    double *w = A.work + (size_t)blockIdx.x * 3 * mat;
    FlexModalStore s{w, w + mat, w + 2 * mat, sv, sp, n, A.pitch};
    for (size_t d = blockIdx.x; d < (size_t)A.nSys; d += gridDim.x) {
        for (size_t k = t; k < nn; k += FLEX_MODAL_THREADS) {
            const int i = (int)(k / n), j = (int)(k - (size_t)i * n);
            s.X(i, j) = A.M[d * nn + k];
            s.H(i, j) = A.C[d * nn + k];
        }
        __syncthreads();
        const int fl = flex_modal_lanes(s, n, A.nModes, t, A.fn + d * n, A.modes + d * (size_t)n * A.nModes);
        if (t == 0) A.flags[d] = fl;
        __syncthreads();                                  // the workspace and the LDS vectors are free for the next system
    }
}
#endif
