// Stand-alone host program for tests/test_flex_modal.py, compiled by a plain host compiler with -ffp-contract=off.  Three
// variants of one eigen method:
//   (a) the serial core modal_core_n<N> of raft_amd/csrc/raftx_modal.h, N = 6, 12, 36 (DOF-claimed columns, all n modes);
//   (b) the same method for n at run time as serial code (tests/csrc/flex_modal_serial.h), ascending order;
//   (c) the lane schedule flex_modal_lanes of raft_amd/csrc/raftx_flex_modal.h, what k_flex_modal runs, with its lane loops run
//       one lane after the other, in the kernel's own storage layout (H, X row-major, Z column-major, pitch n | 1).
//
//     flex_modal_driver IN OUT
// IN:  int32 nSys, n, nModes, then M [nSys,n,n] and C [nSys,n,n] as float64.
// OUT: float64; (b) then (c), per system fn [n], modes [n,nModes], flags; then, for n = 6, 12, 36 only, (a): per system
//      fn [n], modes [n,n], flags.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define RAFTX_MODAL_HD
#include "../../include/raftx_flex_modal.h"
#include "../../raft_amd/csrc/raftx_modal.h"
#include "../../raft_amd/csrc/raftx_flex_modal.h"
#include "flex_modal_serial.h"

static void check(int i, int n) {
    if (i < 0 || i >= n) { fprintf(stderr, "index %d outside [0, %d)\n", i, n); abort(); }
}

struct SerialStore {                     // (a) and (b): H, Z row-major, V [4 n]
    int n;
    std::vector<double> h, z, v;
    explicit SerialStore(int n_) : n(n_), h((size_t)n_ * n_), z((size_t)n_ * n_), v(4 * (size_t)n_) {}
    double &H(int i, int j) { check(i, n); check(j, n); return h[(size_t)i * n + j]; }
    double &Z(int i, int j) { check(i, n); check(j, n); return z[(size_t)i * n + j]; }
    double &V(int k) { check(k, 4 * n); return v[k]; }
};

struct LaneStore {                       // (c): the layout of FlexModalStore
    int n, pitch;
    std::vector<double> h, x, z, v;
    std::vector<int> pw;
    explicit LaneStore(int n_) : n(n_), pitch(n_ | 1), h((size_t)n_ * pitch), x(h.size()), z(h.size()), v(3 * (size_t)n_), pw(2 * (size_t)n_) {}
    double &H(int i, int j) { check(i, n); check(j, n); return h[(size_t)i * pitch + j]; }
    double &X(int i, int j) { check(i, n); check(j, n); return x[(size_t)i * pitch + j]; }
    double &Z(int i, int j) { check(i, n); check(j, n); return z[(size_t)j * pitch + i]; }
    double &V(int k) { check(k, 3 * n); return v[k]; }
    int &P(int k) { check(k, n); return pw[k]; }
    int &W(int k) { check(k, n); return pw[n + k]; }
};

template <int N>
static void run_core(int nSys, const double *M, const double *C, double *o) {
    for (int s = 0; s < nSys; s++, o += N + N * N + 1) {
        SerialStore st(N);
        for (int k = 0; k < N * N; k++) {
            st.z[k] = M[(size_t)s * N * N + k];
            st.h[k] = C[(size_t)s * N * N + k];
        }
        o[N + N * N] = modal_core_n<N>(st, o, o + N);
    }
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t hdr[3];
    if (fread(hdr, sizeof(int32_t), 3, f) != 3) { fprintf(stderr, "short header\n"); return 2; }
    const int nSys = hdr[0], n = hdr[1], nModes = hdr[2];
    if (nSys < 0 || nSys > 100000 || n < 6 || n > RAFTX_FLEX_MODAL_MAX_N || nModes < 0 || nModes > n) {
        fprintf(stderr, "bad header %d %d %d\n", nSys, n, nModes);
        return 2;
    }
    const size_t nn = (size_t)n * n, nm = (size_t)nSys * nn;
    std::vector<double> M(nm), C(nm);
    if (fread(M.data(), sizeof(double), nm, f) != nm || fread(C.data(), sizeof(double), nm, f) != nm) { fprintf(stderr, "short data\n"); return 2; }
    fclose(f);
    const bool core = (n == 6 || n == 12 || n == 36);
    const size_t rec = (size_t)n + (size_t)n * nModes + 1, crec = (size_t)n + nn + 1;
    std::vector<double> out(2 * nSys * rec + (core ? nSys * crec : 0), 0.0);
    for (int s = 0; s < nSys; s++) {
        SerialStore st(n);
        for (size_t k = 0; k < nn; k++) {
            st.z[k] = M[s * nn + k];
            st.h[k] = C[s * nn + k];
        }
        double *o = out.data() + s * rec;
        o[rec - 1] = flex_modal_serial(st, n, nModes, o, o + n);
        LaneStore ls(n);
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) {
                ls.X(i, j) = M[s * nn + (size_t)i * n + j];
                ls.H(i, j) = C[s * nn + (size_t)i * n + j];
            }
        o = out.data() + ((size_t)nSys + s) * rec;
        o[rec - 1] = flex_modal_lanes(ls, n, nModes, 0, o, o + n);
    }
    double *oc = out.data() + 2 * (size_t)nSys * rec;
    if (n == 6) run_core<6>(nSys, M.data(), C.data(), oc);
    if (n == 12) run_core<12>(nSys, M.data(), C.data(), oc);
    if (n == 36) run_core<36>(nSys, M.data(), C.data(), oc);
    FILE *g = fopen(argv[2], "wb");
    if (!g) { perror(argv[2]); return 2; }
    if (fwrite(out.data(), sizeof(double), out.size(), g) != out.size()) { fprintf(stderr, "short write\n"); return 2; }
    fclose(g);
    printf("OK %d %d %d\n", nSys, n, nModes);
    return 0;
}
