// Stand-alone host program for tests/test_array_modal.py: the serial eigen core of raft_amd/csrc/raftx_modal.h
// (modal_core_n<N>, N = 6 .. 36) and the wavefront schedule of raft_amd/csrc/raftx_array_modal.h (modal_wave<N>) with its
// lane loops run one lane after the other, both compiled by a plain host compiler with -ffp-contract=off.
//
//     array_modal_driver IN OUT
// IN:  int32 nSys, int32 N, then M [nSys,N,N] and C [nSys,N,N] as float64.
// OUT: float64, per schedule (serial core first, then the wave schedule) and system: fn [N], modes [N,N], flags.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define RAFTX_MODAL_HD
#include "../../include/raftx_modal.h"
#include "../../raft_amd/csrc/raftx_modal.h"
#include "../../raft_amd/csrc/raftx_array_modal.h"

template <int N>
struct HostSystem {
    std::vector<double> h, z, x, v;
    std::vector<int> p;
    HostSystem() : h(N * N), z(N * N), x(N * N), v(4 * N), p(N) {}
    double &H(int i, int j) { return h.at(i * N + j); }
    double &Z(int i, int j) { return z.at(i * N + j); }
    double &X(int i, int j) { return x.at(i * N + j); }
    double &V(int k) { return v.at(k); }
    int &P(int k) { return p.at(k); }
};

template <int N>
static void run(int nSys, const double *M, const double *C, std::vector<double> &out) {
    const size_t rec = N + N * N + 1;
    out.assign(2 * nSys * rec, 0.0);
    for (int wave = 0; wave < 2; wave++)
        for (int s = 0; s < nSys; s++) {
            HostSystem<N> sys;
            for (int k = 0; k < N * N; k++) {
                sys.z[k] = M[(size_t)s * N * N + k];
                sys.h[k] = C[(size_t)s * N * N + k];
            }
            double *o = out.data() + ((size_t)wave * nSys + s) * rec;
            o[N + N * N] = wave ? modal_wave<N>(sys, 0, o, o + N) : modal_core_n<N>(sys, o, o + N);
        }
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t hdr[2];
    if (fread(hdr, sizeof(int32_t), 2, f) != 2) { fprintf(stderr, "short header\n"); return 2; }
    const int nSys = hdr[0], N = hdr[1];
    if (nSys < 0 || nSys > 100000 || N < 6 || N > 36 || N % 6) { fprintf(stderr, "bad header %d %d\n", nSys, N); return 2; }
    const size_t nm = (size_t)nSys * N * N;
    std::vector<double> M(nm), C(nm), out;
    if (fread(M.data(), sizeof(double), nm, f) != nm || fread(C.data(), sizeof(double), nm, f) != nm) { fprintf(stderr, "short data\n"); return 2; }
    fclose(f);
    switch (N) {
    case 6: run<6>(nSys, M.data(), C.data(), out); break;
    case 12: run<12>(nSys, M.data(), C.data(), out); break;
    case 18: run<18>(nSys, M.data(), C.data(), out); break;
    case 24: run<24>(nSys, M.data(), C.data(), out); break;
    case 30: run<30>(nSys, M.data(), C.data(), out); break;
    default: run<36>(nSys, M.data(), C.data(), out); break;
    }
    FILE *g = fopen(argv[2], "wb");
    if (!g) { perror(argv[2]); return 2; }
    if (fwrite(out.data(), sizeof(double), out.size(), g) != out.size()) { fprintf(stderr, "short write\n"); return 2; }
    fclose(g);
    printf("OK %d %d\n", nSys, N);
    return 0;
}
