// The layouts of raft_amd/csrc/raftx_landing.h under AddressSanitizer and UBSan, without a GPU: for every count each area is
// allocated with exactly `need` doubles on the heap, every region is filled with a pattern of its own through the layout and
// read back, so an undersized need or two overlapping regions is the sanitizer's or the pattern's to report.  The offsets
// are held to the formulas written out below -- not to anything the header computes -- and the need to the figure the
// areas were reserved with before the header existed.  Built and run by tests/test_landing.py; prints "OK <checks>".
#include "../../raft_amd/csrc/raftx_landing.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static long checks = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        checks++;                                                                    \
        if (!(cond)) {                                                               \
            fprintf(stderr, "FAILED %s:%d (%s): %s\n", __FILE__, __LINE__, what, #cond); \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

// a region as the driver expects it: where it starts (bytes from the base), the size of an element, how many
struct Region { const char *name; void *at; size_t byte_off, elem, count; };

// `need` doubles exactly, the regions filled and read back, the offsets, the order, the alignment and the bound
static void run_area(const char *what, size_t need, size_t parent_need, std::vector<Region> (*regions)(double *, const void *),
                     const void *layout) {
    double *base = static_cast<double *>(malloc(need * sizeof(double)));   // (need == 0: a block of no bytes, never dereferenced)
    CHECK(base != nullptr);
    std::vector<Region> R = regions(base, layout);
    CHECK(need <= parent_need);
    size_t end = 0;
    for (size_t r = 0; r < R.size(); r++) {
        const Region &g = R[r];
        CHECK(static_cast<char *>(g.at) == reinterpret_cast<char *>(base) + g.byte_off);
        CHECK(g.byte_off % g.elem == 0);                                     // aligned to its type (the base is 8-byte aligned)
        CHECK(g.byte_off >= end);                                            // in order and disjoint
        end = g.byte_off + g.elem * g.count;
    }
    CHECK(end <= need * sizeof(double));                                     // the last region ends within the need
    CHECK(need * sizeof(double) < end + sizeof(double));                     // ... and the need is that end, rounded up to a double
    for (size_t r = 0; r < R.size(); r++)
        for (size_t i = 0; i < R[r].count; i++) {
            if (R[r].elem == sizeof(double)) static_cast<double *>(R[r].at)[i] = (double)(r * 1000003 + i) + 0.5;
            else static_cast<int32_t *>(R[r].at)[i] = (int32_t)(r * 1000003 + i);
        }
    for (size_t r = 0; r < R.size(); r++)
        for (size_t i = 0; i < R[r].count; i++) {
            if (R[r].elem == sizeof(double)) CHECK(static_cast<double *>(R[r].at)[i] == (double)(r * 1000003 + i) + 0.5);
            else CHECK(static_cast<int32_t *>(R[r].at)[i] == (int32_t)(r * 1000003 + i));
        }
    free(base);
}

static const size_t D = sizeof(double), I = sizeof(int32_t);
static size_t cP, cN, cLine, cProp;       // the counts of the area under test (the region lists below are plain functions)

static std::vector<Region> stats_regions(double *b, const void *l) {
    const landing::Stats &L = *static_cast<const landing::Stats *>(l);
    return {{"sd", b + L.sd, 0, D, cP * 6}, {"niter", L.niter.in(b), 6 * cP * D, I, cP}, {"flags", L.flags.in(b), 6 * cP * D + cP * I, I, cP}};
}
static std::vector<Region> modal_regions(double *b, const void *l) {
    const landing::Modal &L = *static_cast<const landing::Modal *>(l);
    return {{"fn", b + L.fn, 0, D, cN * 6}, {"modes", b + L.modes, 6 * cN * D, D, cN * 36}, {"props", b + L.props, 42 * cN * D, D, cN * cProp},
            {"flags", L.flags.in(b), (42 + cProp) * cN * D, I, cN}};
}
static std::vector<Region> mooring_regions(double *b, const void *l) {
    const landing::Mooring &L = *static_cast<const landing::Mooring *>(l);
    const size_t nT = 2 * cLine;
    return {{"C", b + L.C, 0, D, cN * 36}, {"F", b + L.F, 36 * cN * D, D, cN * 6}, {"T", b + L.T, 42 * cN * D, D, cN * nT},
            {"flags", L.flags.in(b), (42 + nT) * cN * D, I, cN}};
}
static std::vector<Region> pose_regions(double *b, const void *l) {
    const landing::Pose &L = *static_cast<const landing::Pose *>(l);
    return {{"pose", b + L.pose, 0, D, cN * 6}, {"F_res", b + L.Fres, 6 * cN * D, D, cN * 6}, {"iterations", L.iterations.in(b), 12 * cN * D, I, cN},
            {"flags", L.flags.in(b), 12 * cN * D + cN * I, I, cN}};
}

int main() {
    const size_t counts[] = {0, 1, 2, 3, 7, 64, 65}, lines[] = {1, 3};
    const size_t SP_N = 12;                                                  // RAFTX_SP_N of include/raftx.h
    for (size_t n : counts) {
        cP = cN = n;
        cProp = SP_N;
        const landing::Stats S = landing::stats(n);
        run_area("statistics", S.need, 7 * n + 2, stats_regions, &S);
        const landing::Modal M = landing::modal(n, SP_N);
        run_area("eigen analysis", M.need, n * (42 + SP_N) + (n + 1) / 2, modal_regions, &M);
        for (size_t nLine : lines) {
            cLine = nLine;
            const landing::Mooring Q = landing::mooring(n, nLine);
            run_area("mooring", Q.need, n * (42 + 2 * nLine) + (n + 1) / 2 + 1, mooring_regions, &Q);
        }
        const landing::Pose P = landing::pose(n);
        run_area("pose", P.need, 13 * n + 2, pose_regions, &P);
    }
    printf("OK %ld\n", checks);
    return 0;
}
