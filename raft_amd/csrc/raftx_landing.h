// Where each result sits in the page-locked landing areas of a sweep crossing that hold more than one region.  A layout is
// a function of the area's counts: the offset of every region and the doubles the area needs, which is where its last
// region ends -- the kernel or copy that writes a region and the host code that reads it find it through one description.
// The offsets are counts, applied to a base pointer last: the need is known before the area exists.  Host-pure.
// A region of doubles is its offset in doubles (base + offset); a region of int32 is an Ints.
#pragma once
#include <cstddef>
#include <cstdint>

namespace landing {
struct Ints {                            // a region of int32, `dbl` doubles and `i32` ints behind the base (4-byte aligned)
    size_t dbl, i32;
    int32_t *in(double *base) const { return reinterpret_cast<int32_t *>(base + dbl) + i32; }
    const int32_t *in(const double *base) const { return reinterpret_cast<const int32_t *>(base + dbl) + i32; }
    size_t end(size_t count) const { return dbl + (i32 + count + 1) / 2; }   // doubles up to the end of `count` ints, rounded up
};
// every layout: the regions in order, then the doubles the area needs
struct Stats { size_t sd; Ints niter, flags; size_t need; };                // a block of P pairs: std [P,6] | niter [P] | flags [P]
struct Modal { size_t fn, modes, props; Ints flags; size_t need; };         // a block of n designs: fn [n,6] | modes [n,36] | props [n,nProp] | flags [n]
struct Mooring { size_t C, F, T; Ints flags; size_t need; };                // a crossing of n designs: C [n,36] | F [n,6] | T [n,2 nLine] | flags [n]
struct Pose { size_t pose, Fres; Ints iterations, flags; size_t need; };    // a crossing of n designs: pose, F_res [n,6] | iterations, flags [n]
template <class Layout>
Layout sized(Layout L, size_t nFlags) {  // each ends with its flags: the need is their end, typed nowhere else
    L.need = L.flags.end(nFlags);
    return L;
}
inline Stats stats(size_t P) { return sized(Stats{0, {P * 6, 0}, {P * 6, P}, 0}, P); }
inline Modal modal(size_t n, size_t nProp) { return sized(Modal{0, n * 6, n * 42, {n * (42 + nProp), 0}, 0}, n); }
inline Mooring mooring(size_t n, size_t nLine) { return sized(Mooring{0, n * 36, n * 42, {n * (42 + 2 * nLine), 0}, 0}, n); }
inline Pose pose(size_t n) { return sized(Pose{0, n * 6, {n * 12, 0}, {n * 12, n}, 0}, n); }
}   // namespace landing
