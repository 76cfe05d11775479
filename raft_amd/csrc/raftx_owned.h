// Owners of the HIP resources of a context: device blocks (DevPool + Bag; the arrays of one call: Staging; outside the pool:
// DevBuf), page-locked landing areas (Pinned), events, streams.  Host only -- the HIP runtime API and the standard library,
// so that a plain host compiler builds it (tests/csrc/owned_driver.cpp).  Every owner is non-copyable, movable where the
// library moves it, and releases what it holds when destroyed; the allocation, free, create and destroy calls are spelled
// here and nowhere else.  Owners never synchronise: what has to drain before a block is replaced or goes back to the pool
// is its caller's rule.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cassert>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <unordered_map>
#include <utility>
#include <vector>

struct NoCopy {                          // (the owners with move operations of their own are non-copyable by those)
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};

// Per-context device-memory pool: every call of the C-ABI needs a handful of device buffers (tables, results, scratch);
// hipMalloc / hipFree cost 0.1-1 ms each and hipFree synchronises the whole device, which serialises contexts that
// otherwise overlap copies and kernels on their own streams.  Blocks are rounded up (powers of two below 1 MiB, 1 MiB
// multiples above), cached on release and handed out again; everything goes back to the driver when the pool is destroyed.
// Callers return blocks only after their stream has drained.
struct DevPool : NoCopy {
    std::multimap<size_t, void *> free_;
    std::unordered_map<void *, size_t> size_;
    ~DevPool() { trim(); }
    static size_t round_up(size_t b) {
        if (b < 256) b = 256;
        if (b <= ((size_t)1 << 20)) {
            size_t p = 256;
            while (p < b) p <<= 1;
            return p;
        }
        return (b + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
    }
    hipError_t get(size_t bytes, void **out) {
        const size_t cap = round_up(bytes);
        auto it = free_.lower_bound(cap);
        if (it != free_.end() && it->first <= cap + cap / 2 + ((size_t)1 << 20)) {
            *out = it->second;
            free_.erase(it);
            return hipSuccess;
        }
        static const bool dbg = getenv("RAFTX_POOL_DEBUG") != nullptr;   // tuning: pool misses (they cost a hipMalloc) on stderr
        const auto t0 = std::chrono::steady_clock::now();
        hipError_t e = hipMalloc(out, cap);
        if (dbg)
            fprintf(stderr, "[raftx pool] miss: hipMalloc(%zu) %.3f ms (%zu blocks free)\n", cap,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), free_.size());
        if (e != hipSuccess) {                      // make room and retry once
            (void)hipGetLastError();
            trim();
            e = hipMalloc(out, cap);
        }
        if (e == hipSuccess) size_[*out] = cap;
        return e;
    }
    void put(void *p) {
        if (!p) return;
        auto it = size_.find(p);
        if (it == size_.end()) {                    // not one of mine (Bag::get_outside)
            (void)hipFree(p);
            return;
        }
        free_.emplace(it->second, p);
    }
    void trim() {
        for (auto &kv : free_) {
            size_.erase(kv.second);
            (void)hipFree(kv.second);
        }
        free_.clear();
    }
};

// Blocks taken together and given back together: the tables of a design upload, the temporaries of a build job, what a
// crossing keeps on the device, the scratch of one call.  The bag remembers the pool its blocks came from (the one of
// the ctx that fills it); release() puts every block back, and so do the destructor and an assignment over a full bag.
struct Bag {
    DevPool *pool = nullptr;
    std::vector<void *> blocks;
    Bag() = default;
    Bag(Bag &&o) noexcept : pool(o.pool), blocks(std::move(o.blocks)) { o.blocks.clear(); }
    Bag &operator=(Bag &&o) noexcept {              // releases the old blocks first
        if (this != &o) { release(); pool = o.pool; blocks = std::move(o.blocks); o.blocks.clear(); }
        return *this;
    }
    ~Bag() { release(); }
    void release() {
        for (void *p : blocks) pool->put(p);
        blocks.clear();
    }
    // a block of `from` for n elements; a zero count still gives a valid, never-read block
    template <typename Tp>
    hipError_t get(DevPool &from, size_t n, Tp **out) {
        void *p = nullptr;
        const hipError_t e = from.get((n ? n : 1) * sizeof(Tp), &p);
        *out = reinterpret_cast<Tp *>(keep(from, e, p));
        return e;
    }
    // a block of exactly `bytes` straight from the driver, outside the pool (the variant program's); the pool's put() frees it
    hipError_t get_outside(DevPool &from, size_t bytes, void **out) {
        void *p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes);
        *out = keep(from, e, p);
        return e;
    }
    void *keep(DevPool &from, hipError_t e, void *p) {
        if (e != hipSuccess) return nullptr;
        assert(blocks.empty() || pool == &from);   // one pool per filling: release() gives every block to `pool`
        pool = &from;
        blocks.push_back(p);
        return p;
    }
};

// The device side of one call's arrays, each declared once together with its host side: tmp(n) is a device-only block,
// in(host, n) a block plus a queued host-to-device copy of n elements, out(host, n) a block plus a queued device-to-host
// copy, out_from(host, dev, n) a queued copy out of a block somebody else owns.  A zero count, and a null host array of
// in / out, give null and queue nothing; a non-zero request the pool cannot meet gives null and sets `failed`, which stays
// set.  send() issues the uploads declared since the last send() -- none of them once `failed` is set --, fetch() the
// result copies, both in declaration order.
struct Staging {
    struct Copy { void *dst; const void *src; size_t bytes; };
    DevPool &pool;
    Bag bag;
    std::vector<Copy> ups, downs;
    bool failed = false;
    explicit Staging(DevPool &pool_) : pool(pool_) {}
    template <typename Tp>
    Tp *tmp(size_t n) {
        Tp *p = nullptr;
        if (n && bag.get(pool, n, &p) != hipSuccess) failed = true;
        return p;
    }
    template <typename Dp, typename Hp>
    Dp *in(const Hp *host, size_t n) {
        static_assert(sizeof(Dp) == sizeof(Hp), "host and device elements of one size");
        Dp *p = host ? tmp<Dp>(n) : nullptr;
        if (p) ups.push_back({p, host, n * sizeof(Dp)});
        return p;
    }
    template <typename Dp, typename Hp>
    Dp *out(Hp *host, size_t n) {
        Dp *p = host ? tmp<Dp>(n) : nullptr;
        out_from(host, p, n);
        return p;
    }
    template <typename Dp, typename Hp>
    void out_from(Hp *host, const Dp *dev, size_t n) {
        static_assert(sizeof(Dp) == sizeof(Hp), "host and device elements of one size");
        if (host && dev && n) downs.push_back({host, dev, n * sizeof(Dp)});
    }
    hipError_t send(hipStream_t st) {
        if (failed) ups.clear();
        return failed ? hipErrorOutOfMemory : issue(ups, hipMemcpyHostToDevice, st);
    }
    hipError_t fetch(hipStream_t st) { return issue(downs, hipMemcpyDeviceToHost, st); }
    static hipError_t issue(std::vector<Copy> &q, hipMemcpyKind kind, hipStream_t st) {
        hipError_t e = hipSuccess;
        for (size_t i = 0; i < q.size() && e == hipSuccess; i++) e = hipMemcpyAsync(q[i].dst, q[i].src, q[i].bytes, kind, st);
        q.clear();
        return e;
    }
};

// A device buffer outside the pool that only grows: p holds n elements (a zero count still has a valid block).
template <typename Tp>
struct DevBuf {
    Tp *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept {        // releases the old block first
        if (this != &o) { release(); p = std::exchange(o.p, nullptr); n = std::exchange(o.n, 0); }
        return *this;
    }
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    bool holds(size_t want) const { return p && n >= want; }
    // frees the block and allocates room for `want` elements (at least one); on failure: null and zero
    hipError_t grow(size_t want) {
        release();
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, (want ? want : 1) * sizeof(Tp));
        if (e != hipSuccess) return e;
        p = reinterpret_cast<Tp *>(q);
        n = want;
        return hipSuccess;
    }
    // allocated, and zeroed in the order of `stream`, the first time only
    hipError_t zeroed_once(size_t count, hipStream_t stream) {
        if (p) return hipSuccess;
        const hipError_t e = grow(count);
        return e != hipSuccess ? e : hipMemsetAsync(p, 0, count * sizeof(Tp), stream);
    }
};

// A page-locked landing area of a ctx, written by kernels and read by the host: grow-only -- reserve(n) keeps a block that
// holds n elements and replaces a smaller one (contents are not carried over; a zero count still gives a valid block).
template <typename Tp>
struct Pinned : NoCopy {
    Tp *p = nullptr;
    size_t cap = 0;                      // elements p was reserved for
    ~Pinned() { release(); }
    hipError_t reserve(size_t n) {
        if (p && cap >= n) return hipSuccess;
        release();
        void *q = nullptr;
        const hipError_t e = hipHostMalloc(&q, (n ? n : 1) * sizeof(Tp), hipHostMallocDefault);
        if (e != hipSuccess) return e;
        p = reinterpret_cast<Tp *>(q);
        cap = n;
        return hipSuccess;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

// An event: null until ensure() creates it, destroyed with its owner.  Reads as the handle.
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(std::exchange(o.e, nullptr)) {}
    Event &operator=(Event &&o) noexcept {          // destroys the old event first
        if (this != &o) { reset(); e = std::exchange(o.e, nullptr); }
        return *this;
    }
    ~Event() { reset(); }
    hipError_t ensure() { return e ? hipSuccess : hipEventCreate(&e); }                        // with timing
    hipError_t ensure(unsigned flags) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
    void reset() {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    operator hipEvent_t() const { return e; }
};

// A stream: null until ensure(flags) creates it -- in the highest priority class with ensure_highest -- or borrow() lends it
// another owner's (the block contexts of a crossing run on their parent's stream).  Only a stream it created is destroyed
// with it.  Reads as the handle.
struct Stream : NoCopy {
    hipStream_t s = nullptr;
    bool owned = false;
    ~Stream() { reset(); }
    hipError_t ensure(unsigned flags) { return s ? hipSuccess : created(hipStreamCreateWithFlags(&s, flags)); }
    // where the device has one priority class only, nothing is created and the stream stays null
    hipError_t ensure_highest(unsigned flags) {
        int least = 0, greatest = 0;
        if (s) return hipSuccess;
        const hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
        return (e != hipSuccess || least == greatest) ? e : created(hipStreamCreateWithPriority(&s, flags, greatest));
    }
    hipError_t created(hipError_t e) { owned = e == hipSuccess; return e; }
    void borrow(hipStream_t other) {                // destroys a stream of its own first
        reset();
        s = other;
    }
    void reset() {
        if (s && owned) (void)hipStreamDestroy(s);
        s = nullptr;
        owned = false;
    }
    operator hipStream_t() const { return s; }
};
