// The owners of raft_amd/csrc/raftx_owned.h under AddressSanitizer and UBSan, without a GPU and without the HIP runtime:
// this file defines the handful of HIP entry points the header calls, backed by malloc, counting live objects per kind and
// able to fail their k-th call.  A double free or a use after free is then the sanitizer's to report, a leak LeakSanitizer's
// and the counters'.  Built and run by tests/test_owned.py; prints "OK <checks>" when every check held.
#include "../../raft_amd/csrc/raftx_owned.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

enum Kind { DEV, HOST, EVENT, STREAM, NKIND };
static long live[NKIND], made[NKIND], freed[NKIND], calls[NKIND], fail_at[NKIND];   // fail_at: the call (1, 2, ..) that fails; 0: none
static bool fail_also_next[NKIND];                  // ... and the call after it (the pool retries a failed hipMalloc once)
static long memsets = 0;
struct Logged { hipMemcpyKind kind; void *dst; const void *src; size_t bytes; };
static std::vector<Logged> copies;                 // every hipMemcpyAsync, in the order issued

static hipError_t make(Kind k, void **out, size_t bytes, hipError_t err) {
    if (++calls[k] == fail_at[k] || (fail_also_next[k] && calls[k] == fail_at[k] + 1)) {
        *out = nullptr;
        return err;
    }
    *out = malloc(bytes ? bytes : 1);
    live[k]++;
    made[k]++;
    return hipSuccess;
}
static hipError_t drop(Kind k, void *p) {
    if (p) {
        live[k]--;
        freed[k]++;
    }
    free(p);
    return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void **ptr, size_t size) { return make(DEV, ptr, size, hipErrorOutOfMemory); }
hipError_t hipFree(void *ptr) { return drop(DEV, ptr); }
hipError_t hipHostMalloc(void **ptr, size_t size, unsigned int) { return make(HOST, ptr, size, hipErrorOutOfMemory); }
hipError_t hipHostFree(void *ptr) { return drop(HOST, ptr); }
hipError_t hipMemsetAsync(void *dst, int value, size_t sizeBytes, hipStream_t) {
    memsets++;
    memset(dst, value, sizeBytes);                  // (out of bounds: the sanitizer's to report)
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t sizeBytes, hipMemcpyKind kind, hipStream_t) {
    copies.push_back({kind, dst, src, sizeBytes});
    memcpy(dst, src, sizeBytes);                    // (out of bounds on either side: the sanitizer's to report)
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t *e) { return make(EVENT, reinterpret_cast<void **>(e), 1, hipErrorOutOfMemory); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return make(EVENT, reinterpret_cast<void **>(e), 1, hipErrorOutOfMemory); }
hipError_t hipEventDestroy(hipEvent_t e) { return drop(EVENT, e); }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned int) { return make(STREAM, reinterpret_cast<void **>(s), 1, hipErrorOutOfMemory); }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned int, int) { return make(STREAM, reinterpret_cast<void **>(s), 1, hipErrorOutOfMemory); }
hipError_t hipStreamDestroy(hipStream_t s) { return drop(STREAM, s); }
static int priority_classes = 3;
hipError_t hipDeviceGetStreamPriorityRange(int *least, int *greatest) {
    *least = 0;
    *greatest = -(priority_classes - 1);
    return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
}

static int checks = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        checks++;                                                                \
        if (!(cond)) {                                                           \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            exit(1);                                                             \
        }                                                                        \
    } while (0)
static void fresh() {
    for (int k = 0; k < NKIND; k++) {
        CHECK(live[k] == 0);                        // every scene leaves nothing behind
        made[k] = freed[k] = calls[k] = fail_at[k] = 0;
        fail_also_next[k] = false;
    }
    memsets = 0;
    copies.clear();
}

static void dev_buf() {
    {
        DevBuf<double> b;
        CHECK(b.grow(10) == hipSuccess && b.p && b.n == 10 && b.holds(10) && !b.holds(11));
        b.p[9] = 1.0;
        CHECK(b.grow(20) == hipSuccess && b.n == 20 && live[DEV] == 1);       // the old block went first
        CHECK(b.grow(0) == hipSuccess && b.p && b.n == 0 && live[DEV] == 1);   // a zero count still has a block
        fail_at[DEV] = calls[DEV] + 1;
        CHECK(b.grow(30) != hipSuccess && !b.p && b.n == 0 && live[DEV] == 0); // a failed growth: empty, nothing behind
        CHECK(b.grow(5) == hipSuccess && live[DEV] == 1);
    }
    fresh();
    {                                               // two in a row, the second failing: both end empty (ensure_xlio)
        DevBuf<int> a, b;
        fail_at[DEV] = 2;
        hipError_t e = a.grow(8);
        if (e == hipSuccess) e = b.grow(8);
        CHECK(e != hipSuccess && a.p && !b.p);
        a.release();
        b.release();
        CHECK(!a.p && !a.n && !b.p && !b.n && live[DEV] == 0);
    }
    fresh();
    {
        DevBuf<unsigned> z;
        CHECK(z.zeroed_once(16, nullptr) == hipSuccess && z.p[15] == 0 && memsets == 1);
        z.p[3] = 7;
        CHECK(z.zeroed_once(16, nullptr) == hipSuccess && z.p[3] == 7 && memsets == 1 && made[DEV] == 1);   // the first time only
        DevBuf<unsigned> y(std::move(z));
        CHECK(!z.p && !z.n && y.p && y.n == 16 && live[DEV] == 1);
        DevBuf<unsigned> x;
        CHECK(x.grow(4) == hipSuccess && live[DEV] == 2);
        x = std::move(y);                           // over a full owner: the old block is released first
        CHECK(live[DEV] == 1 && x.n == 16 && !y.p && freed[DEV] == 1);
    }
    CHECK(freed[DEV] == 2);                         // the moved-from owners released nothing
    fresh();
}

static void bags() {
    {
        DevPool pool;
        {
            Bag bag;
            double *a = nullptr, *z = nullptr;
            int *b = nullptr;
            CHECK(bag.get(pool, 100, &a) == hipSuccess && bag.get(pool, 3, &b) == hipSuccess && bag.get(pool, 0, &z) == hipSuccess);
            CHECK(a && b && z && live[DEV] == 3);   // a zero count still gives a block
            a[99] = 1.0;
            bag.release();
            CHECK(bag.blocks.empty() && live[DEV] == 3 && pool.free_.size() == 3);   // back in the pool, not freed
            CHECK(bag.get(pool, 100, &a) == hipSuccess && made[DEV] == 3);             // ... and handed out again
        }                                           // destroyed: the block goes back
        CHECK(pool.free_.size() == 3 && live[DEV] == 3);
        pool.trim();
        CHECK(live[DEV] == 0 && freed[DEV] == 3);   // each block freed once
        pool.trim();
        CHECK(freed[DEV] == 3);
    }
    fresh();
    {                                               // a block from outside the pool (the variant program's): freed once, by release
        DevPool pool;
        Bag bag;
        void *raw = nullptr;
        float *pooled = nullptr;
        CHECK(bag.get_outside(pool, 24, &raw) == hipSuccess && bag.get(pool, 6, &pooled) == hipSuccess && live[DEV] == 2);
        bag.release();
        CHECK(live[DEV] == 1 && freed[DEV] == 1 && pool.free_.size() == 1);
        fail_at[DEV] = calls[DEV] + 1;
        CHECK(bag.get_outside(pool, 24, &raw) != hipSuccess && !raw && bag.blocks.empty());
    }                                               // the pool's destructor trims
    CHECK(freed[DEV] == 2);
    fresh();
    {                                               // moves: the source releases nothing, an assignment releases the target's blocks first
        DevPool pool;
        Bag a, b;
        char *p = nullptr;
        CHECK(a.get(pool, 300, &p) == hipSuccess && b.get(pool, 5000, &p) == hipSuccess);
        Bag c(std::move(a));
        CHECK(a.blocks.empty() && c.blocks.size() == 1 && pool.free_.empty());
        b = std::move(c);
        CHECK(c.blocks.empty() && b.blocks.size() == 1 && pool.free_.size() == 1 && pool.free_.begin()->first == 8192);
        b = Bag();                                  // the reset-by-assignment idiom of the library
        CHECK(b.blocks.empty() && pool.free_.size() == 2 && live[DEV] == 2);
    }
    CHECK(freed[DEV] == 2);
    fresh();
    {                                               // the pool retries a failed allocation once, after a trim
        DevPool pool;
        Bag bag;
        double *p = nullptr;
        CHECK(bag.get(pool, 1000, &p) == hipSuccess);
        bag.release();
        fail_at[DEV] = calls[DEV] + 1;
        CHECK(bag.get(pool, 1 << 20, &p) == hipSuccess && live[DEV] == 1 && freed[DEV] == 1);
        fail_at[DEV] = calls[DEV] + 1;
        Bag other;
        CHECK(other.get(pool, 1 << 22, &p) == hipSuccess);
    }
    fresh();
}

static void pinned() {
    {
        Pinned<double> a;
        CHECK(a.reserve(0) == hipSuccess && a.p && live[HOST] == 1);
        CHECK(a.reserve(8) == hipSuccess && a.cap == 8 && live[HOST] == 1 && made[HOST] == 2);
        a.p[7] = 2.0;
        CHECK(a.reserve(4) == hipSuccess && made[HOST] == 2);                  // grow-only
        fail_at[HOST] = calls[HOST] + 1;
        CHECK(a.reserve(16) != hipSuccess && !a.p && a.cap == 0 && live[HOST] == 0);
        CHECK(a.reserve(16) == hipSuccess);
    }                                               // the destructor releases
    fresh();
}

static void events_and_streams() {
    {
        Event e;
        CHECK(!e && e.ensure(hipEventDisableTiming) == hipSuccess && e && e.ensure(hipEventDisableTiming) == hipSuccess && made[EVENT] == 1);   // twice creates once
        Event t;
        CHECK(t.ensure() == hipSuccess && made[EVENT] == 2);
        Event m(std::move(e));
        CHECK(!e && m && live[EVENT] == 2);
        t = std::move(m);                           // the old event is destroyed first
        CHECK(live[EVENT] == 1 && !m && t);
        std::vector<Event> many;
        for (int i = 0; i < 9; i++) {               // (the slab markers: a vector that reallocates moves its events)
            Event x;
            CHECK(x.ensure(hipEventDisableTiming) == hipSuccess);
            many.push_back(std::move(x));
        }
        CHECK(live[EVENT] == 10);
        Event f;
        fail_at[EVENT] = calls[EVENT] + 1;
        CHECK(f.ensure() != hipSuccess && !f);
    }
    CHECK(freed[EVENT] == made[EVENT]);
    fresh();
    {
        Stream own, high, flat;
        CHECK(!own && own.ensure(hipStreamNonBlocking) == hipSuccess && own.owned && own.ensure(hipStreamNonBlocking) == hipSuccess && made[STREAM] == 1);
        CHECK(high.ensure_highest(hipStreamNonBlocking) == hipSuccess && high && high.owned && made[STREAM] == 2);
        priority_classes = 1;                       // a device with one class: nothing is created
        CHECK(flat.ensure_highest(hipStreamNonBlocking) == hipSuccess && !flat && made[STREAM] == 2);
        priority_classes = 3;
        {
            Stream lent;                            // a block context: a stream of its own first, then its parent's
            CHECK(lent.ensure(hipStreamNonBlocking) == hipSuccess && live[STREAM] == 3);
            lent.borrow(own);
            CHECK(live[STREAM] == 2 && (hipStream_t)lent == (hipStream_t)own && !lent.owned);
        }
        CHECK(live[STREAM] == 2 && freed[STREAM] == 1);   // the borrowed stream was not destroyed
        Stream none;
        fail_at[STREAM] = calls[STREAM] + 1;
        CHECK(none.ensure(hipStreamNonBlocking) != hipSuccess && !none && !none.owned);
    }
    CHECK(freed[STREAM] == made[STREAM]);
    fresh();
}

// the arrays of one call (Staging): declared once with their host side, uploads by send, result copies by fetch alone
static bool copied(size_t i, hipMemcpyKind kind, void *dst, const void *src, size_t bytes) {
    return i < copies.size() && copies[i].kind == kind && copies[i].dst == dst && copies[i].src == src && copies[i].bytes == bytes;
}
static void staging() {
    {                                               // nothing to stage: null, no transfer, no failure, no block
        DevPool pool;
        Staging s(pool);
        double host[4] = {1, 2, 3, 4};
        const double *none = nullptr;
        double *nout = nullptr;
        CHECK(!s.tmp<double>(0) && !s.in<double>(none, 4) && !s.in<double>(host, 0) && !s.out<double>(nout, 4) && !s.out<double>(host, 0));
        s.out_from(nout, host, 4);
        s.out_from(host, none, 4);
        s.out_from(host, host, 0);
        CHECK(!s.failed && s.ups.empty() && s.downs.empty() && s.bag.blocks.empty() && calls[DEV] == 0);
        CHECK(s.send(nullptr) == hipSuccess && s.fetch(nullptr) == hipSuccess && copies.empty());
    }
    fresh();
    {                                               // declaration order, exact byte counts, results only by fetch, a round trip
        DevPool pool;
        {
            Staging s(pool);
            const double a[3] = {1.5, -2.5, 3.5};
            const int32_t b[5] = {7, 8, 9, 10, 11};
            const char cc[7] = "abcdef";
            double ra[3] = {0, 0, 0};
            int32_t rb[5] = {0, 0, 0, 0, 0};
            char rc[7] = "";
            double *da = s.in<double>(a, 3);
            float *scratch = s.tmp<float>(9);
            int *db = s.in<int>(b, 5);
            char *dc = s.in<char>(cc, 7);
            CHECK(da && scratch && db && dc && !s.failed && live[DEV] == 4 && copies.empty());     // declared, nothing issued
            s.out_from(rb, db, 5);
            s.out_from(ra, da, 3);
            s.out_from(rc, dc, 7);
            CHECK(s.send(nullptr) == hipSuccess && copies.size() == 3);
            CHECK(copied(0, hipMemcpyHostToDevice, da, a, 3 * sizeof(double)) && copied(1, hipMemcpyHostToDevice, db, b, 5 * sizeof(int32_t)) &&
                  copied(2, hipMemcpyHostToDevice, dc, cc, 7));
            CHECK(rb[0] == 0 && ra[0] == 0 && rc[0] == 0);                                          // no result copy yet
            CHECK(s.send(nullptr) == hipSuccess && copies.size() == 3);                             // sent once
            double later[2] = {4.0, 5.0};                                                            // declared after a send: the next send's
            double *dl = s.in<double>(later, 2);
            CHECK(s.send(nullptr) == hipSuccess && copies.size() == 4 && copied(3, hipMemcpyHostToDevice, dl, later, 2 * sizeof(double)));
            CHECK(s.fetch(nullptr) == hipSuccess && copies.size() == 7);
            CHECK(copied(4, hipMemcpyDeviceToHost, rb, db, 5 * sizeof(int32_t)) && copied(5, hipMemcpyDeviceToHost, ra, da, 3 * sizeof(double)) &&
                  copied(6, hipMemcpyDeviceToHost, rc, dc, 7));
            CHECK(!memcmp(ra, a, sizeof(a)) && !memcmp(rb, b, sizeof(b)) && !memcmp(rc, cc, sizeof(cc)));
            CHECK(s.fetch(nullptr) == hipSuccess && copies.size() == 7);
        }
        CHECK(pool.free_.size() == 5 && live[DEV] == 5);                                            // every block back in the pool
    }
    fresh();
    {                                               // out(): a block of its own, filled by "the kernel", copied by fetch
        DevPool pool;
        Staging s(pool);
        double res[4] = {9, 9, 9, 9};
        double *d = s.out<double>(res, 4);
        CHECK(d && s.downs.size() == 1 && s.ups.empty());
        for (int i = 0; i < 4; i++) d[i] = 0.25 * i;
        CHECK(s.send(nullptr) == hipSuccess && copies.empty() && res[3] == 9);
        CHECK(s.fetch(nullptr) == hipSuccess && copied(0, hipMemcpyDeviceToHost, res, d, 4 * sizeof(double)) && res[3] == 0.75);
    }
    fresh();
    {                                               // a result out of a block somebody else owns: read from that pointer
        DevPool pool;
        Staging s(pool);
        DevBuf<double> resident;
        CHECK(resident.grow(6) == hipSuccess);
        for (int i = 0; i < 6; i++) resident.p[i] = 10.0 + i;
        double res[6] = {0, 0, 0, 0, 0, 0};
        s.out_from(res, resident.p, 6);
        CHECK(s.bag.blocks.empty() && s.downs.size() == 1);
        CHECK(s.fetch(nullptr) == hipSuccess && copies.size() == 1 && copied(0, hipMemcpyDeviceToHost, res, resident.p, 6 * sizeof(double)));
        CHECK(res[0] == 10.0 && res[5] == 15.0);
    }
    fresh();
    for (int k : {1, 3, 5}) {                       // the k-th of five blocks refused: first, middle, last
        DevPool pool;
        {
            Staging s(pool);
            const double a[8] = {0};
            double r[8];
            void *p[5];
            for (int i = 1; i <= 5; i++) {
                if (i == k) {                       // (the pool tries twice: both attempts fail)
                    fail_at[DEV] = calls[DEV] + 1;
                    fail_also_next[DEV] = true;
                }
                p[i - 1] = i == 1 ? (void *)s.in<double>(a, 8) : i == 2 ? (void *)s.tmp<int>(100) : i == 3 ? (void *)s.out<double>(r, 8)
                         : i == 4 ? (void *)s.in<double>(a, 4) : (void *)s.out<double>(r, 2);
                CHECK((p[i - 1] == nullptr) == (i == k) && s.failed == (i >= k));                   // the flag stays set
            }
            CHECK(s.bag.blocks.size() == 4 && live[DEV] == 4 && !s.ups.empty() && !s.downs.empty());
            CHECK(s.send(nullptr) == hipErrorOutOfMemory && copies.empty() && s.ups.empty());       // a failed call uploads nothing
        }
        CHECK(pool.free_.size() == 4 && live[DEV] == 4);                                            // every block back in the pool
        pool.trim();
        CHECK(live[DEV] == 0);
        fresh();
    }
}

// the shape of a context: members declared pool first, released in the reverse order by the destructor alone
struct Holder {
    Stream stream;
    Event ev[3];
    DevPool pool;
    Bag bags[2];
    DevBuf<double> buf;
    Pinned<int> pin;
};
static void holder() {
    for (int fail = 0; fail <= 3; fail++) {         // also: creation stops part way, as in a failed raftx_ctx_create
        Holder *h = new Holder();
        fail_at[EVENT] = fail;
        bool ok = h->stream.ensure(hipStreamNonBlocking) == hipSuccess;
        for (Event &e : h->ev) ok = ok && e.ensure() == hipSuccess;
        CHECK(ok == (fail == 0));
        double *p = nullptr;
        if (ok) CHECK(h->bags[0].get(h->pool, 10, &p) == hipSuccess && h->bags[1].get(h->pool, 10, &p) == hipSuccess && h->buf.grow(4) == hipSuccess && h->pin.reserve(4) == hipSuccess);
        delete h;
        fresh();
    }
}

int main() {
    fresh();
    dev_buf();
    bags();
    pinned();
    events_and_streams();
    staging();
    holder();
    printf("OK %d\n", checks);
    return 0;
}
