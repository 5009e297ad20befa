// tests/c/devmem_test.cpp -- oatk_amd/csrc/devmem.hpp (ChunkPool, DevBuf) on the CPU, against a stand-in for the driver (tests/test_host_devmem.py builds
// this with g++ under AddressSanitizer + UBSan, and the threaded case under ThreadSanitizer).
//
// The hip* entry points the header calls are defined HERE, over a ledger in host memory: hipMalloc'ed blocks are heap blocks of exactly their size (an access one
// byte outside is a sanitizer report), address ranges and pieces are numbers only.  The ledger knows which piece is mapped where and what may be touched, and
// keeps every call in order, so a test can ask what was zeroed, what was copied and what was waited for before a call returned.  Any one kind of call can be
// made to fail at its k-th use.
//   usage: devmem_test caps | keep | zero | fail | own | threads
#include "devmem.hpp"

#include <stdint.h>
#include <string.h>
#include <atomic>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <type_traits>

// ---- the stand-in driver ----
enum Kind { MALLOC, FREE, CREATE, RELEASE, RESERVE, MAP, UNMAP, ACCESS, MEMSET, MEMCPY, STREAM_SYNC, DEVICE_SYNC, N_KINDS };
static const char *const KIND_NAME[N_KINDS] = {"hipMalloc", "hipFree", "hipMemCreate", "hipMemRelease", "hipMemAddressReserve", "hipMemMap", "hipMemUnmap", "hipMemSetAccess",
                                               "hipMemsetAsync", "hipMemcpyAsync", "hipStreamSynchronize", "hipDeviceSynchronize"};
struct Ev { Kind kind; uintptr_t a, b; size_t n; };       // MALLOC/FREE: block, -, size; MAP: address, piece; MEMSET: address, value; MEMCPY: dst, src

struct Ledger {
    std::mutex mu;
    std::vector<Ev> log;
    std::map<uintptr_t, size_t> blocks;                   // live hipMalloc'ed blocks
    std::set<uintptr_t> pieces;                           // live pieces (their handles)
    std::map<uintptr_t, uintptr_t> mapped;                // address of a 64 MB slot -> the piece there
    std::set<uintptr_t> open;                             // slots hipMemSetAccess has opened
    std::vector<std::pair<uintptr_t, size_t>> ranges;     // reserved (never given back)
    uintptr_t next_va = (uintptr_t) 1 << 44, next_piece = 0x1000;
    size_t calls[N_KINDS] = {0};
    int fail_kind = -1;                                   // this kind of call fails ...
    size_t fail_at = 0;                                   // ... when calls[kind] reaches this
    std::vector<std::string> wrong;                       // what the driver itself objects to (an unmapped address written, a block freed twice, ...)

    bool step(Kind k) { return !(++calls[k] == fail_at && (int) k == fail_kind); }          // false: this call is the one that fails
    void arm(int kind, size_t k) { std::unique_lock<std::mutex> lk(mu); fail_kind = kind, fail_at = k; memset(calls, 0, sizeof(calls)); }
    // [a, a + n) lies in one live block
    bool in_block(uintptr_t a, size_t n) const
    {
        auto it = blocks.upper_bound(a);
        if (it == blocks.begin()) return false;
        --it;
        return a >= it->first && a + n <= it->first + it->second;
    }
    // [a, a + n) lies in a range, every slot of it mapped and open
    bool in_pieces(uintptr_t a, size_t n) const
    {
        for (uintptr_t s = a / DM_CHUNK * DM_CHUNK; s < a + n; s += DM_CHUNK) if (!mapped.count(s) || !open.count(s)) return false;
        return n > 0;
    }
    size_t count(Kind k, size_t from = 0) const { size_t c = 0; for (size_t i = from; i < log.size(); ++i) c += log[i].kind == k; return c; }
};
static Ledger *L;
static const hipStream_t ST = (hipStream_t) 0x51;
#define LOCK std::unique_lock<std::mutex> lk(L->mu)

extern "C" {
hipError_t hipMalloc(void **p, size_t n)
{
    LOCK;
    if (!L->step(MALLOC)) return hipErrorOutOfMemory;
    *p = malloc(n);
    L->blocks[(uintptr_t) *p] = n;
    L->log.push_back({MALLOC, (uintptr_t) *p, 0, n});
    return hipSuccess;
}
hipError_t hipFree(void *p)
{
    LOCK;
    auto it = L->blocks.find((uintptr_t) p);
    if (it == L->blocks.end()) { L->wrong.push_back("hipFree of no live block"); return hipErrorInvalidValue; }
    L->log.push_back({FREE, (uintptr_t) p, 0, it->second});
    L->blocks.erase(it);
    free(p);
    return hipSuccess;
}
hipError_t hipMemCreate(hipMemGenericAllocationHandle_t *h, size_t n, const hipMemAllocationProp *, unsigned long long)
{
    LOCK;
    if (n != DM_CHUNK) L->wrong.push_back("hipMemCreate of another size than a piece's");
    if (!L->step(CREATE)) return hipErrorOutOfMemory;
    const uintptr_t id = L->next_piece++;
    L->pieces.insert(id);
    *h = (hipMemGenericAllocationHandle_t) id;
    L->log.push_back({CREATE, id, 0, n});
    return hipSuccess;
}
hipError_t hipMemRelease(hipMemGenericAllocationHandle_t h)
{
    LOCK;
    for (auto &m : L->mapped) if (m.second == (uintptr_t) h) L->wrong.push_back("hipMemRelease of a mapped piece");
    if (!L->pieces.erase((uintptr_t) h)) L->wrong.push_back("hipMemRelease of no live piece");
    L->log.push_back({RELEASE, (uintptr_t) h, 0, DM_CHUNK});
    return hipSuccess;
}
hipError_t hipMemAddressReserve(void **p, size_t n, size_t, void *, unsigned long long)
{
    LOCK;
    if (n % DM_CHUNK) L->wrong.push_back("a range that is no multiple of a piece");
    if (!L->step(RESERVE)) return hipErrorOutOfMemory;
    *p = (void *) L->next_va;
    L->ranges.push_back({L->next_va, n});
    L->log.push_back({RESERVE, L->next_va, 0, n});
    L->next_va += n + DM_CHUNK;                           // (a gap: running off the end of a range hits nothing mapped)
    return hipSuccess;
}
hipError_t hipMemMap(void *p, size_t n, size_t, hipMemGenericAllocationHandle_t h, unsigned long long)
{
    LOCK;
    const uintptr_t a = (uintptr_t) p;
    bool inside = false;
    for (auto &r : L->ranges) inside |= a >= r.first && a + n <= r.first + r.second;
    if (!inside || n != DM_CHUNK || a % DM_CHUNK) L->wrong.push_back("hipMemMap outside a reserved range, or not of one slot");
    if (L->mapped.count(a)) L->wrong.push_back("hipMemMap over a mapped slot");
    for (auto &m : L->mapped) if (m.second == (uintptr_t) h) L->wrong.push_back("hipMemMap of a piece that is mapped elsewhere");
    if (!L->pieces.count((uintptr_t) h)) L->wrong.push_back("hipMemMap of no live piece");
    if (!L->step(MAP)) return hipErrorOutOfMemory;
    L->mapped[a] = (uintptr_t) h;
    L->log.push_back({MAP, a, (uintptr_t) h, n});
    return hipSuccess;
}
hipError_t hipMemUnmap(void *p, size_t n)
{
    LOCK;
    if (n != DM_CHUNK || !L->mapped.erase((uintptr_t) p)) L->wrong.push_back("hipMemUnmap of what is not a mapped slot");
    L->open.erase((uintptr_t) p);
    L->log.push_back({UNMAP, (uintptr_t) p, 0, n});
    return hipSuccess;
}
hipError_t hipMemSetAccess(void *p, size_t n, const hipMemAccessDesc *, size_t)
{
    LOCK;
    if (!n || n % DM_CHUNK) L->wrong.push_back("hipMemSetAccess of no whole slots");
    for (uintptr_t s = (uintptr_t) p; s < (uintptr_t) p + n; s += DM_CHUNK) if (!L->mapped.count(s)) L->wrong.push_back("hipMemSetAccess over an unmapped slot");
    if (!L->step(ACCESS)) return hipErrorInvalidValue;
    for (uintptr_t s = (uintptr_t) p; s < (uintptr_t) p + n; s += DM_CHUNK) L->open.insert(s);
    L->log.push_back({ACCESS, (uintptr_t) p, 0, n});
    return hipSuccess;
}
hipError_t hipMemsetAsync(void *p, int v, size_t n, hipStream_t)
{
    LOCK;
    if (L->in_block((uintptr_t) p, n)) memset(p, v, n);
    else if (!L->in_pieces((uintptr_t) p, n)) L->wrong.push_back("hipMemsetAsync over memory that is not there");
    L->log.push_back({MEMSET, (uintptr_t) p, (uintptr_t) v, n});
    return hipSuccess;
}
hipError_t hipMemset(void *p, int v, size_t n) { return hipMemsetAsync(p, v, n, nullptr); }
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind, hipStream_t)
{
    LOCK;
    const bool db = L->in_block((uintptr_t) d, n), sb = L->in_block((uintptr_t) s, n);
    if ((!db && !L->in_pieces((uintptr_t) d, n)) || (!sb && !L->in_pieces((uintptr_t) s, n))) L->wrong.push_back("hipMemcpyAsync over memory that is not there");
    if (!L->step(MEMCPY)) return hipErrorInvalidValue;
    if (db && sb) memcpy(d, s, n);
    L->log.push_back({MEMCPY, (uintptr_t) d, (uintptr_t) s, n});
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { LOCK; L->log.push_back({STREAM_SYNC, 0, 0, 0}); return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { LOCK; L->log.push_back({DEVICE_SYNC, 0, 0, 0}); return hipSuccess; }
hipError_t hipGetDevice(int *d) { *d = 0; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipMemGetInfo(size_t *fr, size_t *tot) { *fr = *tot = (size_t) 256 << 30; return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "stand-in error"; }
}

// ---- the tests ----
static int n_bad = 0;
static std::string where;
#define CHECK(cond) do { if (!(cond)) { ++n_bad; printf("FAILED %s: %s (line %d)\n", where.c_str(), #cond, __LINE__); } } while (0)

constexpr size_t MB = 1ull << 20, THR = 1 * MB, CH = 64 * MB;          // THR: OATK_DEBUG_POOL_MIN of this program (main)

// one scenario's world: a clean ledger and, on request, a pool for device 0 as oatk_hip_mem_pool makes it
struct World {
    Ledger led;
    ChunkPool *pool = nullptr;
    explicit World(bool with_pool)
    {
        L = &led;
        if (!with_pool) return;
        pool = new ChunkPool();
        pool->device = 0;
        memset(&pool->prop, 0, sizeof(pool->prop));
        memset(&pool->acc, 0, sizeof(pool->acc));
        pool->on = true;
        g_pool[0] = pool;
    }
    // every buffer is gone by now: what the library took from the driver has gone back, or lies idle in the pool
    void balance()
    {
        CHECK(led.blocks.empty());
        CHECK(led.mapped.empty());
        if (pool) { pool->end(); CHECK(led.pieces.size() == pool->ready.size()); pool->trim(); }
        CHECK(led.pieces.empty());
        for (auto &w : led.wrong) { ++n_bad; printf("FAILED %s: the driver saw %s\n", where.c_str(), w.c_str()); }
        led.wrong.clear();
    }
    ~World()
    {
        g_pool[0] = nullptr;
        if (pool) { pool->end(); delete pool; }
        for (auto &b : led.blocks) free((void *) b.first);             // (a failed case leaks into the ledger, not into the sanitizer's report)
        L = nullptr;
    }
};

struct Snap {
    void *p; size_t cap, va; std::vector<hipMemGenericAllocationHandle_t> ch; std::map<uintptr_t, uintptr_t> mapped; std::set<uintptr_t> open; std::map<uintptr_t, size_t> blocks;
    explicit Snap(const DevBuf &b) : p(b.p), cap(b.cap), va(b.va), ch(b.ch), mapped(L->mapped), open(L->open), blocks(L->blocks) {}
    bool same(const DevBuf &b) const { return b.p == p && b.cap == cap && b.va == va && b.ch == ch && L->mapped == mapped && L->open == open && L->blocks == blocks; }
};
static bool empty(const DevBuf &b) { return !b.p && !b.cap && !b.va && b.ch.empty() && L->blocks.empty() && L->mapped.empty(); }
// the buffer is what it says it is: a live block of cap bytes, or cap bytes of open pieces at p, its own, in order
static bool sound(const DevBuf &b)
{
    if (!b.va) return b.ch.empty() && (b.p? L->blocks.count((uintptr_t) b.p) && L->blocks[(uintptr_t) b.p] == b.cap : b.cap == 0);
    if (b.cap != b.ch.size() * CH || b.cap > b.va) return false;
    for (size_t i = 0; i < b.ch.size(); ++i) { const uintptr_t s = (uintptr_t) b.p + i * CH; if (!L->mapped.count(s) || L->mapped[s] != (uintptr_t) b.ch[i] || !L->open.count(s)) return false; }
    return L->mapped.size() == b.ch.size();
}

// Capacities: the numbers of the code before the three entry points had one growth routine, written out
static void test_caps()
{
    const size_t req[7] = {1, THR - 1, THR, CH - 1, CH, CH + 1, 200 * MB};
    const size_t ensure_malloc[7] = {257, 1179902, 1179904, 75497726, 75497728, 75497729, 235929856};                 // bytes + bytes / 8 + 256
    const size_t keep_malloc[7] = {257, 1310974, 1310976, 83886334, 83886336, 83886337, 262144256};                    // bytes + bytes / 4 + 256
    const size_t ensure_pieces[7] = {257, 1179902, 67108864, 134217728, 134217728, 134217728, 268435456};              // below the threshold as above; up(bytes + bytes / 16)
    const size_t keep_pieces[7] = {257, 1310974, 67108864, 67108864, 67108864, 134217728, 268435456};                  // up(bytes)
    for (int with_pool = 0; with_pool < 2; ++with_pool)
        for (int keep = 0; keep < 2; ++keep)
            for (int i = 0; i < 7; ++i) {
                where = std::string("caps ") + (with_pool? "pool " : "no pool ") + (keep? "grow_keep " : "ensure ") + std::to_string(req[i]);
                World w(with_pool != 0);
                {
                    DevBuf b;
                    CHECK(keep? b.grow_keep(req[i], 0, ST) : b.ensure(req[i], ST));
                    CHECK(b.cap == (with_pool? (keep? keep_pieces : ensure_pieces) : (keep? keep_malloc : ensure_malloc))[i]);
                    CHECK((b.va != 0) == (with_pool && req[i] >= THR));
                    CHECK(sound(b));
                    const Snap s(b);
                    CHECK((keep? b.grow_keep(b.cap, 0, ST) : b.ensure(b.cap, ST)) && s.same(b));                      // what fits asks the driver for nothing
                }
                w.balance();
            }
    {   // reserve: in pieces a range and nothing else, by vm_range's formula; otherwise grow_keep
        where = "caps reserve in pieces";
        World w(true);
        {
            DevBuf b;
            CHECK(b.reserve(100 * MB, 0, ST));
            CHECK(b.va == 805306368 && b.cap == 0 && b.ch.empty() && b.p == (void *) L->ranges[0].first);              // up(4 * up(100 MB) + 256 MB)
            CHECK(L->count(MAP) == 0 && L->count(CREATE) == 0 && L->count(MALLOC) == 0);
            CHECK(b.reserve(3ull << 30, 0, ST) && b.va == 6979321856);                                                 // up(3 GB + 1.5 GB + 2 GB)
            CHECK(b.grow_keep(70 * MB, 0, ST) && b.cap == 2 * CH && b.va == 6979321856 && sound(b));                   // the pieces come as the buffer fills, into the range
        }
        w.balance();
    }
    {
        where = "caps reserve without a pool";
        World v(false);
        {
            DevBuf b;
            CHECK(b.reserve(100 * MB, 0, ST) && b.cap == 131072256 && !b.va && sound(b));
            DevBuf c;
            CHECK(c.ensure(1000, ST) && c.reserve(THR, 0, ST) && c.cap == 1310976 && sound(c));
            CHECK(L->blocks.size() == 2);
        }
        v.balance();
    }
    {
        where = "caps reserve of a small block, with a pool";
        World u(true);
        {
            DevBuf b;
            CHECK(b.ensure(1000, ST) && !b.va && b.cap == 1381);
            CHECK(b.reserve(100 * MB, 500, ST) && b.va && b.cap == 2 * CH && sound(b));                                // a block that is there moves: grow_keep
        }
        u.balance();
    }
}

static void fill(void *p, size_t n, unsigned seed) { for (size_t i = 0; i < n; ++i) ((unsigned char *) p)[i] = (unsigned char) (seed + 131 * i + (i >> 8)); }
static bool filled(const void *p, size_t n, unsigned seed) { for (size_t i = 0; i < n; ++i) if (((const unsigned char *) p)[i] != (unsigned char) (seed + 131 * i + (i >> 8))) return false; return true; }
static size_t first_of(Kind k, size_t from = 0) { for (size_t i = from; i < L->log.size(); ++i) if (L->log[i].kind == k) return i; return (size_t) -1; }

static void test_keep()
{
    where = "keep block to block";
    {
        World w(false);
        {
            DevBuf b;
            CHECK(b.ensure(5000, ST));
            fill(b.p, b.cap, 7);
            const uintptr_t old = (uintptr_t) b.p;
            const size_t mark = L->log.size();
            CHECK(b.grow_keep(9000, 3000, ST) && b.cap == 11506 && (uintptr_t) b.p != old);
            CHECK(filled(b.p, 3000, 7));
            CHECK(L->count(MEMCPY, mark) == 1);
            const size_t m = first_of(MALLOC, mark), c = first_of(MEMCPY, mark), s = first_of(STREAM_SYNC, mark), f = first_of(FREE, mark);
            CHECK(m < c && c < s && s < f);                                                   // the new block first, the copy, the wait, and only then the old block goes
            CHECK(L->log[c].a == (uintptr_t) b.p && L->log[c].b == old && L->log[c].n == 3000);      // exactly `used` bytes, old to new
            CHECK(L->log[f].a == old);
        }
        w.balance();
    }
    where = "keep ensure frees first";
    {
        World w(false);
        {
            DevBuf b;
            CHECK(b.ensure(5000, ST));
            const size_t mark = L->log.size();
            CHECK(b.ensure(9000, ST) && b.cap == 10381);
            const size_t s = first_of(STREAM_SYNC, mark), f = first_of(FREE, mark), m = first_of(MALLOC, mark);
            CHECK(s < f && f < m && L->count(MEMCPY, mark) == 0);                             // after a wait the old block is freed BEFORE the new one is taken; nothing is copied
            CHECK(b.ensure(20000, ST, true) && L->log.back().kind == MEMSET && L->log.back().a == (uintptr_t) b.p && L->log.back().n == b.cap && L->log.back().b == 0);   // zero_new: all of it
        }
        w.balance();
    }
    where = "keep in pieces";
    {
        World w(true);
        {
            DevBuf b;
            CHECK(b.grow_keep(65 * MB, 0, ST) && b.cap == 2 * CH && b.va == 805306368);
            const void *p0 = b.p;
            const std::vector<hipMemGenericAllocationHandle_t> two = b.ch;
            CHECK(b.grow_keep(300 * MB, 65 * MB, ST) && b.p == p0 && b.cap == 5 * CH && b.va == 805306368);            // grown where it is
            CHECK(b.ensure(700 * MB, ST) && b.p == p0 && b.cap == 12 * CH && sound(b));                                // up(700 MB + a sixteenth) = the whole range
            CHECK(L->count(RESERVE) == 1 && L->count(UNMAP) == 0 && L->count(MEMCPY) == 0);
            const std::vector<hipMemGenericAllocationHandle_t> twelve = b.ch;
            CHECK(std::vector<hipMemGenericAllocationHandle_t>(twelve.begin(), twelve.begin() + 2) == two);
            const size_t mark = L->log.size();
            CHECK(b.grow_keep(900 * MB, 700 * MB, ST) && b.p != p0 && b.cap == 15 * CH && b.va == 4294967296);         // the range is outgrown: up(4 * 960 MB + 256 MB)
            CHECK(sound(b) && std::vector<hipMemGenericAllocationHandle_t>(b.ch.begin(), b.ch.begin() + 12) == twelve);  // the same pieces at the new range, in order
            CHECK(L->count(MEMCPY, mark) == 0 && L->count(UNMAP, mark) == 12 && L->count(RESERVE, mark) == 1);
            CHECK(first_of(STREAM_SYNC, mark) < first_of(UNMAP, mark) && first_of(DEVICE_SYNC, mark) < first_of(UNMAP, mark));
        }
        w.balance();
    }
    where = "keep block to pieces";
    {
        World w(true);
        {
            DevBuf b;
            CHECK(b.ensure(60000, ST) && !b.va);
            fill(b.p, 40000, 3);
            const uintptr_t old = (uintptr_t) b.p;
            const size_t mark = L->log.size();
            CHECK(b.grow_keep(2 * MB, 40000, ST) && b.va && b.cap == CH && sound(b) && L->blocks.empty());
            const size_t c = first_of(MEMCPY, mark), s = first_of(STREAM_SYNC, c), f = first_of(FREE, mark);
            CHECK(L->count(MEMCPY, mark) == 1 && L->log[c].a == (uintptr_t) b.p && L->log[c].b == old && L->log[c].n == 40000 && c < s && s < f);     // the one copy of its life
        }
        w.balance();
    }
    where = "keep block to pieces, ensure";
    {
        World v(true);
        {
            DevBuf b;
            CHECK(b.ensure(60000, ST) && !b.va);
            const size_t mark = L->log.size();
            CHECK(b.ensure(2 * MB, ST) && b.va && b.cap == CH && sound(b) && L->blocks.empty());
            CHECK(L->count(MEMCPY, mark) == 0 && first_of(STREAM_SYNC, mark) < first_of(FREE, mark) && first_of(FREE, mark) < first_of(RESERVE, mark));   // ensure frees the block
        }
        v.balance();
    }
}

static void test_zero()
{
    where = "zero";
    World w(true);
    {
        DevBuf a, b;
        CHECK(a.ensure(200 * MB, ST) && a.cap == 4 * CH);
        CHECK(L->count(MEMSET) == 0);                                                         // pieces fresh from the driver are zero: none is cleared again
        a.release();
        CHECK(L->mapped.empty() && w.pool->ready.size() == 4);
        size_t mark = L->log.size();
        CHECK(b.ensure(70 * MB, ST) && b.cap == 2 * CH && L->count(CREATE, mark) == 0);       // two pieces that served `a`
        CHECK(L->count(MEMSET, mark) == 1);
        size_t m = first_of(MEMSET, mark);
        CHECK(L->log[m].a == (uintptr_t) b.p && L->log[m].n == 2 * CH && L->log[m].b == 0 && first_of(STREAM_SYNC, m) != (size_t) -1);       // all of it, and waited for
        mark = L->log.size();
        CHECK(b.grow_keep(260 * MB, 70 * MB, ST) && b.cap == 5 * CH && L->count(CREATE, mark) == 1);      // two more of a's and one from the driver
        CHECK(L->count(MEMSET, mark) == 1);
        m = first_of(MEMSET, mark);
        CHECK(L->log[m].a == (uintptr_t) b.p + 2 * CH && L->log[m].n == 3 * CH && L->log[m].b == 0 && first_of(STREAM_SYNC, m) != (size_t) -1);    // exactly the new span: what it holds stays
        mark = L->log.size();
        CHECK(b.grow_keep(330 * MB, 260 * MB, ST) && b.cap == 6 * CH && L->count(MEMSET, mark) == 0);     // one fresh piece: nothing to clear
    }
    w.balance();
}

// Failure injection.  The rules, in all three entry points:
//   (a) a fresh buffer (no mapped piece, no block) that cannot get a range or a first piece becomes hipMalloc's for good, and the call goes on down that path;
//   (b) a buffer with pieces in place that cannot get another returns false, and what it had stays mapped and valid;
//   (c) a failed copy in the move from a block to pieces returns false with the buffer back on its old block (old p, old cap); the pieces go back to the pool.
struct Scenario {
    const char *name;
    bool with_pool;
    size_t bytes;
    std::function<void(DevBuf &)> setup;
    std::function<bool(DevBuf &)> op;
    size_t malloc_cap;                                    // what hipMalloc is asked for where the scenario ends on that path
    bool block;                                           // setup leaves a small block whose first USED bytes are filled
    char rule;                                            // which of the rules a failure of a range or a piece falls under here ('-': none, the outcome alone is checked)
};
static const Kind FALLIBLE[] = {MALLOC, CREATE, RESERVE, MEMCPY, MAP, ACCESS};

static void test_fail()
{
    const size_t USED = 40000;
    auto nothing = [](DevBuf &) {};
    auto small_block = [=](DevBuf &b) { if (!b.ensure(60000, ST)) abort(); fill(b.p, USED, 9); };
    auto one_piece = [](DevBuf &b) { if (!b.ensure(60 * MB, ST) || b.cap != CH) abort(); };
    const Scenario all[] = {
        {"fresh ensure", true, 200 * MB, nothing, [](DevBuf &b) { return b.ensure(200 * MB, ST); }, 200 * MB + 25 * MB + 256, false, 'a'},
        {"fresh grow_keep", true, 200 * MB, nothing, [](DevBuf &b) { return b.grow_keep(200 * MB, 0, ST); }, 200 * MB + 50 * MB + 256, false, 'a'},
        {"fresh reserve", true, 200 * MB, nothing, [](DevBuf &b) { return b.reserve(200 * MB, 0, ST); }, 200 * MB + 50 * MB + 256, false, 'a'},
        {"grow_keep from a small block to pieces", true, 200 * MB, small_block, [=](DevBuf &b) { return b.grow_keep(200 * MB, USED, ST); }, 200 * MB + 50 * MB + 256, true, 'c'},
        {"ensure of a buffer in pieces", true, 200 * MB, one_piece, [](DevBuf &b) { return b.ensure(200 * MB, ST); }, 0, false, 'b'},
        {"grow_keep of a buffer in pieces", true, 200 * MB, one_piece, [](DevBuf &b) { return b.grow_keep(200 * MB, 60 * MB, ST); }, 0, false, 'b'},
        {"fresh ensure, no pool", false, 3 * MB, nothing, [](DevBuf &b) { return b.ensure(3 * MB, ST); }, 0, false, '-'},
        {"fresh grow_keep, no pool", false, 3 * MB, nothing, [](DevBuf &b) { return b.grow_keep(3 * MB, 0, ST); }, 0, false, '-'},
        {"fresh reserve, no pool", false, 3 * MB, nothing, [](DevBuf &b) { return b.reserve(3 * MB, 0, ST); }, 0, false, '-'},
        {"grow_keep of a small block, no pool", false, 3 * MB, small_block, [=](DevBuf &b) { return b.grow_keep(3 * MB, USED, ST); }, 0, true, '-'},
    };
    for (const Scenario &sc : all) {
        size_t n_calls[N_KINDS];
        {   // without a failure: how many calls of each kind the scenario makes
            where = std::string("fail ") + sc.name + ", no failure";
            World w(sc.with_pool);
            {
                DevBuf b;
                sc.setup(b);
                L->arm(-1, 0);
                CHECK(sc.op(b) && (b.cap >= sc.bytes || (b.va >= sc.bytes && b.ch.empty())) && sound(b));
                memcpy(n_calls, L->calls, sizeof(n_calls));
                CHECK(L->count(UNMAP) == 0);                          // (no piece moves in these scenarios: every hipMemMap is of a newly taken piece)
                b.release();
            }
            w.balance();
        }
        size_t n_cases = 0;
        for (Kind kind : FALLIBLE)
            for (size_t k = 1; k <= n_calls[kind]; ++k, ++n_cases) {
                where = std::string("fail ") + sc.name + ": " + KIND_NAME[kind] + " number " + std::to_string(k);
                World w(sc.with_pool);
                {
                    DevBuf b;
                    sc.setup(b);
                    const Snap before(b);
                    L->arm(kind, k);
                    const bool ok = sc.op(b);
                    L->arm(-1, 0);
                    // the outcome is one of two
                    if (ok) CHECK((b.cap >= sc.bytes || (b.va >= sc.bytes && b.ch.empty() && !b.cap)) && sound(b));
                    else CHECK(empty(b) || before.same(b));
                    if (sc.block && !ok) CHECK(filled(b.p, USED, 9));
                    const bool of_pieces = kind == CREATE || kind == RESERVE || kind == MAP || kind == ACCESS;
                    if (sc.rule == 'a' && of_pieces) {                                        // rule (a)
                        CHECK(ok && !b.va && !b.pool && b.ch.empty() && L->mapped.empty() && L->blocks.size() == 1);
                        CHECK(b.cap == sc.malloc_cap);                      // hipMalloc's, with that entry point's slack
                        CHECK(b.ensure(400 * MB, ST) && !b.va && b.cap == 400 * MB + 50 * MB + 256 && L->count(RESERVE) <= 1);      // for good
                    }
                    if (sc.rule == 'b' && of_pieces) CHECK(!ok && before.same(b) && sound(b) && b.cap == CH);        // rule (b)
                    if (sc.rule == 'c' && kind == MEMCPY) {                                    // rule (c)
                        CHECK(!ok && before.same(b) && !b.va && L->mapped.empty() && filled(b.p, USED, 9));
                        CHECK(L->pieces.size() == 4 && w.pool->ready.size() == 4);
                        CHECK(b.grow_keep(200 * MB, USED, ST) && b.va && b.cap == 4 * CH && L->blocks.empty());      // and the next attempt makes the move
                    }
                    if (sc.rule == 'c' && of_pieces) CHECK(ok && !b.va && b.cap == sc.malloc_cap && filled(b.p, USED, 9) && L->blocks.size() == 1 && L->mapped.empty());
                    b.release();
                }
                w.balance();
            }
        CHECK(n_cases >= 1);
        printf("%s: %zu failures injected\n", sc.name, n_cases);
    }
}

static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "a DevBuf owns its memory: no copies");
static_assert(!std::is_move_constructible<DevBuf>::value && !std::is_move_assignable<DevBuf>::value, "a DevBuf owns its memory: no moves");
static void test_own()
{
    where = "own";
    World w(true);
    {
        struct State { DevBuf small, big, many[3]; };
        State *s = new State();
        CHECK(s->small.ensure(1000, ST) && s->big.ensure(100 * MB, ST) && s->many[1].grow_keep(5000, 0, ST) && s->many[2].reserve(80 * MB, 0, ST));
        CHECK(L->blocks.size() == 2 && L->mapped.size() == 2);
        delete s;                                                     // no list of its members anywhere
        CHECK(L->blocks.empty() && L->mapped.empty() && w.pool->ready.size() == 2);
        CHECK(L->log.back().kind == UNMAP || L->log.back().kind == FREE);
    }
    w.balance();
}

static void test_threads()
{
    where = "threads";
    World w(true);
    std::vector<std::thread> th;
    std::atomic<int> bad{0};
    for (int t = 0; t < 8; ++t)
        th.emplace_back([t, &bad] {
            unsigned x = 12345u + 977u * (unsigned) t;
            for (int i = 0; i < 100; ++i) {
                x = x * 1664525u + 1013904223u;
                const size_t first = i % 3 == 0? 1000 + (x >> 12) % 200000 : THR + (x >> 8) % (100 * MB);             // a block, or pieces
                DevBuf b;
                if (!b.ensure(first, ST) || b.cap < first) ++bad;
                if (!b.va) memset(b.p, t, 512);
                if (!b.grow_keep(2 * first + THR, b.va? first : 512, ST) || !b.va || b.cap < 2 * first + THR) ++bad;
                if (i % 7 == 0) b.release();
            }                                                         // the others drop theirs here
        });
    for (int i = 0; i < 20; ++i) { w.pool->warm(512 * MB); std::this_thread::yield(); }
    for (auto &t : th) t.join();
    w.pool->end();                                                    // (the thread that warms writes to the ledger as long as it runs)
    CHECK(bad == 0);
    CHECK(L->count(MAP) >= 800);
    w.balance();
}

int main(int argc, char **argv)
{
    setenv("OATK_DEBUG_POOL_MIN", "1048576", 1);                      // THR
    (void) &pools_end;                                                // (oatk_hip_mem_pool's, which is not part of the header)
    const std::string what = argc > 1? argv[1] : "";
    if (what == "caps") test_caps();
    else if (what == "keep") test_keep();
    else if (what == "zero") test_zero();
    else if (what == "fail") test_fail();
    else if (what == "own") test_own();
    else if (what == "threads") test_threads();
    else { fprintf(stderr, "usage: devmem_test caps | keep | zero | fail | own | threads\n"); return 2; }
    if (n_bad) { printf("%d checks FAILED (%s)\n", n_bad, what.c_str()); return 1; }
    printf("ok: %s\n", what.c_str());
    return 0;
}
