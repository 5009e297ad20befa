// oatk_amd/csrc/devmem.hpp -- the device memory of the library: every hipMalloc / hipFree of csrc/ is in here, and so are the buffers in 64 MB pieces.
//
// Host code over the HIP host API and the standard library only (no kernels, nothing of common.hpp): tests/c/devmem_test.cpp compiles it with g++ against a
// stand-in for the driver and runs every path in it, the failures included.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>
#include <execinfo.h>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

namespace {

static bool env_flag(const char *name) { const char *e = getenv(name); return e && e[0] && e[0] != '0'; }
// OATK_DEBUG_ALLOC_LOG=1: every call into the driver for device memory on stderr, with its size and what it took (development aid)
static int dev_alloc_log()
{
    static const int on = env_flag("OATK_DEBUG_ALLOC_LOG");
    return on;
}
static double dev_now() { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return (double) t.tv_sec + 1e-9 * (double) t.tv_nsec; }

// ---- Device memory in pieces (oatk_hip_mem_pool, include/oatk_hip.h) ----
// What the driver does with device memory (tools/ubench/alloc_*.hip, profiles/r08l_alloc_rates.txt): memory nobody has had since the GPU was reset is cleared when it
// is handed out -- 30 ms per GB INSIDE hipMalloc / hipMemCreate --, memory a process gives back is cleared behind its back at ~33 GB/s, and the next call that wants
// memory (of any size, from any process) waits until that is done.  A process that takes 50 GB for its batch at once therefore stands still for up to 1.5 s on a
// fresh GPU, and one that gives a slab back and takes another stands still for the clearing of the first.  With a pool switched on the larger buffers of this process
// are address ranges backed by 64 MB pieces (hipMemAddressReserve / hipMemCreate / hipMemMap): a buffer grows by mapping more pieces where it is (no copy, no
// slack for growth), a buffer that is released hands its pieces to the next one (nothing goes back to the driver before the process ends), and a thread of the
// pool's own takes pieces from the driver AHEAD of the need -- beside the host's work on the reads, which is what a reader that fills structs is bound by.
constexpr size_t DM_CHUNK = 64ull << 20;          // a piece
static size_t dm_min()                             // buffers below this stay hipMalloc's (32 MB; OATK_DEBUG_POOL_MIN: tests put small buffers into pieces too)
{
    static const size_t v = [] { const char *e = getenv("OATK_DEBUG_POOL_MIN"); return e && atoll(e) > 0? (size_t) atoll(e) : (size_t) (32ull << 20); }();
    return v;
}
struct ChunkPool {
    int device = -1;
    bool on = false;
    std::mutex mu;
    std::condition_variable cv;
    std::vector<hipMemGenericAllocationHandle_t> ready;       // pieces nobody has mapped ...
    std::vector<char> used;                                   // ... and whether a buffer has had them (what the driver hands out is zero, and so is what a buffer gets: vm_grow)
    size_t created = 0, target = 0;                           // pieces taken from the driver so far; what the thread works towards
    bool warming = false, stop = false, failed = false;
    std::thread th;
    hipMemAllocationProp prop;
    hipMemAccessDesc acc;
    double t_wait = 0;                                        // seconds callers stood waiting for a piece

    bool create(hipMemGenericAllocationHandle_t *h)
    {
        const double t0 = dev_alloc_log()? dev_now() : 0;
        const hipError_t e = hipMemCreate(h, DM_CHUNK, &prop, 0);
        if (dev_alloc_log() && (e != hipSuccess || dev_now() - t0 > 0.01)) fprintf(stderr, "[oatk alloc] %.3f hipMemCreate %zu MB: %.4f s%s\n", dev_now(), DM_CHUNK >> 20, dev_now() - t0, e == hipSuccess? "" : " FAILED");
        if (e != hipSuccess) (void) hipGetLastError();
        return e == hipSuccess;
    }
    void run()
    {
        (void) hipSetDevice(device);
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu);
                if (stop || created >= target) { warming = false; cv.notify_all(); return; }
            }
            hipMemGenericAllocationHandle_t h;
            const bool ok = create(&h);
            std::unique_lock<std::mutex> lk(mu);
            if (!ok) { failed = true, warming = false; cv.notify_all(); return; }
            ready.push_back(h), used.push_back(0), ++created;
            cv.notify_all();
        }
    }
    void warm(size_t bytes)
    {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess && bytes > fr / 10 * 7) bytes = fr / 10 * 7;        // (never more than most of what is free now)
        std::unique_lock<std::mutex> lk(mu);
        const size_t want = created + bytes / DM_CHUNK;                        // on top of what the process holds already
        if (want > target) target = want;
        if (!warming && !failed && created < target) {
            if (th.joinable()) th.join();
            warming = true;
            th = std::thread([this] { run(); });
        }
    }
    bool take(hipMemGenericAllocationHandle_t *h, bool *was_used)
    {
        *was_used = false;
        {
            std::unique_lock<std::mutex> lk(mu);
            const double t0 = dev_now();
            for (;;) {
                if (!ready.empty()) { *h = ready.back(), *was_used = used.back() != 0; ready.pop_back(), used.pop_back(); t_wait += dev_now() - t0; return true; }
                if (warming && !failed && created < target) { cv.wait(lk); continue; }     // the thread is at it: two callers inside the driver would only take turns
                break;
            }
            t_wait += dev_now() - t0;
        }
        if (!create(h)) return false;
        std::unique_lock<std::mutex> lk(mu);
        ++created;
        return true;
    }
    void give(hipMemGenericAllocationHandle_t h)
    {
        std::unique_lock<std::mutex> lk(mu);
        ready.push_back(h), used.push_back(1);
    }
    // what nobody has mapped goes back to the driver (a hipMalloc failed: the pool must not be the reason)
    size_t trim()
    {
        std::unique_lock<std::mutex> lk(mu);
        const size_t n = ready.size();
        for (auto h : ready) (void) hipMemRelease(h);
        ready.clear(), used.clear();
        created -= n, target = created;
        return n;
    }
    void end()                                                 // at exit, before the runtime's own handlers: no thread of ours inside the driver when they run
    {
        { std::unique_lock<std::mutex> lk(mu); stop = true; cv.notify_all(); }
        if (th.joinable()) th.join();
    }
};
static std::atomic<ChunkPool *> g_pool[64];                    // by device; made by oatk_hip_mem_pool, never destroyed
static std::mutex g_pool_mu;
static void pools_end() { for (auto &p : g_pool) if (ChunkPool *q = p.load()) q->end(); }
static ChunkPool *pool_of_current_device()
{
    int d = -1;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return nullptr;
    ChunkPool *p = g_pool[d].load();
    return p && p->on? p : nullptr;
}
// (development aid) OATK_DEBUG_POOL_SEQ="lo:hi": only the lo-th .. (hi-1)-th decisions of a buffer to live in pieces are taken; the others stay hipMalloc's
static ChunkPool *pool_for_new_buffer()
{
    ChunkPool *p = pool_of_current_device();
    if (!p) return nullptr;
    struct Window { long lo = 0, hi = 1L << 60; Window() { const char *e = getenv("OATK_DEBUG_POOL_SEQ"); if (e) sscanf(e, "%ld:%ld", &lo, &hi); } };
    static const Window w;
    static std::atomic<long> seq{0};                           // handles decide on several threads
    const long k = seq++;
    if (dev_alloc_log()) {
        void *bt[6];
        const int nb = backtrace(bt, 6);
        char **sy = backtrace_symbols(bt, nb);
        fprintf(stderr, "[oatk alloc] decision %ld%s  <- %s <- %s <- %s\n", k, k >= w.lo && k < w.hi? "" : " (hipMalloc)", nb > 2? sy[2] : "", nb > 3? sy[3] : "", nb > 4? sy[4] : "");
        free(sy);
    }
    return k >= w.lo && k < w.hi? p : nullptr;
}

static hipError_t dev_malloc(void **p, size_t bytes)
{
    const double t0 = dev_alloc_log()? dev_now() : 0;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {
        ChunkPool *pl = pool_of_current_device();
        if (pl && pl->trim()) { (void) hipGetLastError(); e = hipMalloc(p, bytes); }
    }
    if (dev_alloc_log()) fprintf(stderr, "[oatk alloc] %.3f hipMalloc %10.3f MB: %.4f s%s\n", dev_now(), (double) bytes / 1e6, dev_now() - t0, e == hipSuccess? "" : " FAILED");
    {   // OATK_DEBUG_POISON=1 (tests): new memory is 0xA5 all over instead of the driver's zeros -- whatever relies on zeros it did not write shows
        static const int poison = [] { const char *ev = getenv("OATK_DEBUG_POISON"); return ev && ev[0] == '1'; }();
        if (poison && e == hipSuccess) { (void) hipMemset(*p, 0xA5, bytes); (void) hipDeviceSynchronize(); }
    }
    return e;
}
static void dev_free(void *p, size_t bytes)
{
    const double t0 = dev_alloc_log()? dev_now() : 0;
    (void) hipFree(p);
    if (dev_alloc_log()) fprintf(stderr, "[oatk alloc] %.3f hipFree   %10.3f MB: %.4f s\n", dev_now(), (double) bytes / 1e6, dev_now() - t0);
}

// A device array that owns its memory: a hipMalloc'ed block, or (with a pool, from the threshold's size on) an address range backed by pieces.
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    // the form in pieces: p is an address range of `va` bytes, its first ch.size() * DM_CHUNK bytes backed
    size_t va = 0;
    ChunkPool *pool = nullptr;
    bool decided = false;                     // whether this buffer lives in pieces was settled (at its first request of the threshold's size)
    std::vector<hipMemGenericAllocationHandle_t> ch;

    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf(DevBuf &&) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf &operator=(DevBuf &&) = delete;
    ~DevBuf() { release(); }

    bool ensure(size_t bytes, hipStream_t st, bool zero_new = false)
    {
        if (bytes <= cap) return true;
        if (!grow(bytes, false, 0, st)) return false;
        if (zero_new) (void) hipMemsetAsync(p, 0, cap, st);
        return true;
    }
    // grow without losing the first `used` bytes (appending to a resident batch)
    bool grow_keep(size_t bytes, size_t used, hipStream_t st) { return bytes <= cap || grow(bytes, true, used, st); }
    // room for `bytes` LATER: in pieces that is an address range and nothing else (the pieces come as the buffer fills); otherwise the memory itself, now
    bool reserve(size_t bytes, size_t used, hipStream_t st)
    {
        if (bytes <= cap) return true;
        place(bytes);
        if (pool && (va || !p)) {
            if (vm_range(up(bytes), st)) return true;
            if (!ch.empty()) return false;
            pool = nullptr, p = nullptr, cap = 0, va = 0;      // no range for a buffer that holds nothing yet: it is hipMalloc's (see grow)
        }
        return grow(bytes, true, used, st);
    }
    void release()
    {
        if (va) {
            (void) hipDeviceSynchronize();
            for (size_t i = 0; i < ch.size(); ++i) { (void) hipMemUnmap((char *) p + i * DM_CHUNK, DM_CHUNK); pool->give(ch[i]); }
            ch.clear();
            // (the address range is NOT given back: see vm_range)
            if (dev_alloc_log()) fprintf(stderr, "[oatk alloc] %.3f pieces    %10.3f MB back to the pool\n", dev_now(), (double) cap / 1e6);
            p = nullptr, cap = 0, va = 0, decided = false;
            return;
        }
        if (p) dev_free(p, cap);
        p = nullptr; cap = 0, decided = false;
    }
    template <class T> T *as() const { return (T *) p; }

private:
    static size_t up(size_t b) { return (b + DM_CHUNK - 1) / DM_CHUNK * DM_CHUNK; }
    // whether this buffer lives in pieces: settled once, at its first request of the threshold's size
    void place(size_t bytes)
    {
        if (va || decided) return;
        decided = bytes >= dm_min();
        pool = decided? pool_for_new_buffer() : nullptr;
    }
    // an address range of at least `bytes`; what is mapped moves along (no copy).  false: nothing changed
    bool vm_range(size_t bytes, hipStream_t st)
    {
        if (bytes <= va) return true;
        const size_t nva = up(bytes < (1ull << 30)? 4 * bytes + (256ull << 20) : bytes + bytes / 2 + (2ull << 30));     // room to grow in place
        void *np = nullptr;
        { const hipError_t er = hipMemAddressReserve(&np, nva, 2 << 20, nullptr, 0);
          if (er != hipSuccess) { if (dev_alloc_log()) fprintf(stderr, "[oatk alloc] hipMemAddressReserve of %.1f MB FAILED: %s\n", (double) nva / 1e6, hipGetErrorString(er)); (void) hipGetLastError(); return false; } }
        if (!ch.empty()) {
            (void) hipStreamSynchronize(st);
            (void) hipDeviceSynchronize();
            for (size_t i = 0; i < ch.size(); ++i) {
                (void) hipMemUnmap((char *) p + i * DM_CHUNK, DM_CHUNK);
                if (hipMemMap((char *) np + i * DM_CHUNK, DM_CHUNK, 0, ch[i], 0) != hipSuccess) return false;       // (cannot happen on a range just reserved)
            }
            if (hipMemSetAccess(np, ch.size() * DM_CHUNK, &pool->acc, 1) != hipSuccess) return false;
        }
        // An address range, once reserved, is never given back while the process lives -- not the one the pieces have just moved out of, not a released buffer's.
        // With hipMemAddressFree in either place a range reserved LATER (at the same addresses, presumably) showed other contents than were written to it: the
        // correction's results changed in 8 - 14 of 158 cases of tests/test_gpu_ec.py + levdist + light_graph + overlap run over pieces, every run, and in none with the
        // ranges kept (ROCm 7.0.2; translations of the old mapping that outlive it is the guess, not looked into further).  Address space is what this costs: a buffer's
        // range is a few times its size, a process of the CLI has some hundreds of such buffers in its life -- a terabyte of a 47-bit space at the outside.
        if (dev_alloc_log()) fprintf(stderr, "[oatk alloc] %.3f address range %10.3f MB (%zu pieces moved)\n", dev_now(), (double) nva / 1e6, ch.size());
        p = np, va = nva;
        return true;
    }
    // pieces for the first `bytes`, all of them or none: false leaves the buffer as it was (a range that was reserved stays)
    bool vm_grow(size_t bytes, hipStream_t st)
    {
        const size_t want = up(bytes);
        if (!vm_range(want, st)) return false;
        const size_t had = ch.size(), have = had * DM_CHUNK;
        const double t0 = dev_alloc_log()? dev_now() : 0;
        bool any_used = false, ok = true;
        while (ok && ch.size() * DM_CHUNK < want) {
            hipMemGenericAllocationHandle_t h;
            bool was_used;
            if (!pool->take(&h, &was_used)) { if (dev_alloc_log()) fprintf(stderr, "[oatk alloc] no piece to be had\n"); ok = false; break; }
            const hipError_t er = hipMemMap((char *) p + ch.size() * DM_CHUNK, DM_CHUNK, 0, h, 0);
            if (er != hipSuccess) { if (dev_alloc_log()) fprintf(stderr, "[oatk alloc] hipMemMap FAILED: %s\n", hipGetErrorString(er)); (void) hipGetLastError(); pool->give(h); ok = false; break; }
            ch.push_back(h);
            any_used |= was_used;
        }
        if (ok && want > have) {
            const hipError_t er = hipMemSetAccess((char *) p + have, want - have, &pool->acc, 1);
            if (er != hipSuccess) { if (dev_alloc_log()) fprintf(stderr, "[oatk alloc] hipMemSetAccess FAILED: %s\n", hipGetErrorString(er)); (void) hipGetLastError(); ok = false; }
        }
        if (!ok) {                                                 // the pieces that did come go back to the pool
            for (; ch.size() > had; ch.pop_back()) { (void) hipMemUnmap((char *) p + (ch.size() - 1) * DM_CHUNK, DM_CHUNK); pool->give(ch.back()); }
            return false;
        }
        // memory from hipMalloc is zero, always (the driver clears what it hands out): pieces that served another buffer are made so (5 TB/s: 13 us a piece)
        // -- and waited for: the buffer's first user may be a kernel on another stream than `st`
        if (any_used && (hipMemsetAsync((char *) p + have, 0, want - have, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) return false;
        if (dev_alloc_log()) fprintf(stderr, "[oatk alloc] %.3f pieces    %10.3f MB -> %10.3f MB: %.4f s\n", dev_now(), (double) have / 1e6, (double) want / 1e6, dev_now() - t0);
        cap = want;
        return true;
    }
    // The one way a buffer grows, to at least `bytes`.  keep: its first `used` bytes survive, and the slack is for appending (a quarter; none in pieces, which grow
    // where they are).  Otherwise the contents go, a hipMalloc'ed block is freed BEFORE the new one is taken, and the slack is an eighth (a sixteenth in pieces).
    //   false leaves the buffer empty or as it was.
    bool grow(size_t bytes, bool keep, size_t used, hipStream_t st)
    {
        place(bytes);
        void *old = va? nullptr : p;                                // a hipMalloc'ed block
        const size_t old_cap = cap;
        if (old && !keep) { (void) hipStreamSynchronize(st); dev_free(old, old_cap); old = p = nullptr, cap = 0; }
        if (pool) {
            if (old) p = nullptr, cap = 0;                          // from a hipMalloc'ed block (a small one that has outgrown the threshold) to pieces: the one copy of this buffer's life
            const bool grown = vm_grow(keep? bytes : bytes + bytes / 16, st);
            if (grown && (!old || !used || hipMemcpyAsync(p, old, used, hipMemcpyDeviceToDevice, st) == hipSuccess)) {
                if (old) { (void) hipStreamSynchronize(st); dev_free(old, old_cap); }
                return true;
            }
            if (!old && !ch.empty()) return false;                  // out of memory with pieces in place: they stay
            if (old) release();                                     // back onto the old block; the pieces that came go to the pool
            pool = nullptr, p = old, cap = old? old_cap : 0, va = 0;
            if (grown) return false;                                // (the copy failed)
            // no range or no piece to start with: this buffer is hipMalloc's -- for good where it held nothing (a range that was reserved stays reserved)
        }
        void *np = nullptr;
        const size_t want = bytes + bytes / (keep? 4 : 8) + 256;
        if (dev_malloc(&np, want) != hipSuccess) return false;
        if (p && used && hipMemcpyAsync(np, p, used, hipMemcpyDeviceToDevice, st) != hipSuccess) { dev_free(np, want); return false; }
        if (keep) (void) hipStreamSynchronize(st);                 // (what was copied has arrived before the old block goes)
        if (p) dev_free(p, cap);
        p = np, cap = want;
        return true;
    }
};

}  // namespace
