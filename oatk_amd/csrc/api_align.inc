// oatk_amd/csrc/api_align.inc -- C ABI of the read -> unitig alignment (include/oatk_hip_align.h); part of api.hip, after api_ec.inc.
#include "../../include/oatk_hip_align.h"
#include "align.hpp"
#include "align_big.hpp"
#include <vector>

struct RaState {
    DevBuf su_off, su_uid, su_pos, utg_n, idx_p, idx_n, arc_w, arc_ln, arc_del, old_ra;
    DevBuf slab, cnt_aln, cnt_frg, skipped, tmp64, aln_off, frg_off, stats, skip_list, big_list;
    // align_big.hpp: a batch's working arrays -- two dozen of them, carved out of TWO allocations (round 6): bgH holds what is sized by the batch's hits, bgF what is sized by
    // its fragments.  Each array was an allocation of its own that grew with the largest batch seen, some forty hipMalloc / hipFree pairs per run of the config-1 surrogate's
    // CLI -- and those calls take milliseconds in a fresh process on an idle device and tenths of a second while another process holds or has just returned a hundred GB of
    // VRAM (tools/vram_churn_cli.py: scg_read_alignment 0.49 s / 1.38 s / 2.47 s for the same input; VERDICT r05 saw 0.74 and 1.44 s in one bench run).
    struct BgView { void *p = nullptr; template <class T> T *as() const { return (T *) p; } } bg[32];
    DevBuf bg0, bgH, bgF;
    DevBuf o_sid, o_off, o_s, o_uid, o_ubeg, o_uend, o_sbeg, o_send;
    DevBuf p_sid, p_off, p_s, p_uid, p_ubeg, p_uend, p_sbeg, p_send, pool_a, pool_f, pool_used;      // the pool the normal path writes into
    uint64_t n_aln = 0, n_frg = 0, n_skipped = 0;
    bool done = false;
};

static void ra_state_free(oatk_hip_ctx *ctx)
{
    delete ctx->ra;          // (its buffers free themselves: ~DevBuf)
    ctx->ra = nullptr;
}

static int ra_buffer(oatk_hip_ctx *ctx, int which, const void **d_ptr, uint64_t *bytes)
{
    RaState *g = ctx->ra;
    if (!g || !g->done) { ctx->err = "alignments requested before oatk_hip_read_alignment"; return OATK_E_STATE; }
    const uint64_t na = g->n_aln, nf = g->n_frg;
    switch (which) {
        case OATK_BUF_RA_ALN_SID: *d_ptr = g->o_sid.p, *bytes = na * 4; break;
        case OATK_BUF_RA_ALN_OFF: *d_ptr = g->o_off.p, *bytes = (na + 1) * 8; break;
        case OATK_BUF_RA_ALN_S: *d_ptr = g->o_s.p, *bytes = na * 8; break;
        case OATK_BUF_RA_FRG_UID: *d_ptr = g->o_uid.p, *bytes = nf * 8; break;
        case OATK_BUF_RA_FRG_UBEG: *d_ptr = g->o_ubeg.p, *bytes = nf * 4; break;
        case OATK_BUF_RA_FRG_UEND: *d_ptr = g->o_uend.p, *bytes = nf * 4; break;
        case OATK_BUF_RA_FRG_SBEG: *d_ptr = g->o_sbeg.p, *bytes = nf * 4; break;
        case OATK_BUF_RA_FRG_SEND: *d_ptr = g->o_send.p, *bytes = nf * 4; break;
        case OATK_BUF_RA_SKIPPED: *d_ptr = g->skip_list.p, *bytes = g->n_skipped * 4; break;
        default: ctx->err = "unknown buffer id"; return OATK_E_ARG;
    }
    return OATK_OK;
}

// [0] reads with an alignment, [1] with exactly one, [2] reads over the working limits (appended to list, in no particular order)
__global__ void ra_stats_kernel(uint64_t n, const uint32_t *cnt_aln, const uint8_t *skipped, unsigned long long *stats, uint32_t *list)
{
    uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (cnt_aln[i]) atomicAdd(&stats[0], 1ULL);
    if (cnt_aln[i] == 1) atomicAdd(&stats[1], 1ULL);
    if (skipped[i]) list[atomicAdd(&stats[2], 1ULL)] = (uint32_t) i;
}

// the reads the first tier reported, for the second (stats[3] counts them)
__global__ void ra_biglist_kernel(uint64_t n, const uint8_t *skipped, unsigned long long *stats, uint32_t *list)
{
    uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && skipped[i]) list[atomicAdd(&stats[3], 1ULL)] = (uint32_t) i;
}

// OATK_DEBUG_RA: which limit the skipped reads are over ([1..4]) and how many hits they have ([8 + log2 bucket], [7] the most)
__global__ void ra_debug_kernel(oatk::RaArgs a, unsigned long long *dbg)
{
    uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_reads || !a.skipped[r]) return;
    atomicAdd(&dbg[a.skipped[r] & 7u], 1ULL);
    unsigned long long hits = 0;
    for (uint64_t j = a.chain_off[r]; j < a.chain_off[r + 1]; ++j) { const uint64_t s = a.k_mer[j] >> 1; hits += a.su_off[s + 1] - a.su_off[s]; }
    atomicMax(&dbg[7], hits);
    int b = 0;
    while ((hits >> b) > 1 && b < 23) ++b;
    atomicAdd(&dbg[8 + b], 1ULL);
}

#define RENSURE(buf, bytes) ENSURE_IN(g, "align.", buf, bytes)
#define RUPLOAD(buf, src, bytes)                                                                   \
    do {                                                                                           \
        RENSURE(buf, (bytes) + 8);                                                                 \
        if (bytes) CK(hipMemcpyAsync(g->buf.p, (src), (bytes), hipMemcpyHostToDevice, ctx->stream)); \
    } while (0)

// ---- the reads over the lane-per-read limits (align_big.hpp) ----
struct RaBigRun {
    std::vector<uint32_t> list;                      // eligible reads, in the order of the device list
    std::vector<uint64_t> hits;
    std::vector<std::pair<size_t, size_t>> batch;    // [first, last) of list
    uint64_t n_over = 0;                             // reads the big path cannot take either
};
__global__ void rab_iota_kernel(uint32_t *p, uint64_t n)
{
    uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = (uint32_t) i;
}
// array i of the batch: `bytes` (+ slack) at the slab's cursor
#define BTAKE(slab, cur, i, bytes)                                                                 \
    do {                                                                                           \
        const uint64_t need_ = ((uint64_t) (bytes) + 64 + 255) & ~255ULL;                          \
        if ((cur) + need_ > slab##_cap) { ctx->err = "the alignment of reads with many hits: a working array does not fit its slab (internal)"; return OATK_E_STATE; } \
        g->bg[i].p = (uint8_t *) slab##_p + (cur), (cur) += need_;                                 \
    } while (0)
static inline uint64_t rab_pad(uint64_t bytes) { return (bytes + 64 + 255) & ~255ULL; }
// mode 0 / 2: find the reads, count (and with 2 write into the pool); mode 1: write at the scanned offsets (same reads, same batches)
static int ra_big_run(oatk_hip_ctx *ctx, RaState *g, const oatk::RaArgs &a, int mode, RaBigRun *big)
{
    using namespace oatk;
    const uint64_t nr = a.n_reads;
    if (mode != 1) {
        big->list.clear(), big->hits.clear(), big->batch.clear(), big->n_over = 0;
        RENSURE(big_list, (nr + 1) * 4);
        CK(hipMemsetAsync(g->stats.as<uint64_t>() + 3, 0, 8, ctx->stream));
        hipLaunchKernelGGL(ra_biglist_kernel, dim3((unsigned) ((nr + 255) / 256)), dim3(256), 0, ctx->stream, nr, g->skipped.as<uint8_t>(), (unsigned long long *) g->stats.p,
                           g->big_list.as<uint32_t>());
        unsigned long long st4[4];
        CK(hipMemcpyAsync(st4, g->stats.p, sizeof(st4), hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        const uint64_t n_big = st4[3];
        if (!n_big) return OATK_OK;
        if (n_big >= (1ull << 32)) return OATK_OK;
        if (!g->bg0.ensure(n_big * 8 + 64, ctx->stream)) { ctx->err = "hipMalloc failed for the alignment of reads with many hits"; return OATK_E_NOMEM; }
        hipLaunchKernelGGL(rab_count_hits_kernel, dim3((unsigned) ((n_big + 3) / 4)), dim3(256), 0, ctx->stream, a, g->big_list.as<uint32_t>(), (uint32_t) n_big, (unsigned long long *) g->bg0.p);
        std::vector<uint32_t> l(n_big);
        std::vector<uint64_t> h(n_big);
        CK(hipMemcpyAsync(l.data(), g->big_list.p, n_big * 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipMemcpyAsync(h.data(), g->bg0.p, n_big * 8, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        // (the list comes from atomics: put it in read order, so that what the batches hold does not depend on the launch)
        std::vector<std::pair<uint32_t, uint64_t>> lh(n_big);
        for (size_t i = 0; i < n_big; ++i) lh[i] = {l[i], h[i]};
        std::sort(lh.begin(), lh.end());
        // hits per batch.  (A batch costs what its slowest read costs, ~70 ms on the config-1 surrogate, whatever it holds: 16 M per batch took 0.95 s where 96 M take 0.48,
        //  4 M 2.5 s -- profiles/r06w_vram_churn.txt.  The eight gigabytes of working arrays the largest batch then wants are borrowed from the solver, below.)
        uint64_t budget = 96ull << 20;
        { const char *ev = getenv("OATK_DEBUG_RA_BUDGET"); if (ev && atoll(ev) > 0) budget = (uint64_t) atoll(ev); }
        size_t first = 0;
        uint64_t sum = 0;
        for (size_t i = 0; i < n_big; ++i) {
            if (lh[i].second >= RAB_MAX_HITS) { ++big->n_over; continue; }      // (rab_count_hits_kernel: also a read with 2^15 syncmers or more)
            if (big->list.size() - first == (1u << RAB_IDX_BITS) - 1 || (sum + lh[i].second > budget && big->list.size() > first)) {
                big->batch.push_back({first, big->list.size()});
                first = big->list.size(), sum = 0;
            }
            big->list.push_back(lh[i].first), big->hits.push_back(lh[i].second), sum += lh[i].second;
        }
        if (big->list.size() > first) big->batch.push_back({first, big->list.size()});
    }
    void *bgH_p = nullptr, *bgF_p = nullptr;
    size_t bgH_cap = 0, bgF_cap = 0;
    {   // the slab of everything sized by a batch's reads and hits, for the largest batch of this call: one allocation (grown, never shrunk)
        uint64_t need = 0;
        for (const auto &bt : big->batch) {
            const uint64_t nb = bt.second - bt.first;
            uint64_t H = 0;
            for (size_t i = 0; i < nb; ++i) H += big->hits[bt.first + i];
            if (H == 0 || H >= (1ull << 32)) continue;
            const uint64_t n1 = rab_pad(nb * 4) * 2 + rab_pad((nb + 1) * 8) * 2 + rab_pad(H * 8) * 7 + rab_pad(H * 4) * 7 + rab_pad(H);
            if (n1 > need) need = n1;
        }
        // Memory the process already holds before memory it has to ask for: the error-block solver's slabs lie idle once the correction is done (gigabytes on a repeat-rich
        // read set), and hipMalloc of gigabytes is what takes 0.6 - 3.5 s instead of 0.02 while another process holds or has just returned a hundred GB of VRAM
        // (tools/vram_churn_cli.py, profiles/r06v_vram_churn.txt).  The smallest of them that is large enough is borrowed for the call; the solver fills its slabs afresh
        // in every launch, and the handle runs one thing at a time.
        bgH_p = g->bgH.p, bgH_cap = g->bgH.cap;
        if (need > bgH_cap) {
            EcState *e = ctx->ec;
            DevBuf *best = nullptr;
            if (e && e->done && !getenv("OATK_DEBUG_RA_OWN_SLAB")) {
                for (DevBuf &b : e->hyb_slabs) if (b.p && b.cap >= need && (!best || b.cap < best->cap)) best = &b;
                if (e->big_slabs.p && e->big_slabs.cap >= need && (!best || e->big_slabs.cap < best->cap)) best = &e->big_slabs;
            }
            if (best) bgH_p = best->p, bgH_cap = best->cap;
            else {
                if (!g->bgH.ensure(need, ctx->stream)) { ctx->err = "hipMalloc failed for the alignment of reads with many hits"; return OATK_E_NOMEM; }
                bgH_p = g->bgH.p, bgH_cap = g->bgH.cap;
            }
        }
        if (getenv("OATK_DEBUG_RA_STAGES")) fprintf(stderr, "[ra] %zu batches of reads with many hits, the largest wants %.1f MB of working arrays (%s slab: %.1f MB)\n", big->batch.size(), need / 1e6, bgH_p == g->bgH.p? "own" : "the solver's", bgH_cap / 1e6);
    }
    for (const auto &bt : big->batch) {
        const size_t nb = bt.second - bt.first;
        uint64_t curH = 0, curF = 0;
        std::vector<uint64_t> hoff(nb + 1, 0);
        for (size_t i = 0; i < nb; ++i) hoff[i + 1] = hoff[i] + big->hits[bt.first + i];
        const uint64_t H = hoff[nb];
        if (H == 0 || H >= (1ull << 32)) continue;
        RabArgs q;
        memset(&q, 0, sizeof(q));
        q.a = a, q.n_list = (uint32_t) nb, q.mode = mode;
        BTAKE(bgH, curH, 1, nb * 4); BTAKE(bgH, curH, 2, (nb + 1) * 8); BTAKE(bgH, curH, 3, (nb + 1) * 8); BTAKE(bgH, curH, 4, nb * 4);
        CK(hipMemcpyAsync(g->bg[1].p, big->list.data() + bt.first, nb * 4, hipMemcpyHostToDevice, ctx->stream));
        CK(hipMemcpyAsync(g->bg[2].p, hoff.data(), (nb + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        q.list = g->bg[1].as<uint32_t>(), q.hoff = g->bg[2].as<uint64_t>(), q.foff = g->bg[3].as<uint64_t>(), q.f_cnt = g->bg[4].as<uint32_t>();
        BTAKE(bgH, curH, 5, H * 8); BTAKE(bgH, curH, 6, H * 8); BTAKE(bgH, curH, 7, H * 8); BTAKE(bgH, curH, 8, H * 8); BTAKE(bgH, curH, 9, H * 4); BTAKE(bgH, curH, 10, H);
        q.key_lo = g->bg[5].as<uint64_t>(), q.key_hi = g->bg[6].as<uint64_t>(), q.next = g->bg[9].as<uint32_t>(), q.haspred = g->bg[10].as<uint8_t>();
        uint64_t *lo2 = g->bg[7].as<uint64_t>(), *hi2 = g->bg[8].as<uint64_t>();
        hipLaunchKernelGGL(rab_expand_kernel, dim3((unsigned) ((nb + 3) / 4)), dim3(256), 0, ctx->stream, q);
        {   // sr_scm_cmpfunc's order (alignment.c:93-107) over the whole batch: by (read position, unitig position), then -- stable -- by (read, unitig)
            PRIM_IN(g->tmp64, ctx->stream, "hipMalloc failed for align.tmp64", rocprim::radix_sort_pairs, q.key_lo, lo2, q.key_hi, hi2, H, 0, 48, ctx->stream);
            PRIM_IN(g->tmp64, ctx->stream, "hipMalloc failed for align.tmp64", rocprim::radix_sort_pairs, hi2, q.key_hi, lo2, q.key_lo, H, 0, 43 + RAB_IDX_BITS, ctx->stream);
        }
        CK(hipMemsetAsync(q.haspred, 0, H, ctx->stream));
        hipLaunchKernelGGL(rab_links_kernel, dim3((unsigned) nb), dim3(256), 0, ctx->stream, q);
        // fragments as collected: the slots of the hit segments (a read has fewer fragments than hits); unused slots sort behind everything
        BTAKE(bgH, curH, 11, H * 8); BTAKE(bgH, curH, 12, H * 8); BTAKE(bgH, curH, 13, H * 4); BTAKE(bgH, curH, 14, H * 4); BTAKE(bgH, curH, 15, H * 4); BTAKE(bgH, curH, 16, H * 4); BTAKE(bgH, curH, 17, H * 4); BTAKE(bgH, curH, 18, H * 4);
        q.f_uid = g->bg[11].as<uint64_t>(), q.f_key = g->bg[12].as<uint64_t>(), q.f_sbeg = g->bg[13].as<uint32_t>(), q.f_send = g->bg[14].as<uint32_t>();
        q.f_scnt = g->bg[15].as<uint32_t>(), q.f_ubeg = g->bg[16].as<uint32_t>(), q.f_uend = g->bg[17].as<uint32_t>(), q.f_score = g->bg[18].as<int32_t>();
        CK(hipMemsetAsync(q.f_key, 0xFF, H * 8, ctx->stream));
        hipLaunchKernelGGL(rab_frags_kernel, dim3((unsigned) nb), dim3(64), 0, ctx->stream, q);
        std::vector<uint32_t> fc(nb);
        CK(hipMemcpyAsync(fc.data(), q.f_cnt, nb * 4, hipMemcpyDeviceToHost, ctx->stream));
        {   // the reference's stable sort by (s_beg, s_end) of its push order (sr_frg_cmpfunc :109-119), read by read
            uint32_t *iota = (uint32_t *) lo2, *order = (uint32_t *) hi2;              // (the sort's second buffers are free again)
            hipLaunchKernelGGL(rab_iota_kernel, dim3((unsigned) ((H + 255) / 256)), dim3(256), 0, ctx->stream, iota, H);
            BTAKE(bgH, curH, 19, H * 8);
            PRIM_IN(g->tmp64, ctx->stream, "hipMalloc failed for align.tmp64", rocprim::radix_sort_pairs, q.f_key, g->bg[19].as<uint64_t>(), iota, order, H, 0, 64, ctx->stream);
            q.f_order = order;
        }
        CK(hipStreamSynchronize(ctx->stream));
        std::vector<uint64_t> foff(nb + 1, 0);
        for (size_t i = 0; i < nb; ++i) foff[i + 1] = foff[i] + fc[i];
        const uint64_t F = foff[nb];
        CK(hipMemcpyAsync(g->bg[3].p, foff.data(), (nb + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        // (nothing of the batch before lives in the fragments' slab: it may move when a batch has more of them)
        if (!g->bgF.ensure(rab_pad((F + 1) * 8) * 2 + rab_pad((F + 1) * 4 * 8) + rab_pad((F + 1) * 4 * (uint64_t) RAB_PREV), ctx->stream)) { ctx->err = "hipMalloc failed for the alignment of reads with many hits"; return OATK_E_NOMEM; }
        bgF_p = g->bgF.p, bgF_cap = g->bgF.cap;
        BTAKE(bgF, curF, 20, (F + 1) * 8); BTAKE(bgF, curF, 21, (F + 1) * 4 * 8); BTAKE(bgF, curF, 22, (F + 1) * 4 * (uint64_t) RAB_PREV); BTAKE(bgF, curF, 23, (F + 1) * 8);
        q.g_uid = g->bg[20].as<uint64_t>();
        uint32_t *w = g->bg[21].as<uint32_t>();
        q.g_sbeg = w, q.g_send = w + (F + 1), q.g_scnt = w + 2 * (F + 1), q.g_ubeg = w + 3 * (F + 1), q.g_uend = w + 4 * (F + 1), q.g_prevn = w + 5 * (F + 1);
        q.g_score0 = (int32_t *) (w + 6 * (F + 1)), q.g_score = (int32_t *) (w + 7 * (F + 1));
        q.g_prev = g->bg[22].as<uint32_t>(), q.stack = g->bg[23].as<uint64_t>();
        hipLaunchKernelGGL(rab_chain_kernel, dim3((unsigned) nb), dim3(64), 0, ctx->stream, q);
        CK(hipStreamSynchronize(ctx->stream));      // (the host vectors above go out of scope; a batch is hundreds of milliseconds)
    }
    CK(hipGetLastError());
    return OATK_OK;
}
static int ra_big_count(oatk_hip_ctx *ctx, RaState *g, const oatk::RaArgs &a, RaBigRun *big) { return ra_big_run(ctx, g, a, ctx->ra_two_pass? 0 : 2, big); }

extern "C" int oatk_hip_read_alignment(oatk_hip_ctx *ctx, const oatk_ra_graph_t *hg, const int64_t *old_ra, uint64_t *n_aln, uint64_t *n_frg, uint64_t *stats3)
{
    using namespace oatk;
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->counted) { ctx->err = "oatk_hip_read_alignment needs a resident scan + count"; return OATK_E_STATE; }
    if (!hg) { ctx->err = "oatk_hip_read_alignment: no graph"; return OATK_E_ARG; }
    EcState *e = ctx->ec;
    const bool after_ec = e && e->done;
    if (e && e->global && !after_ec) { ctx->err = "oatk_hip_read_alignment: sharded reads are aligned after oatk_hip_ec_correct"; return OATK_E_STATE; }
    if (hg->n_scm != ec_n_vtx(ctx)) { ctx->err = "oatk_hip_read_alignment: the graph's syncmer table is not the resident one"; return OATK_E_ARG; }
    if (hg->n_utg >= (1ULL << 42)) { ctx->err = "too many unitigs"; return OATK_E_ARG; }
    CK(hipSetDevice(ctx->device));
    if (!ctx->ra) ctx->ra = new RaState();
    RaState *g = ctx->ra;
    g->done = false;
    // OATK_DEBUG_RA_STAGES=1: where a call's time goes (the stream is drained at every mark)
    static const bool ra_log = getenv("OATK_DEBUG_RA_STAGES") != nullptr;
    struct timespec ra_t0;
    clock_gettime(CLOCK_MONOTONIC, &ra_t0);
    auto ra_mark = [&](const char *what) {
        if (!ra_log) return;
        (void) hipStreamSynchronize(ctx->stream);
        struct timespec t1;
        clock_gettime(CLOCK_MONOTONIC, &t1);
        fprintf(stderr, "[ra] %-28s %8.2f ms\n", what, ((double) (t1.tv_sec - ra_t0.tv_sec) + 1e-9 * (double) (t1.tv_nsec - ra_t0.tv_nsec)) * 1e3);
        ra_t0 = t1;
    };
    const uint64_t nr = ctx->n_reads, ns = hg->n_scm, nu = hg->n_utg, na = hg->n_arc, nsu = ns? hg->su_off[ns] : 0;
    RUPLOAD(su_off, hg->su_off, (ns + 1) * 8); RUPLOAD(su_uid, hg->su_uid, nsu * 8); RUPLOAD(su_pos, hg->su_pos, nsu * 4);
    RUPLOAD(utg_n, hg->utg_n, nu * 4); RUPLOAD(idx_p, hg->idx_p, 2 * nu * 8); RUPLOAD(idx_n, hg->idx_n, 2 * nu * 8);
    RUPLOAD(arc_w, hg->arc_w, na * 8); RUPLOAD(arc_ln, hg->arc_ln, na * 8); RUPLOAD(arc_del, hg->arc_del, na);
    if (old_ra) RUPLOAD(old_ra, old_ra, nr * 8);
    ra_mark("graph upload");
    const unsigned maxblk = 1024;
    const unsigned nblk = (unsigned) ((nr + 255) / 256 < maxblk? ((nr + 255) / 256 > 0? (nr + 255) / 256 : 1) : maxblk);
    const uint64_t nthr = (uint64_t) nblk * 256;
    RENSURE(slab, ra_slab_bytes<RaSmall>(nthr));
    RENSURE(cnt_aln, (nr + 1) * 4); RENSURE(cnt_frg, (nr + 1) * 4); RENSURE(skipped, nr + 8); RENSURE(stats, 64); RENSURE(skip_list, (nr + 1) * 4);
    CK(hipMemsetAsync(g->stats.p, 0, 64, ctx->stream));
    RaArgs a;
    memset(&a, 0, sizeof(a));
    a.n_reads = nr, a.n_scm = ns;
    a.chain_off = after_ec? e->new_off.as<uint64_t>() : ctx->scm_off.as<uint64_t>();
    a.k_mer = after_ec? e->new_k.as<uint64_t>() : ctx->pos_kid.as<uint64_t>();
    a.m_pos = after_ec? e->new_m.as<uint32_t>() : ctx->pos_mpos.as<uint32_t>();
    a.su_off = g->su_off.as<uint64_t>(), a.su_uid = g->su_uid.as<uint64_t>(), a.su_pos = g->su_pos.as<uint32_t>(), a.utg_n = g->utg_n.as<uint32_t>();
    a.idx_p = g->idx_p.as<uint64_t>(), a.idx_n = g->idx_n.as<uint64_t>(), a.arc_w = g->arc_w.as<uint64_t>(), a.arc_ln = g->arc_ln.as<uint64_t>();
    a.arc_del = g->arc_del.as<uint8_t>(), a.old_ra = old_ra? g->old_ra.as<int64_t>() : nullptr;
    a.slab = g->slab.as<uint8_t>();
    a.cnt_aln = g->cnt_aln.as<uint32_t>(), a.cnt_frg = g->cnt_frg.as<uint32_t>(), a.skipped = g->skipped.as<uint8_t>();
    uint64_t tot_a = 0, tot_f = 0;
    RaBigRun big;
    unsigned long long pu[3] = {0, 0, 0};
    // room for the normal path: a read's alignments go straight into a pool (one atomic per read), then a gather puts the reads in order
    const uint64_t nocc = after_ec? e->new_tot : ctx->n_occ, cap_a = 2 * nr + (1ULL << 16), cap_f = 3 * nocc + (1ULL << 18);
    if (nr) {
        RENSURE(p_sid, cap_a * 4); RENSURE(p_off, cap_a * 8); RENSURE(p_s, cap_a * 8); RENSURE(p_uid, cap_f * 8); RENSURE(p_ubeg, cap_f * 4);
        RENSURE(p_uend, cap_f * 4); RENSURE(p_sbeg, cap_f * 4); RENSURE(p_send, cap_f * 4); RENSURE(pool_a, (nr + 1) * 8); RENSURE(pool_f, (nr + 1) * 8);
        RENSURE(pool_used, 64);
        CK(hipMemsetAsync(g->pool_used.p, 0, 64, ctx->stream));
        a.pool_used = (unsigned long long *) g->pool_used.p, a.pool_cap_a = cap_a, a.pool_cap_f = cap_f;
        a.pool_a = g->pool_a.as<uint64_t>(), a.pool_f = g->pool_f.as<uint64_t>();
        a.o_sid = g->p_sid.as<uint32_t>(), a.o_off = g->p_off.as<uint64_t>(), a.o_s = g->p_s.as<double>(), a.o_uid = g->p_uid.as<uint64_t>();
        a.o_ubeg = g->p_ubeg.as<uint32_t>(), a.o_uend = g->p_uend.as<uint32_t>(), a.o_sbeg = g->p_sbeg.as<uint32_t>(), a.o_send = g->p_send.as<uint32_t>();
        ra_mark("room");
        if (ctx->ra_two_pass) hipLaunchKernelGGL((ra_kernel<0, RaSmall>), dim3(nblk), dim3(256), 0, ctx->stream, a);
        else hipLaunchKernelGGL((ra_kernel<2, RaSmall>), dim3(nblk), dim3(256), 0, ctx->stream, a);
        ra_mark("ra_kernel (a lane per read)");
        // the reads over the lane-per-read limits: data-parallel inside the read (align_big.hpp); their counts land in cnt_aln / cnt_frg like everybody's
        if (!getenv("OATK_DEBUG_RA_NO_BIG")) { int rc = ra_big_count(ctx, g, a, &big); if (rc) return rc; }
        ra_mark("reads with many hits");
        CK(hipMemcpyAsync(pu, g->pool_used.p, sizeof(pu), hipMemcpyDeviceToHost, ctx->stream));
        { int rc = prim_scan_total_u32(ctx, g->cnt_aln, g->tmp64, g->aln_off, nr, &tot_a); if (rc) return rc; }
        { int rc = prim_scan_total_u32(ctx, g->cnt_frg, g->tmp64, g->frg_off, nr, &tot_f); if (rc) return rc; }
    }
    RENSURE(o_sid, (tot_a + 1) * 4); RENSURE(o_off, (tot_a + 2) * 8); RENSURE(o_s, (tot_a + 1) * 8);
    RENSURE(o_uid, (tot_f + 1) * 8); RENSURE(o_ubeg, (tot_f + 1) * 4); RENSURE(o_uend, (tot_f + 1) * 4); RENSURE(o_sbeg, (tot_f + 1) * 4); RENSURE(o_send, (tot_f + 1) * 4);
    if (nr) {
        a.aln_off = g->aln_off.as<uint64_t>(), a.frg_off = g->frg_off.as<uint64_t>();
        RaOut dst = {g->o_sid.as<uint32_t>(), g->o_off.as<uint64_t>(), g->o_s.as<double>(), g->o_uid.as<uint64_t>(), g->o_ubeg.as<uint32_t>(),
                     g->o_uend.as<uint32_t>(), g->o_sbeg.as<uint32_t>(), g->o_send.as<uint32_t>()};
        if (ctx->ra_two_pass || pu[2]) {                                         // the pool ran short (or the test hook asks): run the routine again, writing in place
            a.o_sid = dst.sid, a.o_off = dst.off, a.o_s = dst.s, a.o_uid = dst.uid, a.o_ubeg = dst.ubeg, a.o_uend = dst.uend, a.o_sbeg = dst.sbeg, a.o_send = dst.send;
            if (tot_a) hipLaunchKernelGGL((ra_kernel<1, RaSmall>), dim3(nblk), dim3(256), 0, ctx->stream, a);
            if (tot_a && !big.batch.empty()) { int rc = ra_big_run(ctx, g, a, 1, &big); if (rc) return rc; }

        } else if (tot_a) {
            RaOut src = {g->p_sid.as<uint32_t>(), g->p_off.as<uint64_t>(), g->p_s.as<double>(), g->p_uid.as<uint64_t>(), g->p_ubeg.as<uint32_t>(),
                         g->p_uend.as<uint32_t>(), g->p_sbeg.as<uint32_t>(), g->p_send.as<uint32_t>()};
            hipLaunchKernelGGL(ra_gather_kernel, dim3((unsigned) ((nr + 255) / 256)), dim3(256), 0, ctx->stream, nr, g->cnt_aln.as<uint32_t>(), g->cnt_frg.as<uint32_t>(),
                               g->pool_a.as<uint64_t>(), g->pool_f.as<uint64_t>(), g->aln_off.as<uint64_t>(), g->frg_off.as<uint64_t>(), src, dst);
        }
        hipLaunchKernelGGL(ra_stats_kernel, dim3((unsigned) ((nr + 255) / 256)), dim3(256), 0, ctx->stream, nr, g->cnt_aln.as<uint32_t>(), g->skipped.as<uint8_t>(),
                           (unsigned long long *) g->stats.p, g->skip_list.as<uint32_t>());
    }
    if (nr && getenv("OATK_DEBUG_RA")) {
        unsigned long long dbg[32];
        RENSURE(tmp64, 256);
        CK(hipMemsetAsync(g->tmp64.p, 0, 256, ctx->stream));
        hipLaunchKernelGGL(ra_debug_kernel, dim3((unsigned) ((nr + 255) / 256)), dim3(256), 0, ctx->stream, a, (unsigned long long *) g->tmp64.p);
        CK(hipMemcpyAsync(dbg, g->tmp64.p, 256, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        fprintf(stderr, "[oatk::ra] skipped reads over: hits %llu, fragments %llu, predecessors %llu, depth %llu; most hits %llu; by log2(hits):", dbg[1], dbg[2], dbg[3], dbg[4], dbg[7]);
        for (int b = 0; b < 24; ++b) if (dbg[8 + b]) fprintf(stderr, " 2^%d:%llu", b, dbg[8 + b]);
        fprintf(stderr, "\n");
    }
    ra_mark("scans, room, gather");
    CK(hipMemcpyAsync(g->o_off.as<uint64_t>() + tot_a, &tot_f, 8, hipMemcpyHostToDevice, ctx->stream));     // the closing offset
    uint64_t st[3] = {0, 0, 0};
    CK(hipMemcpyAsync(st, g->stats.p, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    g->n_aln = tot_a, g->n_frg = tot_f, g->n_skipped = st[2], g->done = true;
    if (n_aln) *n_aln = tot_a;
    if (n_frg) *n_frg = tot_f;
    if (stats3) stats3[0] = st[0], stats3[1] = st[1], stats3[2] = st[2];
    return OATK_OK;
}
