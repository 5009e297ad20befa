// oatk_amd/csrc/api_ovl.inc -- C ABI of the pair-distance tables (include/oatk_hip_cons.h: oatk_hip_overlap_hist); part of api.hip,
// after api_ec.inc (shares the pair list kernel and the scan helper).
#include "ovlhist.hpp"

struct OvlState {
    DevBuf keys, dist, keys2, dist2, val2, ukeys, counts, nruns, cnt64, runoff, nout, nout64, outoff, o_dist, o_cnt, o_tail, flags, spill;
    uint64_t n_pairs = 0, n_entries = 0;
    bool done = false;
};

static void ovl_state_free(oatk_hip_ctx *ctx)
{
    delete ctx->ovl;          // (its buffers free themselves: ~DevBuf)
    ctx->ovl = nullptr;
}

static int ovl_buffer(oatk_hip_ctx *ctx, int which, const void **d_ptr, uint64_t *bytes)
{
    OvlState *g = ctx->ovl;
    if (!g || !g->done) { ctx->err = "pair-distance tables requested before oatk_hip_overlap_hist"; return OATK_E_STATE; }
    switch (which) {
        case OATK_BUF_OVL_KEY: *d_ptr = g->ukeys.p, *bytes = g->n_pairs * 8; break;
        case OATK_BUF_OVL_OFF: *d_ptr = g->outoff.p, *bytes = (g->n_pairs + 1) * 8; break;
        case OATK_BUF_OVL_DIST: *d_ptr = g->o_dist.p, *bytes = g->n_entries * 4; break;
        case OATK_BUF_OVL_CNT: *d_ptr = g->o_cnt.p, *bytes = g->n_entries * 4; break;
        case OATK_BUF_OVL_TAIL: *d_ptr = g->o_tail.p, *bytes = g->n_pairs; break;
        default: ctx->err = "unknown buffer id"; return OATK_E_ARG;
    }
    return OATK_OK;
}

#define OENSURE(buf, bytes) ENSURE_IN(g, "ovl.", buf, bytes)

// this batch's adjacent pairs for the tables: canonical key (fillers for slot 0 of a read and for pairs with a corrected member) and
// distance, in (read, slot) order
extern "C" int oatk_hip_overlap_pairs(oatk_hip_ctx *ctx, const void **d_keys, const void **d_dist, uint64_t *n)
{
    using namespace oatk;
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->counted) { ctx->err = "oatk_hip_overlap_pairs needs a resident scan + count"; return OATK_E_STATE; }
    EcState *e = ctx->ec;
    const bool after_ec = e && e->done;
    if (e && e->global && !after_ec) { ctx->err = "oatk_hip_overlap_pairs: sharded reads list their pairs after oatk_hip_ec_correct"; return OATK_E_STATE; }
    CK(hipSetDevice(ctx->device));
    if (!ctx->ovl) ctx->ovl = new OvlState();
    OvlState *g = ctx->ovl;
    const uint64_t nr = ctx->n_reads, nocc = after_ec? e->new_tot : ctx->n_occ;
    OENSURE(keys, (nocc + 1) * 8); OENSURE(dist, (nocc + 1) * 4);
    if (nocc) hipLaunchKernelGGL(egr_pair_keys_kernel, dim3((unsigned) ((nr + 255) / 256)), dim3(256), 0, ctx->stream, nr,
                                 after_ec? e->new_off.as<uint64_t>() : ctx->scm_off.as<uint64_t>(), after_ec? e->new_k.as<uint64_t>() : ctx->pos_kid.as<uint64_t>(),
                                 after_ec? e->new_m.as<uint32_t>() : ctx->pos_mpos.as<uint32_t>(), g->keys.as<uint64_t>(), g->dist.as<uint32_t>(), 1);
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    *d_keys = g->keys.p, *d_dist = g->dist.p, *n = nocc;
    return OATK_OK;
}

extern "C" int oatk_hip_overlap_hist(oatk_hip_ctx *ctx, uint64_t *n_pairs, uint64_t *n_entries)
{
    if (!ctx) return OATK_E_NODEV;
    if (ctx->ec && ctx->ec->global) { ctx->err = "oatk_hip_overlap_hist: reads are sharded; gather the pairs and call oatk_hip_overlap_hist_from_pairs"; return OATK_E_STATE; }
    const void *k = nullptr, *d = nullptr;
    uint64_t n = 0;
    int rc = oatk_hip_overlap_pairs(ctx, &k, &d, &n);
    if (rc) return rc;
    return oatk_hip_overlap_hist_from_pairs(ctx, (const uint64_t *) k, (const uint32_t *) d, n, n_pairs, n_entries);
}

static int ovl_build(oatk_hip_ctx *ctx, const uint64_t *d_keys, const uint32_t *d_dist, const uint64_t *d_val, uint64_t nocc, uint64_t *n_pairs, uint64_t *n_entries);
extern "C" int oatk_hip_overlap_hist_from_pairs(oatk_hip_ctx *ctx, const uint64_t *d_keys, const uint32_t *d_dist, uint64_t nocc, uint64_t *n_pairs, uint64_t *n_entries)
{
    return ovl_build(ctx, d_keys, d_dist, nullptr, nocc, n_pairs, n_entries);
}

// d_val == nullptr: one (key, distance) per adjacency in (read, slot) order; otherwise weighted segments (key, distance | calls << 32) in call order
static int ovl_build(oatk_hip_ctx *ctx, const uint64_t *d_keys, const uint32_t *d_dist, const uint64_t *d_val, uint64_t nocc, uint64_t *n_pairs, uint64_t *n_entries)
{
    using namespace oatk;
    const bool weighted = d_val != nullptr;
    if (!ctx) return OATK_E_NODEV;
    CK(hipSetDevice(ctx->device));
    if (!ctx->ovl) ctx->ovl = new OvlState();
    OvlState *g = ctx->ovl;
    g->done = false;
    if (nocc >= 0xFFFFFFFFULL) { ctx->err = "more than 2^32 adjacent pairs"; return OATK_E_ARG; }
    OENSURE(flags, 64);
    CK(hipMemsetAsync(g->flags.p, 0, 64, ctx->stream));
    uint64_t np = 0, ne = 0;
    OENSURE(ukeys, (nocc + 1) * 8); OENSURE(outoff, (nocc + 2) * 8);
    if (nocc) {
        OENSURE(keys2, (nocc + 1) * 8); OENSURE(dist2, (nocc + 1) * 4); OENSURE(counts, (nocc + 1) * 4); OENSURE(nruns, 64);
        uint64_t *keys_in = const_cast<uint64_t *>(d_keys);
        uint32_t *dist_in = const_cast<uint32_t *>(d_dist);
        uint64_t *keys2 = g->keys2.as<uint64_t>(), *ukeys = g->ukeys.as<uint64_t>();
        uint32_t *counts = g->counts.as<uint32_t>(), *d_nruns = g->nruns.as<uint32_t>();
        int rc;                 // stable: the distances of one key stay in (read, slot) order
        if (weighted) {
            OENSURE(val2, (nocc + 1) * 8);
            rc = prim_sort_runs(ctx, keys_in, keys2, const_cast<uint64_t *>(d_val), g->val2.as<uint64_t>(), nocc, 0, 64, ukeys, counts, d_nruns);
        }
        else rc = prim_sort_runs(ctx, keys_in, keys2, dist_in, g->dist2.as<uint32_t>(), nocc, 0, 64, ukeys, counts, d_nruns);
        if (rc) return rc;
        uint32_t n_runs = 0;
        uint64_t last_key = 0, chk = 0;
        CK(hipMemcpyAsync(&n_runs, g->nruns.p, 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        if (n_runs) {
            CK(hipMemcpyAsync(&last_key, g->ukeys.as<uint64_t>() + (n_runs - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
            { int rc = prim_scan_total_u32(ctx, g->counts, g->cnt64, g->runoff, n_runs, &chk); if (rc) return rc; }
            OENSURE(nout, ((uint64_t) n_runs + 1) * 4); OENSURE(o_tail, (uint64_t) n_runs + 8); OENSURE(spill, OVH_SPILL);
            CK(hipMemsetAsync(g->o_tail.p, 0, (uint64_t) n_runs + 8, ctx->stream));
            auto kern = weighted? ovh_kernel_t<true> : ovh_kernel_t<false>;
            hipLaunchKernelGGL(kern, dim3(n_runs), dim3(64), 0, ctx->stream, (uint64_t) n_runs, g->ukeys.as<uint64_t>(), g->counts.as<uint32_t>(),
                               g->runoff.as<uint64_t>(), g->dist2.as<uint32_t>(), g->val2.as<uint64_t>(), g->nout.as<uint32_t>(), (const uint64_t *) nullptr, (int32_t *) nullptr,
                               (uint32_t *) nullptr, (uint8_t *) nullptr, g->flags.as<uint32_t>(), (const uint32_t *) nullptr, g->spill.as<uint8_t>(), (uint64_t) OVH_SPILL);
            { int rc = prim_scan_total_u32(ctx, g->nout, g->nout64, g->outoff, n_runs, &ne); if (rc) return rc; }
            OENSURE(o_dist, (ne + 1) * 4); OENSURE(o_cnt, (ne + 1) * 4);
            hipLaunchKernelGGL(kern, dim3(n_runs), dim3(64), 0, ctx->stream, (uint64_t) n_runs, g->ukeys.as<uint64_t>(), g->counts.as<uint32_t>(),
                               g->runoff.as<uint64_t>(), g->dist2.as<uint32_t>(), g->val2.as<uint64_t>(), (uint32_t *) nullptr, g->outoff.as<uint64_t>(), g->o_dist.as<int32_t>(),
                               g->o_cnt.as<uint32_t>(), g->o_tail.as<uint8_t>(), g->flags.as<uint32_t>(), g->nout.as<uint32_t>(), g->spill.as<uint8_t>(), (uint64_t) OVH_SPILL);
            np = last_key == EGR_INVALID? n_runs - 1 : n_runs;           // the fillers sort behind every pair
        }
    }
    if (np == 0) CK(hipMemsetAsync(g->outoff.p, 0, 16, ctx->stream));
    OENSURE(o_dist, (ne + 1) * 4); OENSURE(o_cnt, (ne + 1) * 4); OENSURE(o_tail, np + 8);
    uint32_t fl[4] = {0, 0, 0, 0};
    CK(hipMemcpyAsync(fl, g->flags.p, sizeof(fl), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    if (fl[1]) { ctx->err = "the pairs of adjacent syncmers with more than 64 distinct distances need more than the 128 MB of working memory set aside for them"; return OATK_E_SPLIT; }
    if (debug_refuse(ctx, 8, "oatk_hip_overlap_hist")) return OATK_E_SPLIT;
    g->n_pairs = np, g->n_entries = ne, g->done = true;
    if (n_pairs) *n_pairs = np;
    if (n_entries) *n_entries = ne;
    return OATK_OK;
}
