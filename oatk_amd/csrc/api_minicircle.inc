// oatk_amd/csrc/api_minicircle.inc -- C ABI of the mini-circle repeat units from the read alignments (include/oatk_hip_racov.h: oatk_hip_ra_minicircle_units),
// one handle; part of api.hip, after api_multiplex.inc.
#include "minicircle.hpp"
#include <numeric>

struct McState {
    DevBuf a_off, f_uid;                             // uploaded alignments: offsets and uids are all the rule reads
    DevBuf unit[2];                                  // MC_UNIT is unit[cur]; a call works in the other one and switches when nothing can refuse it any more
    int cur = 0;
    DevBuf path_off, path_v, path_cnt;               // MC_PATH_*: written at the end of a call that succeeds
    DevBuf err, n_long, long_idx, flag, nv, pos, voff, rec, p_off, v, key, key2, val, val2, rep, left, cnt, n_sel, o_off, o_v, o_cnt, tmp;
    uint64_t n_aln = 0, n_path = 0, n_path_vtx = 0;
    bool done = false;
    unsigned hash_bits = 0;                          // test hook: 0 = all 64
    uint64_t rounds = 0;                             // verify rounds of the last call (1 unless two paths shared a key)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};      // begin, units done, paths done, distinct done
    float ms[3] = {0.f, 0.f, 0.f};
    ~McState() { for (hipEvent_t e : ev) if (e) (void) hipEventDestroy(e); }
};

static void mc_state_free(oatk_hip_ctx *ctx)
{
    delete ctx->mc;
    ctx->mc = nullptr;
}
static McState *mc_state(oatk_hip_ctx *ctx)
{
    if (!ctx->mc) ctx->mc = new McState();
    return ctx->mc;
}

#define MC_ENSURE(buf, bytes) ENSURE_IN(g, "minicircle.", buf, (uint64_t) (bytes) + 64)
#define MC_PRIM(fn, ...) PRIM_IN(g->tmp, ctx->stream, "hipMalloc failed for minicircle.tmp", fn, __VA_ARGS__)

static int mc_buffer(oatk_hip_ctx *ctx, int which, const void **d_ptr, uint64_t *bytes)
{
    McState *g = ctx->mc;
    if (!g || !g->done) { ctx->err = "mini-circle units requested before oatk_hip_ra_minicircle_units"; return OATK_E_STATE; }
    switch (which) {
        case OATK_BUF_MC_UNIT: *d_ptr = g->unit[g->cur].p, *bytes = g->n_aln * 8; break;
        case OATK_BUF_MC_PATH_OFF: *d_ptr = g->path_off.p, *bytes = (g->n_path + 1) * 8; break;
        case OATK_BUF_MC_PATH_V: *d_ptr = g->path_v.p, *bytes = g->n_path_vtx * 4; break;
        case OATK_BUF_MC_PATH_CNT: *d_ptr = g->path_cnt.p, *bytes = g->n_path * 8; break;
        default: ctx->err = "unknown buffer id"; return OATK_E_ARG;
    }
    return OATK_OK;
}

extern "C" int oatk_hip_debug_mc_hash_bits(oatk_hip_ctx *ctx, unsigned bits)
{
    if (!ctx) return OATK_E_NODEV;
    mc_state(ctx)->hash_bits = bits;
    return OATK_OK;
}

extern "C" int oatk_hip_ra_minicircle_times(oatk_hip_ctx *ctx, float *ms3, uint64_t *rounds)
{
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->mc || !ctx->mc->done) { ctx->err = "oatk_hip_ra_minicircle_times: no units made yet"; return OATK_E_STATE; }
    if (ms3) memcpy(ms3, ctx->mc->ms, sizeof(ctx->mc->ms));
    if (rounds) *rounds = ctx->mc->rounds;
    return OATK_OK;
}

// the results of a call that found `np` distinct paths (host arrays in path_cmpfunc order) become the resident ones
static int mc_commit(oatk_hip_ctx *ctx, McState *g, uint64_t na, const std::vector<uint64_t> &off, const std::vector<uint32_t> &v, const std::vector<uint64_t> &cnt)
{
    const uint64_t np = cnt.size();
    MC_ENSURE(path_off, (np + 1) * 8); MC_ENSURE(path_v, v.size() * 4); MC_ENSURE(path_cnt, np * 8);
    CK(hipMemcpyAsync(g->path_off.p, off.data(), (np + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (np) {
        CK(hipMemcpyAsync(g->path_v.p, v.data(), v.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        CK(hipMemcpyAsync(g->path_cnt.p, cnt.data(), np * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    CK(hipStreamSynchronize(ctx->stream));
    g->cur ^= 1, g->n_aln = na, g->n_path = np, g->n_path_vtx = v.size(), g->done = true;
    return OATK_OK;
}

extern "C" int oatk_hip_ra_minicircle_units(oatk_hip_ctx *ctx, const oatk_racov_aln_t *aln, uint64_t anchor_utg, uint64_t *n_valid, uint64_t *n_path,
                                            uint64_t *n_path_vtx)
{
    using namespace oatk;
    const char *who = "oatk_hip_ra_minicircle_units";
    if (!ctx) return OATK_E_NODEV;
    if (!n_valid || !n_path || !n_path_vtx) { ctx->err = std::string(who) + ": no output"; return OATK_E_ARG; }
    if (anchor_utg >> 31) { ctx->err = std::string(who) + ": the anchor is no unitig id (2^31 or more)"; return OATK_E_ARG; }
    CK(hipSetDevice(ctx->device));
    McState *g = mc_state(ctx);
    McArgs a;
    memset(&a, 0, sizeof(a));
    a.anchor = anchor_utg;
    if (aln) {
        const uint64_t na = aln->n_aln, nf = aln->n_frg;
        if (na && (!aln->off || (nf && !aln->uid))) { ctx->err = std::string(who) + ": no alignments"; return OATK_E_ARG; }
        bool ok = !na || aln->off[0] == 0;
        for (uint64_t i = 0; ok && i < na; ++i) ok = aln->off[i] <= aln->off[i + 1];
        if (!ok || (na && aln->off[na] != nf)) { ctx->err = std::string(who) + ": the alignment offsets do not ascend from 0 to n_frg"; return OATK_E_ARG; }
        MC_ENSURE(a_off, (na + 1) * 8); MC_ENSURE(f_uid, nf * 8);
        if (na) CK(hipMemcpyAsync(g->a_off.p, aln->off, (na + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        if (nf) CK(hipMemcpyAsync(g->f_uid.p, aln->uid, nf * 8, hipMemcpyHostToDevice, ctx->stream));
        a.n_aln = na, a.off = g->a_off.as<uint64_t>(), a.uid = g->f_uid.as<uint64_t>();
    } else {
        RaState *r = ctx->ra;
        if (!r || !r->done) { ctx->err = std::string(who) + ": resident alignments requested before oatk_hip_read_alignment"; return OATK_E_STATE; }
        a.n_aln = r->n_aln, a.off = r->o_off.as<uint64_t>(), a.uid = r->o_uid.as<uint64_t>();
    }
    const uint64_t na = a.n_aln;
    if (na >= 0xFFFFFFFFull) { ctx->err = std::string(who) + ": 2^32 alignment records or more"; return OATK_E_ARG; }
    std::vector<uint64_t> h_off(1, 0), h_cnt;
    std::vector<uint32_t> h_v;
    if (na == 0) {
        *n_valid = *n_path = *n_path_vtx = 0;
        return mc_commit(ctx, g, 0, h_off, h_v, h_cnt);
    }
    for (hipEvent_t &e : g->ev) if (!e) CK(hipEventCreate(&e));
    DevBuf &unit = g->unit[g->cur ^ 1];
    if (!unit.ensure(na * 8 + 64, ctx->stream)) { ctx->err = "hipMalloc failed for minicircle.unit"; return OATK_E_NOMEM; }
    MC_ENSURE(err, 4); MC_ENSURE(n_long, 8); MC_ENSURE(long_idx, na * 4);
    CK(hipMemsetAsync(g->err.p, 0, 4, ctx->stream));
    CK(hipMemsetAsync(g->n_long.p, 0, 8, ctx->stream));
    a.err = g->err.as<unsigned int>();
    unsigned int *n_long = g->n_long.as<unsigned int>();                    // [0] long records, [1] long paths
    const unsigned grid = grid256(na).x < 4096? grid256(na).x : 4096, wgrid = (unsigned) ctx->n_cu * 4;      // the lists are walked by 16 waves per CU
    // (a) every record's unit
    CK(hipEventRecord(g->ev[0], ctx->stream));
    hipLaunchKernelGGL(mc_unit_short_kernel, dim3(grid), dim3(256), 0, ctx->stream, a, unit.as<uint64_t>(), g->long_idx.as<uint32_t>(), n_long);
    hipLaunchKernelGGL(mc_unit_long_kernel, dim3(wgrid), dim3(256), 0, ctx->stream, a, unit.as<uint64_t>(), g->long_idx.as<uint32_t>(), n_long);
    CK(hipEventRecord(g->ev[1], ctx->stream));
    // (b) the valid ones in record order, their paths back to back
    MC_ENSURE(flag, (na + 1) * 8); MC_ENSURE(nv, (na + 1) * 8); MC_ENSURE(pos, (na + 1) * 8); MC_ENSURE(voff, (na + 1) * 8);
    hipLaunchKernelGGL(mc_nv_kernel, grid256(na + 1), dim3(256), 0, ctx->stream, na, unit.as<uint64_t>(), g->flag.as<uint64_t>(), g->nv.as<uint64_t>());
    uint64_t nval = 0, tot = 0;
    { int rc = prim_scan_total(ctx, g->tmp, g->flag.as<uint64_t>(), g->pos.as<uint64_t>(), na, &nval); if (rc) return rc; }
    { int rc = prim_scan_total(ctx, g->tmp, g->nv.as<uint64_t>(), g->voff.as<uint64_t>(), na, &tot); if (rc) return rc; }
    MC_ENSURE(rec, nval * 4); MC_ENSURE(p_off, (nval + 1) * 8); MC_ENSURE(v, tot * 4); MC_ENSURE(key, nval * 8); MC_ENSURE(val, nval * 4);
    hipLaunchKernelGGL(mc_place_kernel, grid256(na + 1), dim3(256), 0, ctx->stream, na, unit.as<uint64_t>(), g->pos.as<uint64_t>(), g->voff.as<uint64_t>(),
                       g->rec.as<uint32_t>(), g->p_off.as<uint64_t>());
    if (nval) {
        const uint64_t mask = oatk_mc::hash_mask(g->hash_bits);
        hipLaunchKernelGGL(mc_path_short_kernel, dim3(grid256(nval).x < 4096? grid256(nval).x : 4096), dim3(256), 0, ctx->stream, a, unit.as<uint64_t>(), nval,
                           g->rec.as<uint32_t>(), g->p_off.as<uint64_t>(), g->v.as<uint32_t>(), g->key.as<uint64_t>(), g->val.as<uint32_t>(), mask,
                           g->long_idx.as<uint32_t>(), n_long + 1);
        hipLaunchKernelGGL(mc_path_long_kernel, dim3(wgrid), dim3(256), 0, ctx->stream, a, unit.as<uint64_t>(), g->rec.as<uint32_t>(), g->p_off.as<uint64_t>(),
                           g->v.as<uint32_t>(), g->key.as<uint64_t>(), mask, g->long_idx.as<uint32_t>(), n_long + 1);
    }
    CK(hipEventRecord(g->ev[2], ctx->stream));
    {
        unsigned int e = 0;
        CK(hipMemcpyAsync(&e, g->err.p, 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        CK(hipGetLastError());
        if (e & MC_ERR_LONG) { ctx->err = std::string(who) + ": an alignment record of 2^31 fragments or more"; return OATK_E_ARG; }
        if (e & MC_ERR_UID) { ctx->err = std::string(who) + ": a repeat unit holds a uid of 2^32 or more (the reference would truncate it)"; return OATK_E_ARG; }
    }
    // (c) the distinct paths and how many records gave each
    uint64_t np = 0, npv = 0;
    g->rounds = 0;
    if (nval) {
        MC_ENSURE(key2, nval * 8); MC_ENSURE(val2, nval * 4); MC_ENSURE(rep, nval * 4); MC_ENSURE(left, nval); MC_ENSURE(cnt, nval * 8); MC_ENSURE(n_sel, 8);
        MC_PRIM(rocprim::radix_sort_pairs, g->key.as<uint64_t>(), g->key2.as<uint64_t>(), g->val.as<uint32_t>(), g->val2.as<uint32_t>(), nval, 0, 64, ctx->stream);
        uint64_t *k_in = g->key2.as<uint64_t>(), *k_out = g->key.as<uint64_t>();
        uint32_t *v_in = g->val2.as<uint32_t>(), *v_out = g->val.as<uint32_t>();
        for (uint64_t n_cur = nval; n_cur; ++g->rounds) {
            hipLaunchKernelGGL(mc_verify_kernel, grid256(n_cur), dim3(256), 0, ctx->stream, n_cur, k_in, v_in, g->p_off.as<uint64_t>(), g->v.as<uint32_t>(),
                               g->rep.as<uint32_t>(), g->left.as<uint8_t>());
            uint64_t n_left = 0, n_left_v = 0;
            { int rc = prim_select(ctx, k_in, g->left.as<uint8_t>(), n_cur, k_out, g->n_sel.as<uint64_t>(), &n_left); if (rc) return rc; }
            if (n_left) { int rc = prim_select(ctx, v_in, g->left.as<uint8_t>(), n_cur, v_out, g->n_sel.as<uint64_t>(), &n_left_v); if (rc) return rc; }
            if (n_left >= n_cur || (n_left && n_left_v != n_left)) { ctx->err = std::string(who) + ": the distinct paths did not settle (internal)"; return OATK_E_STATE; }
            std::swap(k_in, k_out), std::swap(v_in, v_out);
            n_cur = n_left;
        }
        CK(hipMemsetAsync(g->cnt.p, 0, nval * 8, ctx->stream));
        hipLaunchKernelGGL(mc_count_kernel, grid256(nval + 1), dim3(256), 0, ctx->stream, nval, g->rep.as<uint32_t>(), g->p_off.as<uint64_t>(),
                           g->cnt.as<unsigned long long>(), g->flag.as<uint64_t>(), g->nv.as<uint64_t>());
        { int rc = prim_scan_total(ctx, g->tmp, g->flag.as<uint64_t>(), g->pos.as<uint64_t>(), nval, &np); if (rc) return rc; }
        { int rc = prim_scan_total(ctx, g->tmp, g->nv.as<uint64_t>(), g->voff.as<uint64_t>(), nval, &npv); if (rc) return rc; }
        MC_ENSURE(o_off, (np + 1) * 8); MC_ENSURE(o_v, npv * 4); MC_ENSURE(o_cnt, np * 8);
        hipLaunchKernelGGL(mc_gather_kernel, grid256(nval + 1), dim3(256), 0, ctx->stream, nval, g->rep.as<uint32_t>(), g->pos.as<uint64_t>(), g->voff.as<uint64_t>(),
                           g->p_off.as<uint64_t>(), g->v.as<uint32_t>(), g->cnt.as<unsigned long long>(), g->o_off.as<uint64_t>(), g->o_v.as<uint32_t>(),
                           g->o_cnt.as<uint64_t>());
    }
    CK(hipEventRecord(g->ev[3], ctx->stream));
    // the few distinct paths on the host, into path_cmpfunc order (path_finder.c:678)
    std::vector<uint64_t> d_off(np + 1, 0), d_cnt(np);
    std::vector<uint32_t> d_v(npv);
    if (np) {
        CK(hipMemcpyAsync(d_off.data(), g->o_off.p, (np + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipMemcpyAsync(d_cnt.data(), g->o_cnt.p, np * 8, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipMemcpyAsync(d_v.data(), g->o_v.p, npv * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    for (int i = 0; i < 3; ++i) CK(hipEventElapsedTime(&g->ms[i], g->ev[i], g->ev[i + 1]));
    std::vector<uint64_t> order(np);
    std::iota(order.begin(), order.end(), (uint64_t) 0);
    std::sort(order.begin(), order.end(), [&](uint64_t x, uint64_t y) {
        return oatk_mc::path_cmp(d_v.data() + d_off[x], d_off[x + 1] - d_off[x], d_v.data() + d_off[y], d_off[y + 1] - d_off[y]) < 0;
    });
    h_cnt.resize(np);
    h_v.reserve(npv);
    for (uint64_t d = 0; d < np; ++d) {
        const uint64_t x = order[d];
        h_v.insert(h_v.end(), d_v.begin() + d_off[x], d_v.begin() + d_off[x + 1]);
        h_off.push_back(h_v.size()), h_cnt[d] = d_cnt[x];
    }
    { int rc = mc_commit(ctx, g, na, h_off, h_v, h_cnt); if (rc) return rc; }
    *n_valid = nval, *n_path = np, *n_path_vtx = npv;
    return OATK_OK;
}
