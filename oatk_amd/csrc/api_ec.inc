// oatk_amd/csrc/api_ec.inc -- C ABI of the device error correction (include/oatk_hip_ec.h); part of api.hip.
#include "../../include/oatk_hip_ec.h"
#include "ec.hpp"
#include "ec_wave.hpp"
#include "ec_heavy.hpp"
#include "ec_fused.hpp"
#include "ecgraph.hpp"
#include "ec_seq.hpp"
#include <rocprim/iterator/counting_iterator.hpp>

struct EcState {
    DevBuf idx_p, idx_n, arc_v, arc_w, arc_ls, arc_cov, arc_del, conv;   // graph (device copy)
    DevBuf scm_del, err_del, vtx_hs_off, vtx_mpos;
    DevBuf copy_n, seg, keep_all, n_blocks, n_blocks64, blk_off, work, out, path_pool, cursor, todo, todo2, slabs, big_slabs, os_slabs;
    DevBuf qkey, qidx, qtmp[4];   // the solver's queues in source order (ec_queue_sort): keys and sorted lists of a call one behind the other; a side stream's sort has its own temporary
    uint64_t n_live = 0, q_used = 0, qk_used = 0;      // live arcs of the resident marking (the width of a queue key); words of qidx / qkey the call's lists take so far
    DevBuf hyb_slabs[16];         // the hybrid tier's HBM slabs, one buffer per launch of a call (launches may run side by side), sized by the blocks the launch has
    hipStream_t aux[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};       // the larger solver tiers run beside the first one ([4]: of the lowest priority level)
    hipEvent_t aux_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}, fork_ev = nullptr;
    DevBuf new_n, new_n64, new_off, new_k, new_m, new_s, stats;
    DevBuf live32, live64, live_off, larc, lidx_p, lidx_n;               // live arcs (ec_wave.hpp)
    DevBuf cov, fwd, key_id, key_sorted, val_occ, occ, occ_off, cov64;
    uint64_t n_vtx = 0, new_tot = 0;
    uint64_t stats_h[12] = {0};
    uint64_t n_work = 0;
    uint32_t staged_over = 0;           // where the block walk's overflow flag is copied to: a copy queued on the stream may land after the call that queued it has returned on an error
    bool done = false;
    // graph built on the device (ecgraph.hpp)
    DevBuf g_keys, g_keys2, g_ukeys, g_counts, g_nruns, g_nout, g_nout64, g_outoff, g_akey, g_aval, g_skey, g_sval, g_comp, g_flags, g_huge;
    DevBuf g_dist, g_dist2, g_cnt64, g_runoff, g_runls;
    DevBuf g_big, g_keep, g_other, g_lkeys, g_ldist, g_val2, g_wgt2, g_runcov, g_head, g_hpos, g_iota, g_segk, g_segv;   // light graph / weighted segments
    DevBuf g_cbits, g_wcnt, g_wpre, g_candid, g_gcnt, g_gpre;            // light graph on candidate ranks: one bit per vertex, candidates per word and in front of it, the inverse table; kept pairs per workgroup
    uint32_t light_c = 0;               // the resident graph is a light one built for this err_mer_c (0: the full graph)
    uint64_t g_n_vtx = 0, g_n_arc = 0;
    bool graph_resident = false;
    // sharded reads (oatk_hip_ec_set_global): the chains and the graph use GLOBAL syncmer ids
    bool global = false, marked = false;
    uint64_t n_global = 0, imp_used = 0;
    DevBuf g_l2g, g_kid, g_gcov, g_gs;
    // corrected sequences (ec_seq.hpp)
    bool keep_seq = false;              // oatk_hip_ec_keep_seq: the next correction records q_end and the optimum consensus of the blocks it replaces
    bool seq_kept = false, cseq_done = false;      // the resident correction did; oatk_hip_ec_corrected_reads has run on it
    bool seq_global = false;            // the id space that correction was made in (sharded reads: global ids); the strings are built in no other
    DevBuf slot_w, slot_w64, slot_off, slots, qend, sblk, clen, cbytes, cbytes64, coff, cseq;
    uint64_t cseq_bytes = 0;
};

static uint64_t ec_n_vtx(oatk_hip_ctx *ctx) { return ctx->ec && ctx->ec->global? ctx->ec->n_global : ctx->n_scm_total; }
static const uint64_t *ec_chains(oatk_hip_ctx *ctx) { return ctx->ec && ctx->ec->global? ctx->ec->g_kid.as<uint64_t>() : ctx->pos_kid.as<uint64_t>(); }

static void ec_state_free(oatk_hip_ctx *ctx)
{
    if (!ctx->ec) return;
    EcState *e = ctx->ec;
    for (int i = 0; i < 5; ++i) { if (e->aux[i]) (void) hipStreamDestroy(e->aux[i]); if (e->aux_ev[i]) (void) hipEventDestroy(e->aux_ev[i]); }
    if (e->fork_ev) (void) hipEventDestroy(e->fork_ev);
    delete e;
    ctx->ec = nullptr;
}

static int ec_buffer(oatk_hip_ctx *ctx, int which, const void **d_ptr, uint64_t *bytes)
{
    EcState *e = ctx->ec;
    if (e && which >= OATK_BUF_EG_IDX_P && which <= OATK_BUF_EG_OTHER) {
        if (!e->graph_resident) { ctx->err = "EC graph requested before oatk_hip_ec_graph"; return OATK_E_STATE; }
        const uint64_t gv = e->g_n_vtx, ga = e->g_n_arc;
        switch (which) {
            case OATK_BUF_EG_IDX_P: *d_ptr = e->idx_p.p, *bytes = 2 * gv * 8; break;
            case OATK_BUF_EG_IDX_N: *d_ptr = e->idx_n.p, *bytes = 2 * gv * 4; break;
            case OATK_BUF_EG_ARC_V: *d_ptr = e->arc_v.p, *bytes = ga * 8; break;
            case OATK_BUF_EG_ARC_W: *d_ptr = e->arc_w.p, *bytes = ga * 8; break;
            case OATK_BUF_EG_ARC_LS: *d_ptr = e->arc_ls.p, *bytes = ga * 4; break;
            case OATK_BUF_EG_ARC_COV: *d_ptr = e->arc_cov.p, *bytes = ga * 4; break;
            case OATK_BUF_EG_OTHER: *d_ptr = e->g_other.p, *bytes = e->light_c? 2 * gv : 0; break;
            default: *d_ptr = e->g_comp.p, *bytes = ga; break;
        }
        return OATK_OK;
    }
    if (e && (which == OATK_BUF_EC_VTX_SRC || (which == OATK_BUF_EC_ERR_DEL && !e->done))) {
        if (!e->marked) { ctx->err = "vertex sources / marks requested before oatk_hip_ec_mark"; return OATK_E_STATE; }
        if (which == OATK_BUF_EC_VTX_SRC) *d_ptr = e->vtx_hs_off.p, *bytes = e->n_vtx * 8;
        else *d_ptr = e->err_del.p, *bytes = e->n_vtx;
        return OATK_OK;
    }
    if (!e || !e->done) { ctx->err = "unknown buffer id, or error-correction results requested before oatk_hip_ec"; return OATK_E_STATE; }
    if (which == OATK_BUF_EC_BLOCK_WORK) { *d_ptr = e->work.p, *bytes = e->n_work * sizeof(oatk::EcWork); return OATK_OK; }
    if (which == OATK_BUF_EC_BLOCK_OUT) { *d_ptr = e->out.p, *bytes = e->n_work * sizeof(oatk::EcBlockOut); return OATK_OK; }
    if (which == OATK_BUF_EC_BLOCK_QEND) {
        if (!e->seq_kept) { ctx->err = "EC_BLOCK_QEND: the resident correction was made without oatk_hip_ec_keep_seq"; return OATK_E_STATE; }
        *d_ptr = e->qend.p, *bytes = e->n_work * 4;
        return OATK_OK;
    }
    if (which >= OATK_BUF_EC_CSEQ_LEN && which <= OATK_BUF_EC_CSEQ) {
        if (!e->seq_kept || !e->cseq_done) { ctx->err = "corrected sequences requested before oatk_hip_ec_corrected_reads"; return OATK_E_STATE; }
        if (which == OATK_BUF_EC_CSEQ_LEN) *d_ptr = e->clen.p, *bytes = ctx->n_reads * 4;
        else if (which == OATK_BUF_EC_CSEQ_OFF) *d_ptr = e->coff.p, *bytes = (ctx->n_reads + 1) * 8;
        else *d_ptr = e->cseq.p, *bytes = e->cseq_bytes;
        return OATK_OK;
    }
    const uint64_t n = ctx->n_reads, ns = e->n_vtx, tot = e->new_tot;
    switch (which) {
        case OATK_BUF_EC_N_SCM: *d_ptr = e->new_n.p, *bytes = n * 4; break;
        case OATK_BUF_EC_SCM_OFF: *d_ptr = e->new_off.p, *bytes = (n + 1) * 8; break;
        case OATK_BUF_EC_KMER: *d_ptr = e->new_k.p, *bytes = tot * 8; break;
        case OATK_BUF_EC_MPOS: *d_ptr = e->new_m.p, *bytes = tot * 4; break;
        case OATK_BUF_EC_SMER: *d_ptr = e->new_s.p, *bytes = tot * 8; break;
        case OATK_BUF_EC_SCM_COV: *d_ptr = e->cov.p, *bytes = ns * 4; break;
        case OATK_BUF_EC_SCM_DEL: *d_ptr = e->scm_del.p, *bytes = ns; break;
        case OATK_BUF_EC_SCM_OCC_OFF: *d_ptr = e->occ_off.p, *bytes = (ns + 1) * 8; break;
        case OATK_BUF_EC_SCM_OCC: *d_ptr = e->occ.p, *bytes = tot * 8; break;
        case OATK_BUF_EC_ERR_DEL: *d_ptr = e->err_del.p, *bytes = ns; break;
        case OATK_BUF_EC_SCM_FWD: *d_ptr = e->fwd.p, *bytes = ns * 4; break;
        default: ctx->err = "unknown buffer id"; return OATK_E_ARG;
    }
    return OATK_OK;
}

__global__ void ec_narrow_kernel(const uint64_t *in, uint32_t *out, uint64_t n)
{
    uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (uint32_t) in[i];
}
#define EENSURE(buf, bytes, ...) ENSURE_IN(e, "ec.", buf, bytes, ##__VA_ARGS__)

extern "C" int oatk_hip_debug_ec_tiers(oatk_hip_ctx *ctx, int cap_t0, int cap_t1)
{
    if (!ctx) return OATK_E_NODEV;
    if (cap_t0 < 0 || cap_t1 < 0 || (cap_t0 && cap_t1 && cap_t1 < cap_t0)) { ctx->err = "oatk_hip_debug_ec_tiers: 0 <= cap_t0 <= cap_t1"; return OATK_E_ARG; }
    ctx->ec_cap_t0 = cap_t0, ctx->ec_cap_t1 = cap_t1;
    return OATK_OK;
}

// wf_ed_core alone (include/oatk_hip_ec.h): pack the codes sixteen to a word the way the solver holds its strings, one wave per job
static int debug_ed_impl(oatk_hip_ctx *ctx, uint64_t n_jobs, const uint8_t *t_codes, const uint64_t *t_off, const uint8_t *q_codes, const uint64_t *q_off,
                         const int32_t *bw, const int32_t *step_ql, const uint64_t *step_off, int32_t *out3, bool myers, float *kernel_ms, int wg_R = 0,
                         int regroup = 1, uint32_t *turns = nullptr)
{
    using namespace oatk;
    if (!ctx) return OATK_E_NODEV;
    if (n_jobs == 0) return OATK_OK;
    if (n_jobs >= 0x7FFFFFFFULL) { ctx->err = "oatk_hip_debug_wf_ed: too many jobs"; return OATK_E_ARG; }
    CK(hipSetDevice(ctx->device));
    std::vector<uint64_t> tw_off(n_jobs + 1, 0), qw_off(n_jobs + 1, 0), k_off(n_jobs + 1, 0);
    std::vector<int32_t> tl(n_jobs);
    for (uint64_t j = 0; j < n_jobs; ++j) {
        const uint64_t t = t_off[j + 1] - t_off[j], q = q_off[j + 1] - q_off[j];
        if (t == 0 || q == 0 || t > 0x3FFFFFFF || q > 0x3FFFFFFF) { ctx->err = "oatk_hip_debug_wf_ed: empty or oversized string (wf_ed asserts tl > 0 && ql > 0)"; return OATK_E_ARG; }
        for (uint64_t s = step_off[j]; s < step_off[j + 1]; ++s)
            if (step_ql[s] < 1 || (uint64_t) step_ql[s] > q || (s > step_off[j] && step_ql[s] < step_ql[s - 1])) { ctx->err = "oatk_hip_debug_wf_ed: query lengths must ascend within the query"; return OATK_E_ARG; }
        tl[j] = (int32_t) t;
        if (wg_R && (bw[j] >= 0? (uint64_t) 2 * (uint64_t) bw[j] + 3 : t + q + 3) > (wg_R == ECF_NW? (uint64_t) ECF_NW * ECF_OWN : (uint64_t) 64 * ECH_NW * (uint64_t) wg_R)) { ctx->err = "oatk_hip_debug_wf_ed_wg: a job's diagonals do not fit the registers of this variant"; return OATK_E_ARG; }
        tw_off[j + 1] = tw_off[j] + ecw_words((int32_t) t), qw_off[j + 1] = qw_off[j] + ecw_words((int32_t) q);
        k_off[j + 1] = k_off[j] + 2 * (t + q + 8);
    }
    auto pack = [](const uint8_t *codes, const uint64_t *off, const std::vector<uint64_t> &woff, uint64_t n) {
        std::vector<uint32_t> w(woff[n], 0u);
        for (uint64_t j = 0; j < n; ++j)
            for (uint64_t p = 0, len = off[j + 1] - off[j]; p < len; ++p)
                w[woff[j] + (p >> 4)] |= (uint32_t) (codes[off[j] + p] & 3u) << ((p & 15u) << 1);     // field s of word i = base 16 i + s
        return w;
    };
    const std::vector<uint32_t> tw = pack(t_codes, t_off, tw_off, n_jobs), qw = pack(q_codes, q_off, qw_off, n_jobs);
    const uint64_t n_steps = step_off[n_jobs];
    DevBuf d_tw, d_qw, d_two, d_qwo, d_tl, d_bw, d_sq, d_so, d_k, d_ko, d_out, d_slab, d_turns;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (kernel_ms) { *kernel_ms = 0.f; (void) hipEventCreate(&ev0); (void) hipEventCreate(&ev1); }
    int32_t max_t = 0;
    for (uint64_t j = 0; j < n_jobs; ++j) if (tl[j] > max_t) max_t = tl[j];
    const uint64_t n_waves = (n_jobs + 63) / 64, slab_words = (uint64_t) 6 * 64 * (uint64_t) ((max_t + 63) / 64 + 1);
    std::vector<int32_t> ql_last(n_jobs);
    for (uint64_t j = 0; j < n_jobs; ++j) ql_last[j] = step_off[j + 1] > step_off[j]? step_ql[step_off[j + 1] - 1] : (int32_t) (q_off[j + 1] - q_off[j]);
    int rc = OATK_OK;
    hipError_t he = hipSuccess;
    auto up = [&](DevBuf &b, const void *src, size_t bytes) {
        if (rc) return;
        if (!b.ensure(bytes + 16, ctx->stream)) { rc = OATK_E_NOMEM; return; }
        if (bytes && (he = hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess) rc = OATK_E_NODEV;
    };
    up(d_tw, tw.data(), tw.size() * 4); up(d_qw, qw.data(), qw.size() * 4);
    up(d_two, tw_off.data(), (n_jobs + 1) * 8); up(d_qwo, qw_off.data(), (n_jobs + 1) * 8); up(d_ko, k_off.data(), (n_jobs + 1) * 8);
    up(d_tl, tl.data(), n_jobs * 4); up(d_bw, bw, n_jobs * 4); up(d_sq, step_ql, n_steps * 4); up(d_so, step_off, (n_jobs + 1) * 8);
    if (!rc && (!d_k.ensure(k_off[n_jobs] * 4 + 16, ctx->stream) || !d_out.ensure(n_steps * 12 + 16, ctx->stream))) rc = OATK_E_NOMEM;
    if (!rc && turns && !d_turns.ensure(n_jobs * 4 + 16, ctx->stream)) rc = OATK_E_NOMEM;
    if (!rc && myers) {
        if (!d_slab.ensure(n_waves * slab_words * 8 + 64, ctx->stream) || !d_out.ensure(n_jobs * 12 + 16, ctx->stream)) rc = OATK_E_NOMEM;
        up(d_sq, ql_last.data(), n_jobs * 4);                        // (one query length per job: the last one asked for)
    }
    if (!rc) {
        if (ev0) (void) hipEventRecord(ev0, ctx->stream);
#ifdef OATK_EXPERIMENTS
        if (myers)
            hipLaunchKernelGGL(myers_ed_kernel, dim3((unsigned) n_waves), dim3(64), 0, ctx->stream, n_jobs, d_tw.as<uint32_t>(), d_two.as<uint64_t>(), d_tl.as<int32_t>(),
                               d_qw.as<uint32_t>(), d_qwo.as<uint64_t>(), d_sq.as<int32_t>(), d_bw.as<int32_t>(), d_slab.as<uint64_t>(), slab_words, d_out.as<int32_t>());
        else
#endif
        if (wg_R) {
            uint64_t cap_words = 0;
            for (uint64_t j = 0; j < n_jobs; ++j) { if (tw_off[j + 1] - tw_off[j] > cap_words) cap_words = tw_off[j + 1] - tw_off[j]; if (qw_off[j + 1] - qw_off[j] > cap_words) cap_words = qw_off[j + 1] - qw_off[j]; }
            const uint64_t lds = ((uint64_t) ech_misc_words(wg_R) + 2 * cap_words) * 4;
            if (lds > 64 * 1024 || (wg_R != 1 && wg_R != 2 && wg_R != 6 && wg_R != ECF_NW)) { ctx->err = "oatk_hip_debug_wf_ed_wg: strings too long for LDS, or no such variant (1, 2, 6, 16)"; rc = OATK_E_ARG; }
            else if (wg_R == ECF_NW) hipLaunchKernelGGL((ecf_wf_ed_kernel<ECF_NW>), dim3((unsigned) n_jobs), dim3(64 * ECF_NW), (unsigned) (((uint64_t) ecf_misc_words(ECF_NW) + 2 * cap_words) * 4), ctx->stream, d_tw.as<uint32_t>(), d_two.as<uint64_t>(), d_tl.as<int32_t>(),
                                                         d_qw.as<uint32_t>(), d_qwo.as<uint64_t>(), d_bw.as<int32_t>(), d_sq.as<int32_t>(), d_so.as<uint64_t>(), d_out.as<int32_t>(), (int32_t) cap_words);
            else if (wg_R == 1) hipLaunchKernelGGL((ech_wf_ed_kernel<ECH_NW, 1>), dim3((unsigned) n_jobs), dim3(64 * ECH_NW), (unsigned) lds, ctx->stream, d_tw.as<uint32_t>(), d_two.as<uint64_t>(), d_tl.as<int32_t>(),
                                                    d_qw.as<uint32_t>(), d_qwo.as<uint64_t>(), d_bw.as<int32_t>(), d_sq.as<int32_t>(), d_so.as<uint64_t>(), d_out.as<int32_t>(), (int32_t) cap_words);
            else if (wg_R == 2) hipLaunchKernelGGL((ech_wf_ed_kernel<ECH_NW, 2>), dim3((unsigned) n_jobs), dim3(64 * ECH_NW), (unsigned) lds, ctx->stream, d_tw.as<uint32_t>(), d_two.as<uint64_t>(), d_tl.as<int32_t>(),
                                                    d_qw.as<uint32_t>(), d_qwo.as<uint64_t>(), d_bw.as<int32_t>(), d_sq.as<int32_t>(), d_so.as<uint64_t>(), d_out.as<int32_t>(), (int32_t) cap_words);
            else hipLaunchKernelGGL((ech_wf_ed_kernel<ECH_NW, 6>), dim3((unsigned) n_jobs), dim3(64 * ECH_NW), (unsigned) lds, ctx->stream, d_tw.as<uint32_t>(), d_two.as<uint64_t>(), d_tl.as<int32_t>(),
                                    d_qw.as<uint32_t>(), d_qwo.as<uint64_t>(), d_bw.as<int32_t>(), d_sq.as<int32_t>(), d_so.as<uint64_t>(), d_out.as<int32_t>(), (int32_t) cap_words);
        } else
        hipLaunchKernelGGL(ecw_wf_ed_kernel, dim3((unsigned) n_jobs), dim3(64), 0, ctx->stream, d_tw.as<uint32_t>(), d_two.as<uint64_t>(), d_tl.as<int32_t>(),
                           d_qw.as<uint32_t>(), d_qwo.as<uint64_t>(), d_bw.as<int32_t>(), d_sq.as<int32_t>(), d_so.as<uint64_t>(), d_k.as<int32_t>(),
                           d_ko.as<uint64_t>(), d_out.as<int32_t>(), (int32_t) regroup, turns? d_turns.as<uint32_t>() : (uint32_t *) nullptr);
        if (ev1) (void) hipEventRecord(ev1, ctx->stream);
        const uint64_t n_out = myers? n_jobs : n_steps;
        if (n_out && (he = hipMemcpyAsync(out3, d_out.p, n_out * 12, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) rc = OATK_E_NODEV;
        if (!rc && turns && (he = hipMemcpyAsync(turns, d_turns.p, n_jobs * 4, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) rc = OATK_E_NODEV;
        if ((he = hipStreamSynchronize(ctx->stream)) != hipSuccess) rc = OATK_E_NODEV;
        if (!rc && (he = hipGetLastError()) != hipSuccess) rc = OATK_E_NODEV;
    }
    (void) hipStreamSynchronize(ctx->stream);
    if (ev0 && ev1 && !rc) (void) hipEventElapsedTime(kernel_ms, ev0, ev1);
    if (ev0) (void) hipEventDestroy(ev0);
    if (ev1) (void) hipEventDestroy(ev1);
    if (rc == OATK_E_NODEV) ctx->err = std::string("oatk_hip_debug_wf_ed: ") + hipGetErrorString(he);
    if (rc == OATK_E_NOMEM) ctx->err = "oatk_hip_debug_wf_ed: hipMalloc failed";
    return rc;
}

extern "C" int oatk_hip_debug_wf_ed(oatk_hip_ctx *ctx, uint64_t n_jobs, const uint8_t *t_codes, const uint64_t *t_off, const uint8_t *q_codes, const uint64_t *q_off,
                                    const int32_t *bw, const int32_t *step_ql, const uint64_t *step_off, int32_t *out3)
{
    float ms = 0.f;
    const bool timed = getenv("OATK_DEBUG_ED_TIME") != nullptr;
    const int rc = debug_ed_impl(ctx, n_jobs, t_codes, t_off, q_codes, q_off, bw, step_ql, step_off, out3, false, timed? &ms : nullptr);
    if (timed) fprintf(stderr, "[wf_ed_wg] R 0: %llu jobs, kernel %.3f ms\n", (unsigned long long) n_jobs, ms);
    return rc;
}

// ecw_step with its lanes regrouped (regroup != 0, what ships) or not, and the extension turns every job took (include/oatk_hip_ec.h)
extern "C" int oatk_hip_debug_wf_ed_turns(oatk_hip_ctx *ctx, int regroup, uint64_t n_jobs, const uint8_t *t_codes, const uint64_t *t_off, const uint8_t *q_codes, const uint64_t *q_off,
                                          const int32_t *bw, const int32_t *step_ql, const uint64_t *step_off, int32_t *out3, uint32_t *turns)
{
    if (!turns) { if (ctx) ctx->err = "oatk_hip_debug_wf_ed_turns: turns is null"; return OATK_E_ARG; }
    return debug_ed_impl(ctx, n_jobs, t_codes, t_off, q_codes, q_off, bw, step_ql, step_off, out3, false, nullptr, 0, regroup != 0, turns);
}

// the refreshed table's coverage, forward counts and marks from sorted (key, occurrence) pairs on their own (include/oatk_hip_ec.h)
extern "C" int oatk_hip_debug_cov_runs(oatk_hip_ctx *ctx, uint64_t n, const uint32_t *key_sorted, const uint64_t *occ, uint64_t nv, uint32_t *cov, uint32_t *fwd, uint8_t *del)
{
    using namespace oatk;
    if (!ctx) return OATK_E_NODEV;
    if (!nv || n >= 0xFFFFFFFFULL) { ctx->err = "oatk_hip_debug_cov_runs: no keys, or too many entries"; return OATK_E_ARG; }
    for (uint64_t i = 0; i < n; ++i)
        if (key_sorted[i] >= nv || (i && key_sorted[i] < key_sorted[i - 1])) { ctx->err = "oatk_hip_debug_cov_runs: keys must ascend and lie below nv"; return OATK_E_ARG; }
    CK(hipSetDevice(ctx->device));
    DevBuf d_key, d_occ, d_cov, d_fwd, d_del;
    if (!d_key.ensure(n * 4 + 16, ctx->stream) || !d_occ.ensure(n * 8 + 16, ctx->stream) || !d_cov.ensure(nv * 4 + 16, ctx->stream) ||
        !d_fwd.ensure(nv * 4 + 16, ctx->stream) || !d_del.ensure(nv + 16, ctx->stream)) { ctx->err = "oatk_hip_debug_cov_runs: hipMalloc failed"; return OATK_E_NOMEM; }
    if (n) { CK(hipMemcpyAsync(d_key.p, key_sorted, n * 4, hipMemcpyHostToDevice, ctx->stream)); CK(hipMemcpyAsync(d_occ.p, occ, n * 8, hipMemcpyHostToDevice, ctx->stream)); }
    CK(hipMemsetAsync(d_cov.p, 0, nv * 4, ctx->stream));
    CK(hipMemsetAsync(d_fwd.p, 0, nv * 4, ctx->stream));
    if (n) hipLaunchKernelGGL(ec_cov_runs_kernel, grid256(n), dim3(256), 0, ctx->stream, n, d_key.as<uint32_t>(), d_occ.as<uint64_t>(), d_cov.as<uint32_t>(), d_fwd.as<uint32_t>());
    hipLaunchKernelGGL(ec_del_kernel, grid256(nv), dim3(256), 0, ctx->stream, nv, d_fwd.as<uint32_t>(), d_del.as<uint8_t>());
    CK(hipMemcpyAsync(cov, d_cov.p, nv * 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(fwd, d_fwd.p, nv * 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(del, d_del.p, nv, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    return OATK_OK;
}

// the same through the workgroup solver's step (ec_heavy.hpp: ech_step, R = 1, 2 or 6 diagonals per lane); a job whose diagonals do not fit is refused
// the two tables of a long arc on their own (include/oatk_hip_ec.h; ec_rows.hpp: ecb_table)
extern "C" int oatk_hip_debug_tables(oatk_hip_ctx *ctx, uint64_t n_jobs, const uint8_t *t_codes, const uint64_t *t_off, const uint8_t *s_codes, const uint64_t *s_off, int32_t *out, const uint64_t *out_off)
{
    using namespace oatk;
    if (!ctx) return OATK_E_NODEV;
    if (n_jobs == 0) return OATK_OK;
    if (n_jobs >= 0x7FFFFFFFULL) { ctx->err = "oatk_hip_debug_tables: too many jobs"; return OATK_E_ARG; }
    CK(hipSetDevice(ctx->device));
    std::vector<uint64_t> tw_off(n_jobs + 1, 0), qw_off(n_jobs + 1, 0);
    std::vector<int32_t> tl(n_jobs), ql(n_jobs);
    uint64_t cap_words = 0;
    for (uint64_t j = 0; j < n_jobs; ++j) {
        const uint64_t t = t_off[j + 1] - t_off[j], q = s_off[j + 1] - s_off[j];
        if (t == 0 || q == 0 || t > 0x3FFFFFFF || q > 1024) { ctx->err = "oatk_hip_debug_tables: an empty string, or one of more than 1024 bases"; return OATK_E_ARG; }
        if (out_off[j + 1] - out_off[j] < 2 * (t + 1)) { ctx->err = "oatk_hip_debug_tables: a job's output holds 2 (tl + 1) numbers"; return OATK_E_ARG; }
        tl[j] = (int32_t) t, ql[j] = (int32_t) q;
        tw_off[j + 1] = tw_off[j] + ecw_words((int32_t) t), qw_off[j + 1] = qw_off[j] + ecw_words((int32_t) q);
        if (tw_off[j + 1] - tw_off[j] > cap_words) cap_words = tw_off[j + 1] - tw_off[j];
        if (qw_off[j + 1] - qw_off[j] > cap_words) cap_words = qw_off[j + 1] - qw_off[j];
    }
    if (2 * cap_words * 4 > 64 * 1024) { ctx->err = "oatk_hip_debug_tables: strings too long for LDS"; return OATK_E_ARG; }
    auto pack = [](const uint8_t *codes, const uint64_t *off, const std::vector<uint64_t> &woff, uint64_t n) {
        std::vector<uint32_t> w(woff[n], 0u);
        for (uint64_t j = 0; j < n; ++j)
            for (uint64_t p = 0, len = off[j + 1] - off[j]; p < len; ++p)
                w[woff[j] + (p >> 4)] |= (uint32_t) (codes[off[j] + p] & 3u) << ((p & 15u) << 1);
        return w;
    };
    const std::vector<uint32_t> tw = pack(t_codes, t_off, tw_off, n_jobs), qw = pack(s_codes, s_off, qw_off, n_jobs);
    DevBuf d_tw, d_qw, d_two, d_qwo, d_tl, d_ql, d_oo, d_out;
    int rc = OATK_OK;
    hipError_t he = hipSuccess;
    auto up = [&](DevBuf &b, const void *src, size_t bytes) {
        if (rc) return;
        if (!b.ensure(bytes + 16, ctx->stream)) { rc = OATK_E_NOMEM; return; }
        if (bytes && (he = hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess) rc = OATK_E_NODEV;
    };
    up(d_tw, tw.data(), tw.size() * 4); up(d_qw, qw.data(), qw.size() * 4);
    up(d_two, tw_off.data(), (n_jobs + 1) * 8); up(d_qwo, qw_off.data(), (n_jobs + 1) * 8);
    up(d_tl, tl.data(), n_jobs * 4); up(d_ql, ql.data(), n_jobs * 4); up(d_oo, out_off, (n_jobs + 1) * 8);
    const uint64_t n_out = out_off[n_jobs];
    if (!rc && !d_out.ensure(n_out * 4 + 16, ctx->stream)) rc = OATK_E_NOMEM;
    if (!rc) {
        // OATK_DEBUG_TABLES_SEG="<waves>:<cut>" (tests): the tables as the second stage of the solver builds them -- by 2, 4, 8 or 16 waves, table 0 in stretches that are exact up
        // to `cut`, table 1 only where it can be below it (entries that are not written come back as -1)
        int seg_nw = 1, seg_cut = 0;
        { const char *ev = getenv("OATK_DEBUG_TABLES_SEG"); if (ev && sscanf(ev, "%d:%d", &seg_nw, &seg_cut) != 2) seg_nw = 1, seg_cut = 0; }
        if (n_out && (he = hipMemsetAsync(d_out.p, 0xFF, n_out * 4, ctx->stream)) != hipSuccess) rc = OATK_E_NODEV;
#define OATK_TABLES_LAUNCH(NW) hipLaunchKernelGGL((ecb_tables_kernel<NW>), dim3((unsigned) n_jobs), dim3(64 * NW), (unsigned) (2 * cap_words * 4), ctx->stream, d_tw.as<uint32_t>(), d_two.as<uint64_t>(), d_tl.as<int32_t>(), \
                           d_qw.as<uint32_t>(), d_qwo.as<uint64_t>(), d_ql.as<int32_t>(), d_out.as<int32_t>(), d_oo.as<uint64_t>(), (int32_t) cap_words, (int32_t) seg_cut)
        if (seg_nw == 2) OATK_TABLES_LAUNCH(2); else if (seg_nw == 4) OATK_TABLES_LAUNCH(4); else if (seg_nw == 8) OATK_TABLES_LAUNCH(8); else if (seg_nw == 16) OATK_TABLES_LAUNCH(16); else OATK_TABLES_LAUNCH(1);
#undef OATK_TABLES_LAUNCH
        if (n_out && (he = hipMemcpyAsync(out, d_out.p, n_out * 4, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) rc = OATK_E_NODEV;
        if ((he = hipStreamSynchronize(ctx->stream)) != hipSuccess) rc = OATK_E_NODEV;
        if (!rc && (he = hipGetLastError()) != hipSuccess) rc = OATK_E_NODEV;
    }
    (void) hipStreamSynchronize(ctx->stream);
    if (rc == OATK_E_NODEV) ctx->err = std::string("oatk_hip_debug_tables: ") + hipGetErrorString(he);
    if (rc == OATK_E_NOMEM) ctx->err = "oatk_hip_debug_tables: hipMalloc failed";
    return rc;
}

extern "C" int oatk_hip_debug_wf_ed_wg(oatk_hip_ctx *ctx, int R, uint64_t n_jobs, const uint8_t *t_codes, const uint64_t *t_off, const uint8_t *q_codes, const uint64_t *q_off,
                                       const int32_t *bw, const int32_t *step_ql, const uint64_t *step_off, int32_t *out3)
{
    if (R != 1 && R != 2 && R != 6 && R != ECF_NW) { if (ctx) ctx->err = "oatk_hip_debug_wf_ed_wg: R must be 1, 2, 6 (a workgroup per wavefront) or 16 (several steps per barrier: sixteen waves, 896 diagonals)"; return OATK_E_ARG; }
    float ms = 0.f;
    const bool timed = getenv("OATK_DEBUG_ED_TIME") != nullptr;          // (tools/stepbench.py: the kernel's duration on stderr)
    const int rc = debug_ed_impl(ctx, n_jobs, t_codes, t_off, q_codes, q_off, bw, step_ql, step_off, out3, false, timed? &ms : nullptr, R);
    if (timed) fprintf(stderr, "[wf_ed_wg] R %d: %llu jobs, kernel %.3f ms\n", R, (unsigned long long) n_jobs, ms);
    return rc;
}

#ifdef OATK_EXPERIMENTS
// the A/B of SURVEY.md 7-5: the same jobs (one query length each: the last of its steps) through the wavefront routine (myers = 0) or through Myers'
// bit-vector algorithm, one lane per pair (myers = 1); out3 has one triple per JOB, *kernel_ms the duration of the one kernel (HIP events)
extern "C" int oatk_hip_debug_ed_ab(oatk_hip_ctx *ctx, int myers, uint64_t n_jobs, const uint8_t *t_codes, const uint64_t *t_off, const uint8_t *q_codes,
                                    const uint64_t *q_off, const int32_t *bw, int32_t *out3, float *kernel_ms)
{
    if (!ctx) return OATK_E_NODEV;
    std::vector<int32_t> ql(n_jobs);
    std::vector<uint64_t> so(n_jobs + 1);
    for (uint64_t j = 0; j < n_jobs; ++j) ql[j] = (int32_t) (q_off[j + 1] - q_off[j]), so[j] = j;
    so[n_jobs] = n_jobs;
    return debug_ed_impl(ctx, n_jobs, t_codes, t_off, q_codes, q_off, bw, ql.data(), so.data(), out3, myers != 0, kernel_ms);
}
#endif

extern "C" int oatk_hip_ec_stats(oatk_hip_ctx *ctx, uint64_t *stats12)
{
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->ec || !ctx->ec->done) { ctx->err = "oatk_hip_ec has not run"; return OATK_E_STATE; }
    for (int i = 0; i < 12; ++i) stats12[i] = ctx->ec->stats_h[i];
    return OATK_OK;
}

// sharded reads: from now on the chains of this batch and the EC graph are in global syncmer ids (include/oatk_hip_ec.h)
extern "C" int oatk_hip_ec_set_global(oatk_hip_ctx *ctx, uint64_t n_global, const uint32_t *d_l2g, const uint32_t *d_cov, const uint64_t *d_s)
{
    using namespace oatk;
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->counted) { ctx->err = "oatk_hip_ec_set_global needs a resident scan + count"; return OATK_E_STATE; }
    CK(hipSetDevice(ctx->device));
    if (!ctx->ec) ctx->ec = new EcState();
    EcState *e = ctx->ec;
    e->graph_resident = false, e->done = false, e->marked = false, e->imp_used = 0;
    if (n_global == 0) { e->global = false, e->n_global = 0; return OATK_OK; }
    if (n_global < ctx->n_scm_total || n_global >= 0x7FFFFFFFULL) { ctx->err = "oatk_hip_ec_set_global: bad global table size"; return OATK_E_ARG; }
    const uint64_t nl = ctx->n_scm_total, nocc = ctx->n_occ;
    EENSURE(g_l2g, (nl + 1) * 4); EENSURE(g_gcov, (n_global + 1) * 4); EENSURE(g_gs, (n_global + 1) * 8); EENSURE(g_kid, (nocc + 1) * 8);
    CK(hipMemcpyAsync(e->g_l2g.p, d_l2g, nl * 4, hipMemcpyDeviceToDevice, ctx->stream));
    CK(hipMemcpyAsync(e->g_gcov.p, d_cov, n_global * 4, hipMemcpyDeviceToDevice, ctx->stream));
    CK(hipMemcpyAsync(e->g_gs.p, d_s, n_global * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (nocc) hipLaunchKernelGGL(ec_remap_kernel, dim3((unsigned) ((nocc + 255) / 256)), dim3(256), 0, ctx->stream, nocc, ctx->pos_kid.as<uint64_t>(),
                                 e->g_l2g.as<uint32_t>(), e->g_kid.as<uint64_t>());
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    e->global = true, e->n_global = n_global;
    return OATK_OK;
}

// canonical key + distance of every pair of syncmers adjacent on a read of this batch, in (read, slot) order (ecgraph.hpp)
extern "C" int oatk_hip_ec_pairs(oatk_hip_ctx *ctx, const void **d_keys, const void **d_dist, uint64_t *n_pairs)
{
    using namespace oatk;
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->counted) { ctx->err = "oatk_hip_ec_pairs needs a resident scan + count"; return OATK_E_STATE; }
    CK(hipSetDevice(ctx->device));
    if (!ctx->ec) ctx->ec = new EcState();
    EcState *e = ctx->ec;
    const uint64_t nr = ctx->n_reads, nocc = ctx->n_occ;
    EENSURE(g_keys, (nocc + 1) * 8); EENSURE(g_dist, (nocc + 1) * 4);
    if (nocc) hipLaunchKernelGGL(egr_pair_keys_kernel, dim3((unsigned) ((nr + 255) / 256)), dim3(256), 0, ctx->stream, nr, ctx->scm_off.as<uint64_t>(),
                                 ec_chains(ctx), ctx->pos_mpos.as<uint32_t>(), e->g_keys.as<uint64_t>(), e->g_dist.as<uint32_t>(), 0);
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    *d_keys = e->g_keys.p, *d_dist = e->g_dist.p, *n_pairs = nocc;
    return OATK_OK;
}

// make_syncmer_graph(sr_db, scm_db, 0, 0.) + the arc overlaps of scg_consensus(hoco) from a list of adjacent pairs (ecgraph.hpp).
// The list is this batch's own (oatk_hip_ec_graph) or, with sharded reads, the lists of all shards in shard order.  Entries are single
// pairs (d_dist) or weighted segments (d_val = distance | calls << 32: that many consecutive pairs of one key and one distance).
// The light graph on candidate ranks (ec_light_packed) enters with its keys already packed: `pk` names them (d_keys is null).  They are sorted and
// run-length encoded in that form, the distinct ones are written to g_ukeys as keys on vertex ids, and from there on nothing differs.
struct EgrPacked { void *keys; uint32_t B; bool wide; const uint32_t *cand_id; };      // keys: uint32_t, or uint64_t when wide; ra << B | rb (ecgraph.hpp)

static int ec_graph_build(oatk_hip_ctx *ctx, const uint64_t *d_keys, const uint32_t *d_dist, const uint64_t *d_val, uint64_t nocc, bool timer_running = false,
                          const EgrPacked *pk = nullptr)
{
    using namespace oatk;
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->counted) { ctx->err = "oatk_hip_ec_graph needs a resident scan + count"; return OATK_E_STATE; }
    CK(hipSetDevice(ctx->device));
    if (!ctx->ec) ctx->ec = new EcState();
    EcState *e = ctx->ec;
    e->graph_resident = false, e->marked = false, e->light_c = 0;
    const bool weighted = d_val != nullptr;
    if (nocc >= 0xFFFFFFFFULL) { ctx->err = "more than 2^32 adjacent pairs"; return OATK_E_ARG; }
    const uint64_t nv = ec_n_vtx(ctx);
    if (nv >= 0x7FFFFFFFULL) { ctx->err = "too many syncmers for 32-bit oriented vertex ids"; return OATK_E_ARG; }
    EENSURE(g_flags, 64);
    if (!timer_running) t_begin(ctx, OATK_T_EC_GRAPH);
    CK(hipMemsetAsync(e->g_flags.p, 0, 64, ctx->stream));
    EENSURE(idx_p, (2 * nv + 1) * 8); EENSURE(idx_n, (2 * nv + 1) * 4);
    CK(hipMemsetAsync(e->idx_p.p, 0, (2 * nv + 1) * 8, ctx->stream));
    CK(hipMemsetAsync(e->idx_n.p, 0, (2 * nv + 1) * 4, ctx->stream));
    uint64_t na = 0;
    if (nocc) {
        // 1. canonical keys of adjacent pairs, sorted, run-length encoded = the arc counter of syncasm.c:242-261
        EENSURE(g_keys2, (nocc + 1) * 8); EENSURE(g_ukeys, (nocc + 1) * 8); EENSURE(g_counts, (nocc + 1) * 4);
        EENSURE(g_nruns, 64); EENSURE(g_dist2, (nocc + 1) * 4);
        uint64_t *keys_in = const_cast<uint64_t *>(d_keys);
        uint32_t *dist_in = const_cast<uint32_t *>(d_dist);
        uint32_t *counts = e->g_counts.as<uint32_t>(), *d_nruns = e->g_nruns.as<uint32_t>();
        int rc = OATK_OK;       // the sorts are stable: the distances of one key stay in (read, slot) order
        if (weighted) {         // (the segments' values are split between the sort and the runs, so the two steps are spelt out)
            EENSURE(g_val2, (nocc + 1) * 8); EENSURE(g_wgt2, (nocc + 1) * 4);
            uint64_t *val_in = const_cast<uint64_t *>(d_val);
            PRIM(rocprim::radix_sort_pairs, keys_in, e->g_keys2.as<uint64_t>(), val_in, e->g_val2.as<uint64_t>(), nocc, 0, 64, ctx->stream);
            hipLaunchKernelGGL(egr_seg_split_kernel, grid256(nocc), dim3(256), 0, ctx->stream, nocc, e->g_val2.as<uint64_t>(), e->g_dist2.as<uint32_t>(), e->g_wgt2.as<uint32_t>());
            PRIM(rocprim::run_length_encode, e->g_keys2.as<uint64_t>(), (unsigned int) nocc, e->g_ukeys.as<uint64_t>(), counts, d_nruns, ctx->stream);
        }
        // packed keys: from bit 0 (DESIGN.md 6: rocPRIM's small-input paths and ranges that start higher); the distinct keys go where the unsorted ones were
        else if (pk && pk->wide) rc = prim_sort_runs(ctx, (uint64_t *) pk->keys, e->g_keys2.as<uint64_t>(), dist_in, e->g_dist2.as<uint32_t>(), nocc, 0, 2 * pk->B, (uint64_t *) pk->keys, counts, d_nruns);
        else if (pk) rc = prim_sort_runs(ctx, (uint32_t *) pk->keys, e->g_keys2.as<uint32_t>(), dist_in, e->g_dist2.as<uint32_t>(), nocc, 0, 2 * pk->B, (uint32_t *) pk->keys, counts, d_nruns);
        else rc = prim_sort_runs(ctx, keys_in, e->g_keys2.as<uint64_t>(), dist_in, e->g_dist2.as<uint32_t>(), nocc, 0, 64, e->g_ukeys.as<uint64_t>(), counts, d_nruns);
        if (rc) return rc;
        uint32_t n_runs = 0;
        CK(hipMemcpyAsync(&n_runs, e->g_nruns.p, 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        if (pk && n_runs) {
            if (pk->wide) hipLaunchKernelGGL(egr_unpack_keys_kernel<uint64_t>, grid256(n_runs), dim3(256), 0, ctx->stream, (uint64_t) n_runs, (const uint64_t *) pk->keys, pk->B, pk->cand_id, e->g_ukeys.as<uint64_t>());
            else hipLaunchKernelGGL(egr_unpack_keys_kernel<uint32_t>, grid256(n_runs), dim3(256), 0, ctx->stream, (uint64_t) n_runs, (const uint32_t *) pk->keys, pk->B, pk->cand_id, e->g_ukeys.as<uint64_t>());
        }
        // 2. every distinct key becomes an arc and (unless it is its own) the complementary arc, syncasm.c:264-282
        EENSURE(g_nout, ((uint64_t) n_runs + 1) * 4);
        hipLaunchKernelGGL(egr_expand_count_kernel, grid256(n_runs), dim3(256), 0, ctx->stream, (uint64_t) n_runs, e->g_ukeys.as<uint64_t>(), e->g_nout.as<uint32_t>());
        { int rc = prim_scan_total_u32(ctx, e->g_nout, e->g_nout64, e->g_outoff, n_runs, &na); if (rc) return rc; }
        // the overlap of each key's arc: K - the most frequent distance of its run (syncasm.c:793-812)
        uint64_t chk = 0;
        EENSURE(g_runls, ((uint64_t) n_runs + 1) * 4); EENSURE(g_runcov, ((uint64_t) n_runs + 1) * 4);
        { int rc = prim_scan_total_u32(ctx, e->g_counts, e->g_cnt64, e->g_runoff, n_runs, &chk); if (rc) return rc; }
        if (n_runs) {
            EENSURE(g_big, ((uint64_t) n_runs + 1) * 8);                     // the list of long runs, and behind it the list of runs with more than 48 distinct distances
            EENSURE(g_huge, EGR_HUGE_SCRATCH);
            const uint32_t *wg = weighted? e->g_wgt2.as<uint32_t>() : (const uint32_t *) nullptr;
            uint32_t *rc_ = weighted? e->g_runcov.as<uint32_t>() : (uint32_t *) nullptr;
            hipLaunchKernelGGL(egr_mode_kernel, dim3((n_runs + 63) / 64), dim3(64), 0, ctx->stream, (uint64_t) n_runs, e->g_ukeys.as<uint64_t>(),
                               e->g_counts.as<uint32_t>(), e->g_runoff.as<uint64_t>(), e->g_dist2.as<uint32_t>(), ctx->K, e->g_runls.as<uint32_t>(),
                               e->g_flags.as<uint32_t>(), e->g_big.as<uint32_t>(), e->g_big.as<uint32_t>() + n_runs + 1, wg, rc_);
            hipLaunchKernelGGL(egr_mode_big_kernel, dim3(n_runs < 8192u? n_runs : 8192u), dim3(64), 0, ctx->stream, e->g_counts.as<uint32_t>(), e->g_runoff.as<uint64_t>(),
                               e->g_dist2.as<uint32_t>(), ctx->K, e->g_runls.as<uint32_t>(), e->g_flags.as<uint32_t>(), e->g_big.as<uint32_t>(),
                               e->g_big.as<uint32_t>() + n_runs + 1, wg, rc_);
            hipLaunchKernelGGL(egr_mode_huge_kernel, dim3(1024), dim3(64), 0, ctx->stream, e->g_counts.as<uint32_t>(), e->g_runoff.as<uint64_t>(),
                               e->g_dist2.as<uint32_t>(), ctx->K, e->g_runls.as<uint32_t>(), e->g_flags.as<uint32_t>(), e->g_big.as<uint32_t>() + n_runs + 1,
                               e->g_huge.as<uint8_t>(), (uint64_t) EGR_HUGE_SCRATCH, wg, rc_);
        }
        EENSURE(g_akey, (na + 1) * 8); EENSURE(g_aval, (na + 1) * 8); EENSURE(g_skey, (na + 1) * 8); EENSURE(g_sval, (na + 1) * 8);
        if (na) {
            hipLaunchKernelGGL(egr_expand_kernel, grid256(n_runs), dim3(256), 0, ctx->stream, (uint64_t) n_runs, e->g_ukeys.as<uint64_t>(),
                               weighted? e->g_runcov.as<uint32_t>() : e->g_counts.as<uint32_t>(), e->g_runls.as<uint32_t>(), e->g_outoff.as<uint64_t>(), e->g_akey.as<uint64_t>(), e->g_aval.as<uint64_t>());
            // 3. (v, w) order, asmg_arc_sort graph.c:70-83
            PRIM(rocprim::radix_sort_pairs, e->g_akey.as<uint64_t>(), e->g_skey.as<uint64_t>(), e->g_aval.as<uint64_t>(), e->g_sval.as<uint64_t>(), na, 0, 64, ctx->stream);
        }
    }
    EENSURE(arc_v, (na + 1) * 8); EENSURE(arc_w, (na + 1) * 8); EENSURE(arc_ls, (na + 1) * 4); EENSURE(arc_cov, (na + 1) * 4); EENSURE(arc_del, na + 8);
    EENSURE(g_comp, na + 8);
    EgrArcs a;
    a.n_arc = na, a.arc_v = e->arc_v.as<uint64_t>(), a.arc_w = e->arc_w.as<uint64_t>(), a.arc_ls = e->arc_ls.as<uint32_t>(), a.arc_cov = e->arc_cov.as<uint32_t>();
    a.arc_comp = e->g_comp.as<uint8_t>(), a.arc_del = e->arc_del.as<uint8_t>(), a.idx_p = e->idx_p.as<uint64_t>(), a.idx_n = e->idx_n.as<uint32_t>();
    a.flags = e->g_flags.as<uint32_t>();
    if (na) {
        hipLaunchKernelGGL(egr_unpack_kernel, grid256(na), dim3(256), 0, ctx->stream, a, (const uint64_t *) e->g_skey.p, (const uint64_t *) e->g_sval.p);
    }
    uint32_t fl[4] = {0, 0, 0, 0};
    CK(hipMemcpyAsync(fl, e->g_flags.p, sizeof(fl), hipMemcpyDeviceToHost, ctx->stream));
    t_end(ctx, OATK_T_EC_GRAPH);
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    t_collect(ctx, OATK_T_EC_GRAPH, OATK_T_EC_GRAPH);
    if (fl[0]) { ctx->err = "EC graph has duplicate arcs (a syncmer adjacent to itself on both strands): the reference's order is unspecified"; return OATK_E_SPLIT; }
    if (fl[1]) { ctx->err = "EC graph: the arcs with more than 48 distinct syncmer distances need more than the 256 MB of working memory set aside for them"; return OATK_E_SPLIT; }
    if (debug_refuse(ctx, 1, "oatk_hip_ec_graph")) return OATK_E_SPLIT;
    e->g_n_vtx = nv, e->g_n_arc = na;
    e->graph_resident = true;
    return OATK_OK;
}

extern "C" int oatk_hip_ec_graph_from_pairs(oatk_hip_ctx *ctx, const uint64_t *d_keys, const uint32_t *d_dist, uint64_t nocc)
{
    return ec_graph_build(ctx, d_keys, d_dist, nullptr, nocc);
}

extern "C" int oatk_hip_ec_graph_from_segments(oatk_hip_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_val, uint64_t n_seg)
{
    if (ctx && !d_val && n_seg) { ctx->err = "oatk_hip_ec_graph_from_segments: no segment values"; return OATK_E_ARG; }
    return ec_graph_build(ctx, d_keys, nullptr, d_val? d_val : (const uint64_t *) d_keys, n_seg);
}

extern "C" int oatk_hip_ec_graph(oatk_hip_ctx *ctx)
{
    const void *k = nullptr, *d = nullptr;
    uint64_t n = 0;
    int rc = oatk_hip_ec_pairs(ctx, &k, &d, &n);
    if (rc) return rc;
    return oatk_hip_ec_graph_from_pairs(ctx, (const uint64_t *) k, (const uint32_t *) d, n);
}

// the pairs a light graph is made of (ecgraph.hpp, egr_pair_light_wave_kernel): both ends seen at least `c` times; the others leave their mark
// in g_other, one byte per oriented vertex.  Keys of 64 bits on vertex ids: what the sharded round exchanges (api_multi.inc), and the light graph of a single
// handle under OATK_DEBUG_EC_LIGHT_PACKED=0; otherwise that one takes ec_light_packed below
static int ec_light_pairs(oatk_hip_ctx *ctx, uint32_t c, const uint64_t **d_keys, const uint32_t **d_dist, uint64_t *n_keep)
{
    using namespace oatk;
    if (!ctx->counted) { ctx->err = "the light EC graph needs a resident scan + count"; return OATK_E_STATE; }
    if (!ctx->ec) ctx->ec = new EcState();
    EcState *e = ctx->ec;
    const uint64_t nv = ec_n_vtx(ctx), nr = ctx->n_reads, n = ctx->n_occ;
    int rc;
    EENSURE(g_keys, (n + 1) * 8); EENSURE(g_dist, (n + 1) * 4);
    EENSURE(g_other, 2 * nv + 8); EENSURE(g_keep, n + 8); EENSURE(g_lkeys, (n + 1) * 8); EENSURE(g_ldist, (n + 1) * 4);
    t_begin(ctx, OATK_T_EC_GRAPH);
    CK(hipMemsetAsync(e->g_other.p, 0, 2 * nv + 8, ctx->stream));
    if (n) hipLaunchKernelGGL(egr_pair_light_wave_kernel, dim3((unsigned) ((nr + 3) / 4)), dim3(256), 0, ctx->stream, nr, ctx->scm_off.as<uint64_t>(), ec_chains(ctx),
                              ctx->pos_mpos.as<uint32_t>(), e->global? e->g_gcov.as<uint32_t>() : ctx->scm_cov.as<uint32_t>(), c, e->g_keys.as<uint64_t>(), e->g_dist.as<uint32_t>(),
                              e->g_keep.as<uint8_t>(), e->g_other.as<uint8_t>());
    uint64_t nk = 0;
    if (n) {
        if (n >= 0xFFFFFFFFULL) { ctx->err = "more than 2^32 adjacent pairs"; return OATK_E_ARG; }
        EENSURE(g_keys2, (n + 1) * 8); EENSURE(g_nruns, 64);                  // (g_keys2: scratch here, the sorted keys of ec_graph_build afterwards)
        uint32_t *pos = e->g_keys2.as<uint32_t>();
        uint64_t *d_cnt = e->g_nruns.as<uint64_t>() + 2;
        auto flags = rocprim::make_transform_iterator(e->g_keep.as<uint8_t>(), [] __device__(uint8_t f) -> uint32_t { return f; });
        PRIM(rocprim::exclusive_scan, flags, pos, 0u, n, rocprim::plus<uint32_t>(), ctx->stream);
        hipLaunchKernelGGL(egr_compact_pairs_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, ctx->stream, n, e->g_keep.as<uint8_t>(), pos, e->g_keys.as<uint64_t>(),
                           e->g_dist.as<uint32_t>(), e->g_lkeys.as<uint64_t>(), e->g_ldist.as<uint32_t>(), d_cnt);
        CK(hipMemcpyAsync(&nk, d_cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
    }
    (void) rc;
    CK(hipGetLastError());
    *d_keys = e->g_lkeys.as<uint64_t>(), *d_dist = e->g_ldist.as<uint32_t>(), *n_keep = nk;
    return OATK_OK;
}

// the views the EC kernels work on (local ids, or global ids with sharded reads)
#define EC_VIEWS()                                                                                                                       \
    const uint64_t nv = e->g_n_vtx, na = e->g_n_arc, nr = ctx->n_reads, nocc = ctx->n_occ;                                               \
    EcGraph g;                                                                                                                           \
    g.n_vtx = nv, g.n_arc = na, g.idx_p = e->idx_p.as<uint64_t>(), g.idx_n = e->idx_n.as<uint32_t>();                                    \
    g.arc_v = e->arc_v.as<uint64_t>(), g.arc_w = e->arc_w.as<uint64_t>(), g.arc_ls = e->arc_ls.as<uint32_t>(), g.arc_cov = e->arc_cov.as<uint32_t>(); \
    g.arc_del = e->arc_del.as<uint8_t>(), g.scm_del = e->scm_del.as<uint8_t>();                                                          \
    g.scm_cov = e->global? e->g_gcov.as<uint32_t>() : ctx->scm_cov.as<uint32_t>(), g.scm_s = e->global? e->g_gs.as<uint64_t>() : ctx->scm_s.as<uint64_t>(); \
    g.vtx_hs_off = e->vtx_hs_off.as<uint64_t>(), g.vtx_mpos = e->vtx_mpos.as<uint32_t>();                                                \
    g.other = e->light_c? e->g_other.as<uint8_t>() : (const uint8_t *) nullptr;                                                          \
    EcReads rd;                                                                                                                          \
    rd.n_reads = nr, rd.sid0 = ctx->sid0, rd.K = ctx->K, rd.hoco_s = ctx->hoco_s.as<uint8_t>(), rd.off = ctx->d_off, rd.hoco_l = ctx->hoco_l.as<uint32_t>(); \
    rd.scm_off = ctx->scm_off.as<uint64_t>(), rd.k_mer = ec_chains(ctx), rd.m_pos = ctx->pos_mpos.as<uint32_t>();                        \
    (void) nocc; (void) rd

// the reference's own graph, flattened by the host, replaces a resident one
static int ec_upload_graph(oatk_hip_ctx *ctx, const oatk_ec_graph_t *hg)
{
    EcState *e = ctx->ec;
    const uint64_t nv = hg->n_vtx, na = hg->n_arc;
    e->graph_resident = false, e->light_c = 0;

    EENSURE(idx_p, (2 * nv + 1) * 8); EENSURE(idx_n, (2 * nv + 1) * 4); EENSURE(conv, (2 * nv + na + 2) * 8);
    EENSURE(arc_v, (na + 1) * 8); EENSURE(arc_w, (na + 1) * 8); EENSURE(arc_ls, (na + 1) * 4); EENSURE(arc_cov, (na + 1) * 4); EENSURE(arc_del, na + 8);
    CK(hipMemcpyAsync(e->idx_p.p, hg->idx_p, 2 * nv * 8, hipMemcpyHostToDevice, ctx->stream));
    CK(hipMemcpyAsync(e->conv.p, hg->idx_n, 2 * nv * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(ec_narrow_kernel, grid256(2 * nv), dim3(256), 0, ctx->stream, e->conv.as<uint64_t>(), e->idx_n.as<uint32_t>(), 2 * nv);
    if (na) {
        CK(hipMemcpyAsync(e->arc_v.p, hg->arc_v, na * 8, hipMemcpyHostToDevice, ctx->stream));
        CK(hipMemcpyAsync(e->arc_w.p, hg->arc_w, na * 8, hipMemcpyHostToDevice, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));          // conv is reused below
        CK(hipMemcpyAsync(e->conv.p, hg->arc_ls, na * 8, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(ec_narrow_kernel, grid256(na), dim3(256), 0, ctx->stream, e->conv.as<uint64_t>(), e->arc_ls.as<uint32_t>(), na);
        CK(hipMemcpyAsync(e->arc_cov.p, hg->arc_cov, na * 4, hipMemcpyHostToDevice, ctx->stream));
        CK(hipMemcpyAsync(e->arc_del.p, hg->arc_del, na, hipMemcpyHostToDevice, ctx->stream));
    }
    CK(hipStreamSynchronize(ctx->stream));              // the host arrays may go away
    e->g_n_vtx = nv, e->g_n_arc = na;
    e->graph_resident = true;
    return OATK_OK;
}

// find_error_syncmers (syncerr.c:679-757) on the resident graph; also where every vertex's k-mer can be read
extern "C" int oatk_hip_ec_mark(oatk_hip_ctx *ctx, uint32_t err_mer_c, uint32_t max_err_c, uint32_t err_arc_c, double max_arc_f)
{
    using namespace oatk;
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->counted || !ctx->ec || !ctx->ec->graph_resident) { ctx->err = "oatk_hip_ec_mark needs a resident scan + count and an EC graph"; return OATK_E_STATE; }
    CK(hipSetDevice(ctx->device));
    EcState *e = ctx->ec;
    e->done = false, e->marked = false, e->imp_used = 0;
    if (e->g_n_vtx != ec_n_vtx(ctx)) { ctx->err = "EC graph must have one vertex per syncmer"; return OATK_E_ARG; }
    if (e->light_c && !(err_mer_c >= e->light_c && err_arc_c >= err_mer_c && max_err_c >= err_mer_c)) {
        ctx->err = "the resident EC graph is a light one: it serves err_arc_c >= err_mer_c >= the coverage it was built for, and max_err_c >= err_mer_c (oatk_hip_ec_graph_light)";
        return OATK_E_ARG;
    }
    e->n_vtx = e->g_n_vtx;
    EENSURE(scm_del, e->g_n_vtx + 8); EENSURE(err_del, e->g_n_vtx + 8); EENSURE(vtx_hs_off, (e->g_n_vtx + 1) * 8); EENSURE(vtx_mpos, (e->g_n_vtx + 1) * 4);
    EC_VIEWS();
    t_begin(ctx, OATK_T_EC_MARK);
    CK(hipMemsetAsync(e->scm_del.p, 0, nv + 8, ctx->stream));
    if (na) CK(hipMemsetAsync(e->arc_del.p, 0, na, ctx->stream));           // a previous correction marked arcs (a host graph brings its own flags)
    CK(hipMemsetAsync(e->vtx_hs_off.p, 0xFF, (nv + 1) * 8, ctx->stream));   // EC_NO_SRC
    const uint64_t nl = ctx->n_scm_total;
    if (nl) hipLaunchKernelGGL(ec_vtx_src_kernel, grid256(nl), dim3(256), 0, ctx->stream, nl, ctx->scm_loc.as<uint64_t>(),
                               e->global? e->g_l2g.as<uint32_t>() : (const uint32_t *) nullptr, e->vtx_hs_off.as<uint64_t>(), e->vtx_mpos.as<uint32_t>());
    hipLaunchKernelGGL(ec_mark_kernel, grid256(nv), dim3(256), 0, ctx->stream, g, err_mer_c, max_err_c, err_arc_c, max_arc_f);
    if (na) hipLaunchKernelGGL(ec_arc_del_kernel, grid256(na), dim3(256), 0, ctx->stream, g);
    CK(hipMemcpyAsync(e->err_del.p, e->scm_del.p, nv, hipMemcpyDeviceToDevice, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    e->marked = true;
    return OATK_OK;
}

// sharded reads: k-mers of vertices as stand-alone strings, to hand to the shards that never saw them ...
extern "C" int oatk_hip_ec_export_kmers(oatk_hip_ctx *ctx, const uint32_t *d_ids, uint64_t n, uint8_t *d_out, uint32_t stride, uint8_t *d_rev)
{
    using namespace oatk;
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->ec || !ctx->ec->marked) { ctx->err = "oatk_hip_ec_export_kmers needs oatk_hip_ec_mark"; return OATK_E_STATE; }
    if (stride % 16 || stride < (uint32_t) ((ctx->K + 3) / 4 + 8)) { ctx->err = "k-mer stride must be a multiple of 16 and hold the k-mer + 8 bytes"; return OATK_E_ARG; }
    CK(hipSetDevice(ctx->device));
    EcState *e = ctx->ec;
    if (n) hipLaunchKernelGGL(ecw_export_kmer_kernel, dim3((unsigned) n), dim3(64), 0, ctx->stream, n, d_ids, e->vtx_hs_off.as<uint64_t>(), e->vtx_mpos.as<uint32_t>(),
                              ctx->hoco_s.as<uint8_t>(), ctx->K, stride, d_out, d_rev);
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    return OATK_OK;
}

// ... and the other direction: the strings go behind the hoco strings of this batch and become the vertices' sources
extern "C" int oatk_hip_ec_import_kmers(oatk_hip_ctx *ctx, const uint32_t *d_ids, const uint8_t *d_rev, const uint8_t *d_kmers, uint64_t n, uint32_t stride)
{
    using namespace oatk;
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->ec || !ctx->ec->marked) { ctx->err = "oatk_hip_ec_import_kmers needs oatk_hip_ec_mark"; return OATK_E_STATE; }
    if (stride % 16 || stride < (uint32_t) ((ctx->K + 3) / 4 + 8)) { ctx->err = "k-mer stride must be a multiple of 16 and hold the k-mer + 8 bytes"; return OATK_E_ARG; }
    CK(hipSetDevice(ctx->device));
    EcState *e = ctx->ec;
    if (n && !ctx->hoco_s.p) { ctx->err = "oatk_hip_ec_import_kmers: this batch has no hoco strings to put k-mers behind"; return OATK_E_STATE; }
    const uint64_t base = ((ctx->seq_bytes / 4 + 128) + 15) & ~15ULL;
    if (e->imp_used + n * stride > ctx->import_reserve) { ctx->err = "imported k-mers exceed the reserve behind the hoco strings (oatk_hip_ec_reserve_import before the scan)"; return OATK_E_NOMEM; }
    if (n) {
        CK(hipMemcpyAsync(ctx->hoco_s.as<uint8_t>() + base + e->imp_used, d_kmers, n * stride, hipMemcpyDeviceToDevice, ctx->stream));
        hipLaunchKernelGGL(ecw_import_kmer_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, ctx->stream, n, d_ids, d_rev, base + e->imp_used, stride,
                           e->vtx_hs_off.as<uint64_t>(), e->vtx_mpos.as<uint32_t>());
        e->imp_used += n * stride;
    }
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    return OATK_OK;
}

extern "C" int oatk_hip_ec_reserve_import(oatk_hip_ctx *ctx, uint64_t bytes)
{
    if (!ctx) return OATK_E_NODEV;
    ctx->import_reserve = bytes < (1u << 20)? (1u << 20) : (bytes + 15) & ~15ULL;
    return OATK_OK;
}

// Every switch of the error-block solver that the environment can set, read in ONE place at the start of a call.  None of them changes a result, and each is
// here because a test or a tool drives it (tests/test_gpu_ec.py runs the solver's variants against the compiled reference); defaults are what ships.
struct EcKnobs {
    int heavy = -1;               // OATK_DEBUG_EC_HEAVY=0: always round 4's tiers (ec_solve_tiers); =1: always the classes with budgets and the second stage
                                  // (ec_solve_classes); unset: by the graph (oatk_hip_ec_correct).  Tests name the solver of every variant but "device"
    bool stages = false;          // OATK_DEBUG_EC_STAGES: the stages' sizes and times on stderr
    bool serial_tiers = false;    // OATK_DEBUG_EC_SERIAL_TIERS=1: the tiers with nothing routed (tests: besides a K too large for tier 0, the only way into that flow)
    int32_t step_budget = 1000;   // OATK_DEBUG_EC_STEP_BUDGET: wavefront steps after which a first-stage class gives a block up (tests: 1 sends everything on; 3000 until r06: 242 -> 228 ms on the surrogate)
    int32_t min_nw = 0;           // OATK_DEBUG_EC_FUSED_MIN_NW: the second stage's narrowest class has that many waves (0 / 1: the single-wave class too; tests: 2, 4, 8, 16)
    int32_t heavy_cap2 = 0;       // OATK_DEBUG_EC_HEAVY_CAP2: longest block of the second class (tests: blocks the cases would not send there)
    int32_t heavy_fl = 0;         // OATK_DEBUG_EC_HEAVY_FL: bytes of the classes' LDS frame arena (tests: 64 sends every frame to HBM)
    int32_t waves = 32;           // OATK_DEBUG_EC_WAVES: first-tier waves per CU (tools/solverbench.py)
    int memo = 2;                 // OATK_DEBUG_EC_MEMO=0: every level of every block gathers its k-mer again (ec_wave.hpp: EcwMemo); =1: levels are reused, no block starts at its
                                  // sink; unset: both (A/B, tests)
    bool queue_sort = true;       // OATK_DEBUG_EC_QUEUE_SORT=0: the wave solver's queues in read order (A/B, tests)
    bool light_packed = true;     // OATK_DEBUG_EC_LIGHT_PACKED=0: the light graph's pairs sorted as 64-bit keys on vertex ids (ec_light_pairs), not on candidate ranks (A/B, tests)
    bool regroup = true;          // OATK_DEBUG_EC_REGROUP=0: the wave solver's alignment keeps its lanes on the diagonals they started a step on (ec_wave.hpp: ecw_step) (A/B, tests)
    int32_t batch = ECW_BATCH;    // OATK_DEBUG_EC_BATCH: blocks a first-tier wave takes from its queue at a time, 1 .. 64 (A/B, tests)
    bool assemble_pairs = true;   // OATK_DEBUG_EC_ASSEMBLE_PAIRS=0: the corrected chains by a wave per read (ec_assemble_seg_kernel) instead of two reads to a wave where both have at most 32
                                  // chain entries and blocks (ec_assemble_pair_kernel) (A/B, tests)
    bool light_wide = false;      // OATK_DEBUG_EC_LIGHT_KEYBITS=64: packed keys of 64 bits whatever the number of candidates (tests: the form large candidate sets take)
};
static EcKnobs ec_knobs_read()
{
    EcKnobs k;
    auto num = [](const char *n, int32_t lo, int32_t dflt) { const char *e = getenv(n); return e && atoi(e) >= lo? (int32_t) atoi(e) : dflt; };
    { const char *e = getenv("OATK_DEBUG_EC_HEAVY"); k.heavy = e && (e[0] == '0' || e[0] == '1') && !e[1]? e[0] - '0' : -1; }
    k.stages = getenv("OATK_DEBUG_EC_STAGES") != nullptr;
    { const char *e = getenv("OATK_DEBUG_EC_SERIAL_TIERS"); k.serial_tiers = e && e[0] == '1'; }
    k.step_budget = num("OATK_DEBUG_EC_STEP_BUDGET", 1, 1000);
    k.min_nw = num("OATK_DEBUG_EC_FUSED_MIN_NW", 2, 0);
    k.heavy_cap2 = num("OATK_DEBUG_EC_HEAVY_CAP2", 1, 0), k.heavy_fl = num("OATK_DEBUG_EC_HEAVY_FL", 64, 0) & ~7;
    k.waves = num("OATK_DEBUG_EC_WAVES", 1, 32);
    { const char *e = getenv("OATK_DEBUG_EC_MEMO"); k.memo = e && (e[0] == '0' || e[0] == '1') && !e[1]? e[0] - '0' : 2; }
    { const char *e = getenv("OATK_DEBUG_EC_QUEUE_SORT"); k.queue_sort = !(e && e[0] == '0' && !e[1]); }
    { const char *e = getenv("OATK_DEBUG_EC_LIGHT_PACKED"); k.light_packed = !(e && e[0] == '0' && !e[1]); }
    { const char *e = getenv("OATK_DEBUG_EC_REGROUP"); k.regroup = !(e && e[0] == '0' && !e[1]); }
    k.batch = num("OATK_DEBUG_EC_BATCH", 1, ECW_BATCH);
    if (k.batch > 64) k.batch = 64;                    // (lane i holds block i of a batch)
    { const char *e = getenv("OATK_DEBUG_EC_ASSEMBLE_PAIRS"); k.assemble_pairs = !(e && e[0] == '0' && !e[1]); }
    { const char *e = getenv("OATK_DEBUG_EC_LIGHT_KEYBITS"); k.light_wide = e && !strcmp(e, "64"); }
    return k;
}

// The light graph of a handle in local ids, on candidate ranks (ecgraph.hpp): the rank table, the kept pairs with packed keys -- by a lane per chain entry in
// two passes -- and ec_graph_build's entry for packed keys.  One wait on the host brings the number of candidates and of kept pairs.
static int ec_light_packed(oatk_hip_ctx *ctx, uint32_t c, bool force_wide)
{
    using namespace oatk;
    EcState *e = ctx->ec;
    const uint64_t nv = ec_n_vtx(ctx), nr = ctx->n_reads, n = ctx->n_occ, nw = (nv + 63) / 64, nwg = (nr + 255) / 256;
    if (n >= 0xFFFFFFFFULL) { ctx->err = "more than 2^32 adjacent pairs"; return OATK_E_ARG; }
    if (nv >= 0x7FFFFFFFULL) { ctx->err = "too many syncmers for 32-bit oriented vertex ids"; return OATK_E_ARG; }
    EENSURE(g_other, 2 * nv + 8); EENSURE(g_cbits, (nw + 1) * 8); EENSURE(g_wcnt, (nw + 1) * 4); EENSURE(g_wpre, (nw + 1) * 4);
    EENSURE(g_gcnt, (nwg + 1) * 4); EENSURE(g_gpre, (nwg + 1) * 4); EENSURE(g_nruns, 64);
    t_begin(ctx, OATK_T_EC_GRAPH);
    CK(hipMemsetAsync(e->g_other.p, 0, 2 * nv + 8, ctx->stream));
    uint32_t n_cand = 0, nk32 = 0;
    EgrPacked pk = {nullptr, 1, force_wide, nullptr};
    if (n && nv) {
        const uint64_t *bits = e->g_cbits.as<uint64_t>();
        const uint32_t *wpre = e->g_wpre.as<uint32_t>();
        const uint64_t *scm_off = ctx->scm_off.as<uint64_t>(), *chains = ec_chains(ctx);
        const uint32_t *mpos = ctx->pos_mpos.as<uint32_t>();
        hipLaunchKernelGGL(egr_cand_flag_kernel, grid256(nv), dim3(256), 0, ctx->stream, nv, nw, ctx->scm_cov.as<uint32_t>(), c, e->g_cbits.as<uint64_t>(), e->g_wcnt.as<uint32_t>());
        PRIM(rocprim::exclusive_scan, e->g_wcnt.as<const uint32_t>(), e->g_wpre.as<uint32_t>(), 0u, nw + 1, rocprim::plus<uint32_t>(), ctx->stream);
        CK(hipMemcpyAsync(&n_cand, e->g_wpre.as<uint32_t>() + nw, 4, hipMemcpyDeviceToHost, ctx->stream));
        hipLaunchKernelGGL((egr_pair_entry_kernel<uint32_t, false>), dim3((unsigned) nwg), dim3(256), 0, ctx->stream, nr, scm_off, chains, mpos, bits, wpre, 0u,
                           e->g_gcnt.as<uint32_t>(), (const uint32_t *) nullptr, (uint32_t *) nullptr, (uint32_t *) nullptr, (uint8_t *) nullptr);
        PRIM(rocprim::exclusive_scan, e->g_gcnt.as<const uint32_t>(), e->g_gpre.as<uint32_t>(), 0u, nwg + 1, rocprim::plus<uint32_t>(), ctx->stream);
        CK(hipMemcpyAsync(&nk32, e->g_gpre.as<uint32_t>() + nwg, 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        // B = the bits of the largest oriented rank, 2 n_cand - 1; n_cand <= nv < 2^31 keeps a key within 64 bits, and the test stays all the same
        while ((1ULL << pk.B) < 2 * (uint64_t) n_cand) ++pk.B;
        if (2 * pk.B > 64) { ctx->err = "light EC graph: a pair of candidate ranks does not fit a 64-bit key"; return OATK_E_ARG; }
        pk.wide = force_wide || 2 * pk.B > 32;
        EENSURE(g_lkeys, ((uint64_t) nk32 + 1) * (pk.wide? 8 : 4)); EENSURE(g_ldist, ((uint64_t) nk32 + 1) * 4); EENSURE(g_candid, ((uint64_t) n_cand + 1) * 4);
        pk.keys = e->g_lkeys.p, pk.cand_id = e->g_candid.as<uint32_t>();
        if (n_cand) hipLaunchKernelGGL(egr_cand_id_kernel, grid256(nv), dim3(256), 0, ctx->stream, nv, bits, wpre, e->g_candid.as<uint32_t>());
        if (pk.wide) hipLaunchKernelGGL((egr_pair_entry_kernel<uint64_t, true>), dim3((unsigned) nwg), dim3(256), 0, ctx->stream, nr, scm_off, chains, mpos, bits, wpre, pk.B,
                                        (uint32_t *) nullptr, (const uint32_t *) e->g_gpre.as<uint32_t>(), e->g_lkeys.as<uint64_t>(), e->g_ldist.as<uint32_t>(), e->g_other.as<uint8_t>());
        else hipLaunchKernelGGL((egr_pair_entry_kernel<uint32_t, true>), dim3((unsigned) nwg), dim3(256), 0, ctx->stream, nr, scm_off, chains, mpos, bits, wpre, pk.B,
                                (uint32_t *) nullptr, (const uint32_t *) e->g_gpre.as<uint32_t>(), e->g_lkeys.as<uint32_t>(), e->g_ldist.as<uint32_t>(), e->g_other.as<uint8_t>());
        CK(hipGetLastError());
    }
    return ec_graph_build(ctx, nullptr, e->g_ldist.as<uint32_t>(), nullptr, nk32, true, &pk);
}

// The graph read_error_correction needs and no more (include/oatk_hip_ec.h): arcs between syncmers seen at least err_mer_c times, plus one
// flag per oriented vertex for "has arcs to rarer syncmers".  oatk_hip_ec_mark / oatk_hip_ec accept it for err_arc_c >= err_mer_c >= this c.
extern "C" int oatk_hip_ec_graph_light(oatk_hip_ctx *ctx, uint32_t err_mer_c)
{
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->counted) { ctx->err = "oatk_hip_ec_graph_light needs a resident scan + count"; return OATK_E_STATE; }
    CK(hipSetDevice(ctx->device));
    if (!ctx->ec) ctx->ec = new EcState();
    if (err_mer_c == 0) return oatk_hip_ec_graph(ctx);
    const uint64_t *k = nullptr;
    const uint32_t *d = nullptr;
    uint64_t n = 0;
    const EcKnobs kn = ec_knobs_read();
    int rc;
    if (kn.light_packed && !ctx->ec->global) {           // (a handle in global ids: the sharded round's pairs, 64-bit keys on global ids)
        if ((rc = ec_light_packed(ctx, err_mer_c, kn.light_wide)) != OATK_OK) return rc;
    } else {
        if ((rc = ec_light_pairs(ctx, err_mer_c, &k, &d, &n)) != OATK_OK) return rc;
        if ((rc = ec_graph_build(ctx, k, d, nullptr, n, true)) != OATK_OK) return rc;
    }
    ctx->ec->light_c = err_mer_c;
    return OATK_OK;
}


namespace oatk {

// ---- the solver's pieces: oatk_hip_ec_correct runs one of two strategies, ec_solve_classes or ec_solve_tiers, and both are made of these ----
static const int32_t EC_CAP_T0 = 3072;         // longest block of the first tier (test hook: oatk_hip_debug_ec_tiers)
static const int32_t EC_CAP_T1 = 16384;        // longest block of round 4's last LDS tier (the same hook)
static const int32_t EC_ARC_BUDGET = 512;      // arcs (and twice as many wavefront steps) after which the classes' first tier gives a block up

// a carve-up of ec_wave.hpp: its limits, the LDS of one wave, and (hybrid) the HBM slab of one wave
struct EcTier { int32_t cap_t, cap_c, cap_w, cap_path, cap_f; uint64_t bytes, slab; bool usable, hybrid; int wpb; };

static int32_t ec_cap_c(int32_t cap_t, int K) { return cap_t + cap_t / 8 + 2 * K + 64; }       // the consensus of a block of cap_t bases

// the longest block whose band fits bwmax diagonals (bw = ceil(l * max_edist)), at most 60 000 bases
static int32_t ec_band_cap(int32_t bwmax, double max_edist)
{
    int64_t ct = max_edist > 0? (int64_t) floor((double) bwmax / max_edist) : 0x3FFFFFFF;
    while (ct > 0 && (int32_t) ceil((double) ct * max_edist) > bwmax) --ct;
    return (int32_t) (ct > 60000? 60000 : ct);
}

// workgroups of `bytes` of LDS each that one CU holds: 160 KiB of LDS, at most 16 workgroups, at least one
static uint64_t ec_wg_per_cu(uint64_t bytes)
{
    const uint64_t n = 160 * 1024 / (bytes + 256);
    return n > 16? 16 : (n? n : 1);
}

// an LDS tier of ec_wave.hpp (MODE 0: every array in LDS).  Hybrid (MODE 2): only what the alignment reads in LDS; the paths and DFS frames lie in an HBM slab
// per wave -- a path may be as long as the consensus has bases, and 1 MB holds a few thousand levels that all branch.
static EcTier ec_lds_tier(int32_t cap_t, int32_t cap_path, int32_t cap_f, bool hybrid, double max_edist, int K)
{
    EcTier t;
    const int32_t bw = (int32_t) (cap_t * max_edist) + 1;
    t.cap_t = cap_t, t.cap_w = 2 * (bw > EC_MIN_ERR_BASE? bw : EC_MIN_ERR_BASE) + 12, t.cap_c = ec_cap_c(cap_t, K);
    t.hybrid = hybrid;
    if (hybrid) {
        t.cap_path = t.cap_c, t.cap_f = 1 << 20;
        t.bytes = (uint64_t) ecw_lds_words_hybrid(t.cap_t, t.cap_c, t.cap_w) * 4;
        t.slab = ecw_slab_bytes_hybrid(t.cap_path, t.cap_f);
    } else {
        t.cap_path = cap_path, t.cap_f = cap_f;
        t.bytes = (uint64_t) ecw_scratch_words(t.cap_t, t.cap_c, t.cap_w, t.cap_path, t.cap_f, false) * 4;
        t.slab = 0;
    }
    t.usable = t.bytes <= 64 * 1024;                        // (a very large K goes straight to the slabs)
    t.wpb = ECW_WPB * t.bytes <= 64 * 1024? ECW_WPB : 1;    // waves per workgroup, each with its own carve-up
    return t;
}

// waves of an LDS tier's launch: what the CUs hold, at most per_cu_max a CU (the hardware places at most 16 workgroups on a CU, so the waves come in workgroups
// of t.wpb that share nothing)
static uint64_t ec_tier_waves(const EcTier &t, int32_t per_cu_max, int n_cu)
{
    uint64_t per_cu = ec_wg_per_cu((uint64_t) t.wpb * t.bytes) * (uint64_t) t.wpb;
    if (per_cu > (uint64_t) per_cu_max) per_cu = (uint64_t) per_cu_max / (uint64_t) t.wpb * (uint64_t) t.wpb;
    return (uint64_t) n_cu * (per_cu? per_cu : (uint64_t) t.wpb);
}

// words of one wave's optimum consensus in an LDS tier (it lives in HBM: ec_wave_kernel)
static uint64_t ec_os_words(int32_t cap_c) { return ((uint64_t) ecw_words(cap_c) + 15) & ~15ULL; }

static void ec_set_caps(EcwArgs &a, const EcTier &t) { a.cap_t = t.cap_t, a.cap_c = t.cap_c, a.cap_w = t.cap_w, a.cap_path = t.cap_path, a.cap_f = t.cap_f; }

// one launcher per kernel family: `lds` bytes of LDS per wave (ec_wave_kernel) or per workgroup (the others).  A launch that records the optimum consensus
// (a.seq_qend, oatk_hip_ec_keep_seq) runs the kernel's KEEP instantiation; every other launch runs the code it always ran.
template <int MODE, int WPB> static void ec_wave_launch(uint64_t waves, uint64_t lds, hipStream_t st, const EcwArgs &a)
{
    if (a.seq_qend) hipLaunchKernelGGL((ec_wave_kernel<MODE, WPB, true>), dim3((unsigned) ((waves + WPB - 1) / WPB)), dim3(64 * WPB), (unsigned) (WPB * lds), st, a);
    else hipLaunchKernelGGL((ec_wave_kernel<MODE, WPB>), dim3((unsigned) ((waves + WPB - 1) / WPB)), dim3(64 * WPB), (unsigned) (WPB * lds), st, a);
}
static void ec_launch_lds_tier(const EcTier &t, uint64_t waves, hipStream_t st, const EcwArgs &a)
{
    if (t.wpb > 1) {
        if (t.hybrid) ec_wave_launch<2, ECW_WPB>(waves, t.bytes, st, a);
        else ec_wave_launch<0, ECW_WPB>(waves, t.bytes, st, a);
    } else {
        if (t.hybrid) ec_wave_launch<2, 1>(waves, t.bytes, st, a);
        else ec_wave_launch<0, 1>(waves, t.bytes, st, a);
    }
}
template <int NW, int R> static void ec_heavy_launch(uint64_t wgs, uint64_t lds, hipStream_t st, const EcwArgs &a)
{
    if (a.seq_qend) hipLaunchKernelGGL((ec_heavy_kernel<NW, R, true>), dim3((unsigned) wgs), dim3(64 * NW), (unsigned) lds, st, a);
    else hipLaunchKernelGGL((ec_heavy_kernel<NW, R>), dim3((unsigned) wgs), dim3(64 * NW), (unsigned) lds, st, a);
}
template <int NW> static void ec_fused_launch(uint64_t wgs, uint64_t lds, hipStream_t st, const EcwArgs &a)
{
    if (a.seq_qend) hipLaunchKernelGGL((ec_fused_kernel<NW, true>), dim3((unsigned) wgs), dim3(64 * NW), (unsigned) lds, st, a);
    else hipLaunchKernelGGL((ec_fused_kernel<NW>), dim3((unsigned) wgs), dim3(64 * NW), (unsigned) lds, st, a);
}

// the next of the call's HBM slab buffers: launches that may run side by side each take one of their own
static int ec_slab_buf(oatk_hip_ctx *ctx, EcState *e, int &k, uint64_t bytes, hipStream_t st, const char *who, const char *what, void **p)
{
    if (k >= 16) { ctx->err = std::string("EC solver: more launches of ") + who + " than slab buffers (internal)"; return OATK_E_STATE; }
    DevBuf &b = e->hyb_slabs[k++];
    if (!b.ensure(bytes, st)) { ctx->err = std::string("hipMalloc failed for ") + who + "'s " + what; return OATK_E_NOMEM; }
    *p = b.p;
    return OATK_OK;
}

// the solver's side streams (made once per handle), and the fork event recorded on the handle's stream
static int ec_fork_side_streams(oatk_hip_ctx *ctx, EcState *e)
{
    if (!e->aux[0]) {
        // (Streams share the runtime's hardware queues -- four per priority level by default, handed out by use count -- and two launches on one queue run one AFTER
        //  the other: with the reads' uploader, the handle's own stream and a host program's streams about, the second stage's four classes were seen running
        //  8 waves, then 4 waves (rocprofv3 kernel trace, round 6).  The solver's side streams are the only ones of their priority level, so they get queues of their own.)
        int pr_least = 0, pr_greatest = 0;
        CK(hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest));
        for (int i = 0; i < 5; ++i) { CK(hipStreamCreateWithPriority(&e->aux[i], hipStreamNonBlocking, i < 4? pr_greatest : pr_least)); CK(hipEventCreateWithFlags(&e->aux_ev[i], hipEventDisableTiming)); }
        CK(hipEventCreateWithFlags(&e->fork_ev, hipEventDisableTiming));
    }
    CK(hipEventRecord(e->fork_ev, ctx->stream));
    return OATK_OK;
}

// every work item onto the list of the first tier or class whose longest block holds it; the lists' counts back to the host
static int ec_route(oatk_hip_ctx *ctx, EcState *e, uint64_t n_work, const EcRoute &rt, unsigned long long *routed, size_t bytes)
{
    hipLaunchKernelGGL(ec_route_kernel, dim3((unsigned) ((n_work + 256 * ECW_ROUTE_ITEMS - 1) / (256 * ECW_ROUTE_ITEMS))), dim3(256), 0, ctx->stream, e->work.as<EcWork>(), n_work, rt);
    CK(hipMemcpyAsync(routed, rt.cnt[0], bytes, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return OATK_OK;
}

// a list of blocks, longest first: a block's length is what the host can tell of its search, and the longest search of a batch (0.6 s on the config-1 surrogate)
// must not start when the others are done.  A radix sort on ~length, its keys and values in todo2 (the caller has made room for 3 (n + 1) words).
static int ec_sort_longest_first(oatk_hip_ctx *ctx, EcState *e, uint32_t *list, uint64_t n)
{
    uint32_t *k_in = e->todo2.as<uint32_t>(), *k_out = k_in + (n + 1), *v_out = k_out + (n + 1);
    hipLaunchKernelGGL(ec_route_keys_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, ctx->stream, e->work.as<EcWork>(), list, n, k_in);
    PRIM(rocprim::radix_sort_pairs, k_in, k_out, list, v_out, n, 0, 32, ctx->stream);
    CK(hipMemcpyAsync(list, v_out, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    return OATK_OK;
}

// A queue of the wave solver in source order: blocks of one source, and among them of one sink, next to each other, so that a wave's batch is mostly one walk
// (ec_wave.hpp: EcwMemo).  The key is the source's first live arc -- one per source that has an arc -- then the sink.  Only neighbours matter, not the order, so
// the key is as narrow as the batch allows: the bits its live arcs need, and of the sink the low bits that fill the key up to the next whole 8-bit pass of the
// sort beyond eight (at config 3: 14 + 10 bits, three passes over 32-bit keys; the vertex ids themselves need 24 bits and would make it 64-bit keys and five
// passes, 0.75 ms -- profiles/r17a).  Two sinks of one source that agree in those bits are interleaved in read order, which costs their blocks the start at the
// sink and nothing else; the sort keeps read order among equal keys.  list == nullptr: every work item.  The sorted list is *sorted, in qidx behind the call's
// earlier ones (the caller has made room: ec_queue_room); `st` and `tmp`: the stream the launch is on and a temporary nobody else on another stream uses.
static int ec_queue_room(oatk_hip_ctx *ctx, EcState *e, uint64_t n_work)
{
    e->q_used = e->qk_used = 0;
    EENSURE(qkey, (4 * (n_work + 1) + 64) * 4); EENSURE(qidx, 2 * (n_work + 1) * 4);
    return OATK_OK;
}
static int ec_queue_sort(oatk_hip_ctx *ctx, EcState *e, const uint32_t *list, uint64_t n, hipStream_t st, DevBuf &tmp, const uint32_t **sorted)
{
    auto bits = [](uint64_t v) { int b = 1; while (b < 64 && (v >> b)) ++b; return b; };
    const uint64_t end_max = 2 * e->g_n_vtx;                 // (an open block's EC_NONE: one value for all of them)
    const uint32_t lp_max = (uint32_t) e->n_live;
    const int lb = bits(lp_max), total = lb + 8 >= 32? 32 : (lb + 8 + 7) & ~7;
    const int eb = bits(end_max) < total - lb? bits(end_max) : total - lb;
    if (e->q_used + n > e->qidx.cap / 4 || e->qk_used + 2 * (n + 1) > e->qkey.cap / 4) { ctx->err = "EC solver: more sorted queues than room for them (internal)"; return OATK_E_STATE; }
    uint32_t *v_out = e->qidx.as<uint32_t>() + e->q_used, *k_in = e->qkey.as<uint32_t>() + e->qk_used, *k_out = k_in + (n + 1);
    e->q_used += n, e->qk_used += 2 * (n + 1);
    hipLaunchKernelGGL(ec_queue_keys_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, st, e->work.as<EcWork>(), list, n, lp_max, end_max, eb, k_in);
    if (list) PRIM_IN(tmp, st, "hipMalloc failed (EC queue sort)", rocprim::radix_sort_pairs, k_in, k_out, list, v_out, n, 0, (unsigned) (eb + lb), st);
    else {
        rocprim::counting_iterator<uint32_t> iota(0);
        PRIM_IN(tmp, st, "hipMalloc failed (EC queue sort)", rocprim::radix_sort_pairs, k_in, k_out, iota, v_out, n, 0, (unsigned) (eb + lb), st);
    }
    *sorted = v_out;
    return OATK_OK;
}
// blocks a wave of a larger tier takes from its queue at a time: consecutive blocks of a sorted list share a wave only in a batch, and a few hundred long blocks
// must still have a wave each (r04e)
static int32_t ec_routed_batch(uint64_t n_todo, uint64_t waves, int32_t cap)
{
    const uint64_t b = waves? n_todo / (16 * waves) : 1;
    return (int32_t) (b < 1? 1 : (b > (uint64_t) cap? (uint64_t) cap : b));
}
// OATK_DEBUG_EC_STAGES: what the launches of ec_wave_kernel reused and how many turns their alignments took (EcwArgs::memo_stat: three counters per launch behind the cursor's 64)
struct EcMemoLog { int tier; unsigned long long n; int32_t batch; int slot; };
static int ec_memo_report(oatk_hip_ctx *ctx, EcState *e, const std::vector<EcMemoLog> &log)
{
    if (log.empty()) return OATK_OK;
    unsigned long long c[192];
    CK(hipMemcpyAsync(c, (unsigned long long *) e->cursor.p + 64, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    for (const EcMemoLog &l : log)
        fprintf(stderr, "[ec stages] wave solver, tier %d, %llu blocks: batch %d, %llu levels reused, %llu blocks started at their sink, %llu extension turns\n", l.tier, l.n, (int) l.batch, c[3 * l.slot], c[3 * l.slot + 1], c[3 * l.slot + 2]);
    return OATK_OK;
}

// The slab tier: deeper than the carve-ups' frames, or longer than their blocks.  One wave per block, every array in an HBM slab sized for the longest read of
// the batch (ec_wave_kernel MODE 1); what outgrows even that is only counted (cursor[63]) and the call fails.  todo == nullptr: every work item.
static int ec_launch_slab_tier(oatk_hip_ctx *ctx, EcState *e, const EcwArgs &base, uint32_t &max_hl, const uint32_t *todo, uint64_t n_todo,
                               unsigned long long *queue, hipStream_t st)
{
    if (max_hl == 0) {
        std::vector<uint32_t> hl(ctx->n_reads);
        CK(hipMemcpy(hl.data(), ctx->hoco_l.p, ctx->n_reads * 4, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < ctx->n_reads; ++i) if (hl[i] > max_hl) max_hl = hl[i];
    }
    EcwArgs a = base;
    a.cap_t = (int32_t) max_hl + 64, a.cap_c = ec_cap_c(a.cap_t, ctx->K);
    a.cap_w = 2 * ((int32_t) (max_hl * base.max_edist) + 16) + 16, a.cap_path = ec_cap_c((int32_t) max_hl, ctx->K), a.cap_f = 1 << 22;
    a.todo = todo, a.n_todo = n_todo, a.next = queue, a.skip_l = 0x7FFFFFFF, a.batch = 1;
    a.todo_out = e->todo2.as<uint32_t>(), a.todo_cnt = base.pool_cursor + 63;
    a.slab_bytes = ((uint64_t) ecw_scratch_words(a.cap_t, a.cap_c, a.cap_w, a.cap_path, a.cap_f) * 4 + 63) & ~63ULL;
    uint64_t waves = todo? n_todo : base.n_work;
    if (waves > 1024) waves = 1024;
    if (!waves) return OATK_OK;
    EENSURE(big_slabs, waves * a.slab_bytes);
    a.slabs = e->big_slabs.as<uint8_t>();
    ec_wave_launch<1, 1>(waves, 0, st, a);
    return OATK_OK;
}

// The second stage: the blocks that went past the first stage's step budget or outgrew a class (`todo`, nh of them), several steps per barrier, longest first.
// A wave owns 56 slots of the wavefront (ec_fused.hpp), a block needs 2 bw + 3: classes of 16, 8, 4 and 2 waves -- the fewer waves meet, the cheaper the meeting, the
// fewer copies of the search's scalar bookkeeping run (every wave of a block executes all of it: 276 scalar + 150 vector instructions per arc and wave on the
// config-1 surrogate, profiles/r06b_config1s_pmc_ec.csv -- the second stage is bound by instruction issue while every CU is full) and the more blocks a CU holds.
// The narrowest bands (2 bw + 3 <= 64: blocks of up to 1500 bases) take ONE wave each, the wavefront a diagonal per lane in registers, no barrier anywhere
// (ec_heavy.hpp with NW = 1, the first stage's engine without its budget): such a block's search is arcs, not steps -- 0.9 steps per arc on four diagonals on the
// config-1 surrogate, a long arc that dies costs its thirty steps at most -- and two waves that meet at four barriers per arc took 3 us per arc where the first
// tier's single wave took 1.75.  (Wider bands on one wave, two diagonals per lane, were tried: 78 s of wave time against 104, but their long dying arcs are not
// asked by table there and the longest block took 451 ms against 209.)  In a list sorted longest first the classes are consecutive stretches.  All launches run
// side by side; what outgrows one (frames, paths) goes onto `todo_out` (cursor[1], `left` of them) for the slab tier.
static int ec_second_stage(oatk_hip_ctx *ctx, EcState *e, const EcKnobs &kn, const EcwArgs &base, uint32_t *todo, uint64_t nh, uint32_t *todo_out,
                           int &qslot, int &hyb_k, unsigned long long &left)
{
    unsigned long long *cur = base.pool_cursor;
    struct timespec ts0, ts1;
    if (kn.stages) clock_gettime(CLOCK_MONOTONIC, &ts0);
    if (nh > 1 && nh <= (4u << 20)) {
        if (3 * (nh + 1) > base.n_work + 1) EENSURE(todo2, 3 * (nh + 1) * 4);
        int rc = ec_sort_longest_first(ctx, e, todo, nh); if (rc) return rc;
    }
    const int NCLS = 5;
    const int NWS[NCLS] = {16, 8, 4, 2, 1};
    EcwArgs fa[NCLS];
    uint64_t lds[NCLS];
    for (int i = 0; i < NCLS; ++i) {
        const int NW = NWS[i];
        EcwArgs &a = fa[i];
        a = base;
        a.cap_t = ec_band_cap(((NW == 1? 64 : NW * ECF_OWN) - 3) / 2, base.max_edist);
        a.cap_c = ec_cap_c(a.cap_t, ctx->K), a.cap_w = 0, a.cap_path = a.cap_c;
        a.cap_f = kn.heavy_fl? kn.heavy_fl : (NW == 16? 32768 : (NW == 8? 24576 : (NW == 4? 16384 : (NW == 2? 12288 : 8192))));
        a.os_words = 1 << 20;
        lds[i] = (uint64_t) (NW == 1? ech_lds_words(a.cap_t, a.cap_c, a.cap_f, 1) : ecf_lds_words(a.cap_t, a.cap_c, a.cap_f, NW)) * 4;
    }
    int narrowest = NCLS - 1;                                          // OATK_DEBUG_EC_FUSED_MIN_NW=2: no single-wave class (A/B, tests); =8: the two classes of round 5
    if (kn.min_nw >= 2) narrowest = kn.min_nw >= 16? 0 : (kn.min_nw >= 8? 1 : (kn.min_nw >= 4? 2 : 3));
    while (narrowest > 0 && lds[narrowest] > 64 * 1024) --narrowest;
    // longer[i] = blocks too long for class i + 1 (the head of the sorted list): class i takes todo[longer[i - 1] .. longer[i])
    unsigned long long longer[NCLS] = {0, 0, 0, 0, 0};
    CK(hipMemsetAsync(cur + 1, 0, 40, ctx->stream));                  // [1] what is left over, [2 .. 5] the counts
    for (int i = 0; i < narrowest; ++i)
        hipLaunchKernelGGL(ec_route_longer_kernel, dim3((unsigned) ((nh + 255) / 256)), dim3(256), 0, ctx->stream, e->work.as<EcWork>(), todo, nh, lds[i + 1] <= 64 * 1024? fa[i + 1].cap_t : -1, cur + 2 + i);
    CK(hipMemcpyAsync(longer, cur + 2, 32, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    if (nh > (4u << 20)) longer[0] = nh;                               // (unsorted: sixteen waves for all)
    longer[narrowest] = nh;
    for (int i = 1; i <= narrowest; ++i) if (longer[i] < longer[i - 1]) longer[i] = longer[i - 1];
    // A class whose carve-up does not fit LDS runs nothing (the sixteen waves below max_edist ~ 0.0075: ec_band_cap's 60 000 bases, DESIGN.md 8.3): its blocks are
    // too long for the classes behind it and go straight on to the slab tier, ahead of what the launches leave over
    unsigned long long passed = 0;
    for (int i = 0; i <= narrowest; ++i) {
        const uint64_t b0 = i? longer[i - 1] : 0, b1 = longer[i];
        if (b1 <= b0 || lds[i] <= 64 * 1024) continue;
        CK(hipMemcpyAsync(todo_out + passed, todo + b0, (b1 - b0) * 4, hipMemcpyDeviceToDevice, ctx->stream));
        passed += b1 - b0;
    }
    if (passed) CK(hipMemcpyAsync(cur + 1, &passed, 8, hipMemcpyHostToDevice, ctx->stream));     // (the stream is synchronised before `passed` goes)
    if (passed && kn.stages) fprintf(stderr, "[ec stages] %llu blocks past a class that does not fit LDS\n", passed);
    auto launch = [&](int i, const uint32_t *list, uint64_t n, hipStream_t st) -> int {
        const int NW = NWS[i];
        if (qslot >= 60) { ctx->err = "EC solver: more launches than work-queue counters (internal)"; return OATK_E_STATE; }
        EcwArgs a = fa[i];
        a.todo = list, a.n_todo = n, a.next = cur + qslot++, a.skip_l = 0x7FFFFFFF, a.batch = 1, a.arc_budget = 0;
        a.todo_out = todo_out, a.todo_cnt = cur + 1;
        a.slab_bytes = ech_slab_bytes(a.cap_c, a.cap_path, (int32_t) a.os_words);
        uint64_t per_cu = ec_wg_per_cu(lds[i]);                        // one wave per block (ec_heavy.hpp)
        if (NW > 1) {                                                  // a workgroup per block: 2048 threads a CU
            const uint64_t by_lds = 160 * 1024 / (lds[i] + 512);
            per_cu = 2048 / (64 * (uint64_t) NW);
            if (per_cu > by_lds) per_cu = by_lds;
            if (per_cu > 16) per_cu = 16;
            if (!per_cu) per_cu = 1;
        }
        uint64_t wgs = (uint64_t) ctx->n_cu * per_cu;
        if (wgs > n) wgs = n;
        void *p = nullptr;
        { int rc = ec_slab_buf(ctx, e, hyb_k, wgs * a.slab_bytes + 64, st, "the workgroup solver", "slabs", &p); if (rc) return rc; }
        a.slabs = (uint8_t *) p;
        if (NW == 1) {
            ec_heavy_launch<1, 1>(wgs, lds[i], st, a);
            if (kn.stages) fprintf(stderr, "[ec stages] one wave: %llu blocks on %llu waves (%llu B of LDS, slabs %.1f MB)\n", (unsigned long long) n, (unsigned long long) wgs, (unsigned long long) lds[i], wgs * a.slab_bytes / 1e6);
            return OATK_OK;
        }
        { int rc = ec_slab_buf(ctx, e, hyb_k, wgs * ecf_tab_words(a.cap_t) * 4 + 64, st, "the workgroup solver", "tables", &p); if (rc) return rc; }
        a.os_slabs = (uint32_t *) p;                                   // a region of tables per workgroup
        if (NW == 2) ec_fused_launch<2>(wgs, lds[i], st, a);
        else if (NW == 4) ec_fused_launch<4>(wgs, lds[i], st, a);
        else if (NW == 8) ec_fused_launch<8>(wgs, lds[i], st, a);
        else ec_fused_launch<16>(wgs, lds[i], st, a);
        if (kn.stages) fprintf(stderr, "[ec stages] %d waves: %llu blocks on %llu workgroups (%llu B of LDS, slabs %.1f MB)\n", NW, (unsigned long long) n, (unsigned long long) wgs, (unsigned long long) lds[i], wgs * a.slab_bytes / 1e6);
        return OATK_OK;
    };
    CK(hipEventRecord(e->fork_ev, ctx->stream));
    int used_aux = 0;
    bool used_low = false;
    for (int i = 0; i <= narrowest; ++i) {                             // the longest blocks first, each class on a side stream of its own ([4]: the single waves)
        const uint64_t b0 = i? longer[i - 1] : 0, b1 = longer[i];
        if (b1 <= b0 || lds[i] > 64 * 1024) continue;
        const int s = NWS[i] == 1? 4 : used_aux;
        CK(hipStreamWaitEvent(e->aux[s], e->fork_ev, 0));
        { int rc = launch(i, todo + b0, b1 - b0, e->aux[s]); if (rc) return rc; }
        CK(hipEventRecord(e->aux_ev[s], e->aux[s]));
        if (s == 4) used_low = true; else ++used_aux;
    }
    if (used_low) CK(hipStreamWaitEvent(ctx->stream, e->aux_ev[4], 0));
    for (int i = 0; i < used_aux; ++i) CK(hipStreamWaitEvent(ctx->stream, e->aux_ev[i], 0));
    CK(hipMemcpyAsync(&left, cur + 1, 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    if (kn.stages) { clock_gettime(CLOCK_MONOTONIC, &ts1); fprintf(stderr, "[ec stages] second stage %.1f ms; %llu left for the slabs\n", ((double) (ts1.tv_sec - ts0.tv_sec) + 1e-9 * (double) (ts1.tv_nsec - ts0.tv_nsec)) * 1e3, left); }
    return OATK_OK;
}

// Round 5's classes with step budgets, then the second stage (the live graph branches: the config-1 surrogate).  Classes by block length: the first tier of
// ec_wave.hpp (a wave per block, everything in LDS) for the millions of small blocks; three carve-ups of ec_heavy.hpp -- classes 1 and 2 ONE wave per block with
// the wavefront in 4 / 8 registers per lane (2 bw + 3 <= 64 R: no barrier at all, fifteen blocks a CU), class 3 ECH_NW waves and 6 (2 bw + 3 <= 256 R).  The
// classes run with a BUDGET of wavefront steps: nearly every block is done within a few dozen (config 3: 258 k blocks past the first tier).  A block that goes
// past it is a search inside a repeat -- a million steps on hundreds of diagonals -- and starts again in the second stage; what outgrows that, in the slab tier.
// (A solver that shares a block's search TREE among eight waves was built in round 5, is exact and 2 - 8 x slower on repeats: tools/experiments/ec_tree.hpp.)
// n_big: the blocks the first tier did not finish.
static int ec_solve_classes(oatk_hip_ctx *ctx, EcState *e, const EcKnobs &kn, const EcwArgs &base, uint32_t &max_hl, uint64_t &n_big)
{
    const uint64_t n_work = base.n_work;
    unsigned long long *cur = base.pool_cursor;    // [0] pool, [1 .. 4] entries of list[c], [5 ...] one work queue per launch, [63] blocks that outgrew the slabs
    struct EcClass { int32_t cap_t, cap_c, cap_fl, cap_fh; int R; uint64_t lds, slab; bool usable, routes; } H[4];
    const int hr[4] = {0, 4, 8, 6};
    for (int c = 1; c <= 3; ++c) {
        EcClass &h = H[c];
        h.R = hr[c];
        int32_t ct = ec_band_cap(((c < 3? 64 : 256) * h.R - 3) / 2, base.max_edist);
        if (c == 1 && ctx->ec_cap_t1 > 0 && ctx->ec_cap_t1 < ct) ct = ctx->ec_cap_t1;      // (test hooks: push blocks into the larger classes)
        if (c == 2 && kn.heavy_cap2 > H[1].cap_t && kn.heavy_cap2 < ct) ct = kn.heavy_cap2;
        h.cap_t = ct, h.cap_c = ec_cap_c(ct, ctx->K);              // (the paths have cap_c entries: every arc appends at least one base)
        h.cap_fl = kn.heavy_fl? kn.heavy_fl : (c < 3? 4096 : 32768);
        h.cap_fh = c < 3? 128 << 10 : 1 << 20;                     // (thousands of single waves: a megabyte of HBM frames each would be gigabytes; what outgrows 128 KB is a heavy search and goes on anyway)
        h.lds = (uint64_t) ech_lds_words(h.cap_t, h.cap_c, h.cap_fl, h.R) * 4;
        h.slab = ech_slab_bytes(h.cap_c, h.cap_c, h.cap_fh);
        h.usable = h.lds <= 64 * 1024;
        h.routes = h.usable && (c == 1 || h.cap_t > H[c - 1].cap_t);      // (a class that takes no longer blocks than the one before it only takes that one's left-overs)
    }
    EcTier T0 = ec_lds_tier(ctx->ec_cap_t0 > 0? ctx->ec_cap_t0 : EC_CAP_T0, 32, 2048, false, base.max_edist, ctx->K);
    T0.usable = T0.usable && H[1].usable && T0.cap_t <= H[1].cap_t;
    const uint64_t t0_waves = T0.usable? ec_tier_waves(T0, kn.waves, ctx->n_cu) : 0;
    EENSURE(os_slabs, (t0_waves + ECW_WPB) * ec_os_words(T0.cap_c) * 4 + 64);
    // lists 1 .. 3: the classes' blocks (routed there by length, or left over by the first tier); list 4: what the classes gave up on
    EENSURE(todo, 4 * (n_work + 1) * 4); EENSURE(todo2, (n_work + 1) * 4);
    uint32_t *list[5] = {nullptr, e->todo.as<uint32_t>(), e->todo.as<uint32_t>() + (n_work + 1), e->todo.as<uint32_t>() + 2 * (n_work + 1), e->todo.as<uint32_t>() + 3 * (n_work + 1)};
    int qslot = 5, hyb_k = 0;
    auto launch_class = [&](int c, const uint32_t *todo, uint64_t n_todo, hipStream_t st) -> int {
        if (!n_todo) return OATK_OK;
        if (qslot >= 60) { ctx->err = "EC solver: more launches than work-queue counters (internal)"; return OATK_E_STATE; }
        const EcClass &h = H[c];
        EcwArgs a = base;
        a.cap_t = h.cap_t, a.cap_c = h.cap_c, a.cap_w = kn.step_budget, a.cap_path = h.cap_c, a.cap_f = h.cap_fl, a.os_words = (uint64_t) h.cap_fh;
        a.todo = todo, a.n_todo = n_todo, a.next = cur + qslot++, a.skip_l = 0x7FFFFFFF, a.batch = 1;
        a.todo_out = list[4], a.todo_cnt = cur + 4;
        uint64_t wgs = (uint64_t) ctx->n_cu * (c < 3? ec_wg_per_cu(h.lds) : 8);
        if (wgs > n_todo) wgs = n_todo;
        while (wgs > (uint64_t) ctx->n_cu && wgs * h.slab > (3ULL << 30)) wgs -= (uint64_t) ctx->n_cu;          // (no launch holds more than three gigabytes of slabs: several handles share a device)
        void *p = nullptr;
        { int rc = ec_slab_buf(ctx, e, hyb_k, wgs * h.slab + 64, st, "the workgroup solver", "slabs", &p); if (rc) return rc; }
        a.slabs = (uint8_t *) p, a.slab_bytes = h.slab;
        if (c == 1) ec_heavy_launch<1, 4>(wgs, h.lds, st, a);
        else if (c == 2) ec_heavy_launch<1, 8>(wgs, h.lds, st, a);
        else ec_heavy_launch<ECH_NW, 6>(wgs, h.lds, st, a);
        return OATK_OK;
    };
    // 1. route by length, the classes of long blocks on streams of their own (longest first: they are the longest chains of dependent steps), the first tier beside them
    //    A class whose carve-up does not fit LDS runs nothing (class 3 below max_edist ~ 0.0128: ec_band_cap's 60 000 bases, DESIGN.md 8.3): the blocks routed to it
    //    go onto the second stage's list (routed[4] of them), which hands on to the slab tier what its own classes cannot hold
    EcRoute rt;
    for (int c = 0; c < 4; ++c) rt.list[c] = list[c], rt.cnt[c] = cur + c;
    for (int c = 1; c < 4; ++c) if (!H[c].usable) rt.list[c] = list[4], rt.cnt[c] = cur + 4;
    // (no first tier -- above max_edist ~ 0.049 class 1 holds fewer than its 3072 bases -- sends every block on: a cap of -1, as a trailing block can have 0 bases)
    rt.cap[0] = T0.usable? T0.cap_t : -1, rt.cap[1] = H[1].routes? H[1].cap_t : 0, rt.cap[2] = H[2].routes? H[2].cap_t : 0, rt.cap[3] = 0x7FFFFFFF;
    unsigned long long routed[5] = {0, 0, 0, 0, 0}, cnts[5] = {0, 0, 0, 0, 0};
    if (n_work) { int rc = ec_route(ctx, e, n_work, rt, routed, sizeof(routed)); if (rc) return rc; }
    { int rc = ec_fork_side_streams(ctx, e); if (rc) return rc; }
    {   // (room to sort a class's list)
        unsigned long long mx = routed[1] > routed[2]? routed[1] : routed[2];
        mx = routed[3] > mx? routed[3] : mx;
        if (mx <= (4u << 20) && 3 * (mx + 1) > n_work + 1) EENSURE(todo2, 3 * (mx + 1) * 4);
    }
    int used_aux = 0;
    for (int c = 3; c >= 1; --c) {
        if (!routed[c]) continue;
        if (routed[c] > 1 && routed[c] <= (64u << 10)) {               // (the lists are small: thousands of blocks)
            int rc = ec_sort_longest_first(ctx, e, list[c], routed[c]); if (rc) return rc;
            CK(hipEventRecord(e->fork_ev, ctx->stream));
        }
        hipStream_t st = e->aux[used_aux];
        CK(hipStreamWaitEvent(st, e->fork_ev, 0));
        { int rc = launch_class(c, list[c], routed[c], st); if (rc) return rc; }
        CK(hipEventRecord(e->aux_ev[used_aux], st));
        ++used_aux;
    }
    std::vector<EcMemoLog> mlog;
    if (T0.usable && n_work) {
        EcwArgs a = base;
        ec_set_caps(a, T0);
        a.todo = nullptr, a.n_todo = 0, a.next = cur + qslot++, a.skip_l = T0.cap_t, a.batch = kn.batch;
        if (kn.queue_sort && n_work > 1) {          // (where the graph branches a walk ends at the first frame, and the kernel reuses nothing behind it)
            { int rc = ec_queue_room(ctx, e, n_work); if (rc) return rc; }
            { int rc = ec_queue_sort(ctx, e, nullptr, n_work, ctx->stream, ctx->tmp, &a.todo); if (rc) return rc; }
            a.n_todo = n_work;
        }
        if (kn.stages) a.memo_stat = cur + 64 + 3 * mlog.size(), mlog.push_back(EcMemoLog{0, (unsigned long long) n_work, a.batch, (int) mlog.size()});
        // (a small block inside a repeat tries tens of thousands of arcs on a handful of diagonals -- 70 ms of ONE wave on the config-1 surrogate with everything else waiting
        //  for this launch: past the arc budget it is left to the classes and, past their step budget, to the second stage)
        a.arc_budget = EC_ARC_BUDGET;
        a.todo_out = list[1], a.todo_cnt = cur + 1;        // what outgrows the first tier's frames or paths is short: the first class takes it
        a.os_words = ec_os_words(T0.cap_c), a.os_slabs = e->os_slabs.as<uint32_t>();
        uint64_t waves = t0_waves;
        const uint64_t groups = (n_work + (uint64_t) a.batch - 1) / (uint64_t) a.batch;
        if (waves > groups) waves = groups;
        ec_launch_lds_tier(T0, waves, ctx->stream, a);
    }
    // 2. the first tier's left-overs (deep searches: the longest chains of the batch) as soon as it is done; then everything launched so far; then the second stage
    CK(hipMemcpyAsync(cnts, cur, sizeof(cnts), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    if (kn.stages) { int rc = ec_memo_report(ctx, e, mlog); if (rc) return rc; }
    if (cnts[1] > routed[1]) { int rc = launch_class(1, list[1] + routed[1], cnts[1] - routed[1], ctx->stream); if (rc) return rc; }
    n_big = cnts[1] + routed[2] + routed[3] + routed[4];
    for (int i = 0; i < used_aux; ++i) CK(hipStreamWaitEvent(ctx->stream, e->aux_ev[i], 0));
    CK(hipMemcpyAsync(cnts, cur, sizeof(cnts), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    if (kn.stages) fprintf(stderr, "[ec stages] first stage done: %llu blocks go on (classes got %llu + %llu + %llu; %llu past a class that does not fit LDS)\n", cnts[4], cnts[1], routed[2], routed[3], routed[4]);
    if (!cnts[4]) return OATK_OK;
    unsigned long long left = 0;
    { int rc = ec_second_stage(ctx, e, kn, base, list[4], cnts[4], list[1], qslot, hyb_k, left); if (rc) return rc; }
    if (!left) return OATK_OK;
    return ec_launch_slab_tier(ctx, e, base, max_hl, list[1], left, cur + qslot++, ctx->stream);
}

// Round 4's tiers (the live graph does not branch: config 2 and config 3).  One wave per block in every tier: small LDS carve-ups for every block, larger ones
// (fewer waves per CU) for the blocks that did not fit, the last of them hybrid, HBM slabs for the rest.  n_big: the blocks the first tier did not finish.
static int ec_solve_tiers(oatk_hip_ctx *ctx, EcState *e, const EcKnobs &kn, const EcwArgs &base, uint32_t &max_hl, uint64_t &n_big)
{
    const int LAST = 3;                  // tiers 0 .. LAST - 1 carve LDS (more per wave, fewer waves per CU), tier LAST uses HBM slabs
    const uint64_t n_work = base.n_work;
    unsigned long long *cur = base.pool_cursor;    // [0] pool, [1 .. 3] entries of list[t], [4 ...] one work queue per launch, [63] blocks that outgrew the slabs
    const int32_t t_lo = ctx->ec_cap_t0 > 0? ctx->ec_cap_t0 : EC_CAP_T0, t_hi = ctx->ec_cap_t1 > 0? ctx->ec_cap_t1 : EC_CAP_T1;
    EcTier T[LAST + 1];
    T[0] = ec_lds_tier(t_lo, 32, 2048, false, base.max_edist, ctx->K);
    T[1] = ec_lds_tier(2 * t_lo < t_hi? 2 * t_lo : t_hi, 64, 4096, false, base.max_edist, ctx->K);
    T[2] = ec_lds_tier(t_hi, 0, 0, true, base.max_edist, ctx->K);
    T[LAST] = EcTier{}, T[LAST].usable = true;                 // the slab tier, sized when (if) a block gets there: it takes the longest read of the batch
    // the LDS tiers' optimum consensus: one slab per wave and launch (a tier is launched at most twice, and tiers run side by side), sized before anything runs
    uint64_t os_total = 0, os_next = 0;
    for (int t = 0; t < LAST; ++t) if (T[t].usable) os_total += 3 * (ec_tier_waves(T[t], kn.waves, ctx->n_cu) + ECW_WPB) * ec_os_words(T[t].cap_c);
    EENSURE(os_slabs, os_total * 4 + 64);
    // lists: list[t] collects the blocks tier t must run -- routed there by length before anything runs, or left over by a smaller tier
    EENSURE(todo, 3 * (n_work + 1) * 4); EENSURE(todo2, (n_work + 1) * 4);
    uint32_t *list[4] = {nullptr, e->todo.as<uint32_t>(), e->todo.as<uint32_t>() + (n_work + 1), e->todo.as<uint32_t>() + 2 * (n_work + 1)};
    int qslot = 4, hyb_k = 0;
    std::vector<EcMemoLog> mlog;
    if (kn.queue_sort) { int rc = ec_queue_room(ctx, e, n_work); if (rc) return rc; }
    auto next_usable = [&](int t) { int u = t + 1; while (u < LAST && !T[u].usable) ++u; return u; };
    auto launch = [&](int tier, const uint32_t *todo, uint64_t n_todo, hipStream_t st, bool routed, uint64_t max_waves = 0) -> int {
        if (qslot >= 60) { ctx->err = "EC solver: more rounds of left-overs than queue counters (internal)"; return OATK_E_STATE; }
        unsigned long long *queue = cur + qslot++;
        if (kn.stages) fprintf(stderr, "[ec stages] tier %d: %llu blocks%s\n", tier, (unsigned long long) (todo? n_todo : n_work), todo? (routed? " routed by length" : " left over") : "");
        if (tier == LAST) return ec_launch_slab_tier(ctx, e, base, max_hl, todo, n_todo, queue, st);
        const EcTier &t = T[tier];
        EcwArgs a = base;
        ec_set_caps(a, t);
        a.todo = todo, a.n_todo = n_todo, a.next = queue;
        a.skip_l = routed && tier == 0? t.cap_t : 0x7FFFFFFF;
        a.batch = kn.batch;                                        // (a larger tier: by its blocks and waves, below)
        // a block outgrows an LDS tier by the depth of its search or by its frames (its length was checked before): the hybrid tier, without such limits, takes it
        const int nx = tier < LAST - 1 && T[LAST - 1].usable? LAST - 1 : next_usable(tier);
        a.todo_out = list[nx], a.todo_cnt = cur + nx;
        uint64_t waves = ec_tier_waves(t, kn.waves, ctx->n_cu);
        a.os_words = ec_os_words(t.cap_c);
        if ((os_next + waves * a.os_words) * 4 > e->os_slabs.cap) { ctx->err = "EC solver: more launches than optimum-consensus slabs (internal)"; return OATK_E_STATE; }
        a.os_slabs = e->os_slabs.as<uint32_t>() + os_next;
        os_next += waves * a.os_words;
        const uint64_t n_items = todo? n_todo : n_work;
        if (tier > 0) {                                            // (241 long blocks in batches of sixteen were sixteen waves' work: r04e)
            uint64_t w1 = waves < n_items? waves : n_items;
            if (max_waves && w1 > max_waves) w1 = max_waves;
            a.batch = ec_routed_batch(n_items, w1, kn.batch);
        }
        // the queue in source order: every block for the first tier, a routed list for a larger one where its waves take batches (a wave forgets between batches:
        // a list taken block by block gains nothing).  Sorted on the launch's own stream: the first tier does not wait for a side stream's list, and its own sort,
        // of every block, ends after a side stream's, of some: the larger tiers must be on the CUs before the first tier fills them (below).  Sorted in front of
        // the routing instead, the first tier got there first and the second ran behind it: 21.3 ms against 12.7 (profiles/r17a_ab_bench.txt)
        if (kn.queue_sort && (todo? routed : true) && n_items > 1 && a.batch > 1) {
            DevBuf *tmp = &ctx->tmp;
            for (int i = 0; i < 4; ++i) if (st == e->aux[i]) tmp = &e->qtmp[i];
            { int rc = ec_queue_sort(ctx, e, todo, n_items, st, *tmp, &a.todo); if (rc) return rc; }
            a.n_todo = n_items;
        }
        const uint64_t groups = (n_items + (uint64_t) a.batch - 1) / (uint64_t) a.batch;
        if (waves > groups) waves = groups;
        if (max_waves && waves > max_waves) waves = max_waves;
        if (!waves) return OATK_OK;
        if (kn.stages && mlog.size() < 64) a.memo_stat = cur + 64 + 3 * mlog.size(), mlog.push_back(EcMemoLog{tier, (unsigned long long) n_items, a.batch, (int) mlog.size()});
        if (t.hybrid) {
            void *p = nullptr;
            int rc = ec_slab_buf(ctx, e, hyb_k, (waves + ECW_WPB) * t.slab + 64, st, "the hybrid tier", "slabs", &p); if (rc) return rc;
            a.slabs = (uint8_t *) p, a.slab_bytes = t.slab;
        }
        ec_launch_lds_tier(t, waves, st, a);
        return OATK_OK;
    };
    // 1. route by length (one pass over the work items), then the LDS tiers side by side.  A long block is a long chain of dependent steps and
    //    its tier's carve-up lets few waves onto a CU, so run after the first tier the larger tiers are a tail of mostly idle CUs (0.8 ms for
    //    86 blocks at config 2; 4 waves per CU for 4 ms at config 3).  Run BESIDE it they must not crowd it out either: a larger tier starts
    //    first with a small share of every CU's LDS (a wave per CU, a wave per two CUs) and the first tier fills the rest.  Each larger tier
    //    is launched ONCE, with a wave of its own for every block routed to it (the second tier capped at two waves per CU).
    EcRoute rt;
    for (int t = 0; t <= LAST; ++t) rt.cap[t] = T[t].usable? T[t].cap_t : 0, rt.list[t] = list[t], rt.cnt[t] = cur + t;
    rt.cap[LAST] = 0x7FFFFFFF;
    // (measured: at config 2, 0.8 M blocks, side by side saves 0.9 of 3.7 ms.  At config 3, 7.9 M blocks, it used to cost more than the tails it hides
    //  -- 24.3 against 23.5 ms in r02 -- and was kept for small batches only; since r03 the first tier is known to run no faster with more than
    //  sixteen of its waves on a CU (DESIGN.md 8.3), the slots the larger tiers take cost it nothing, and side by side is 15.5 against 18.6 ms)
    const bool side_by_side = T[0].usable && !kn.serial_tiers && n_work;
    unsigned long long routed[4] = {0, 0, 0, 0}, done[4] = {0, 0, 0, 0}, cnts[4] = {0, 0, 0, 0};
    int used_aux = 0;
    if (side_by_side) {
        { int rc = ec_route(ctx, e, n_work, rt, routed, sizeof(routed)); if (rc) return rc; }
        { int rc = ec_fork_side_streams(ctx, e); if (rc) return rc; }
        for (int tier = LAST - 1; tier >= 1; --tier) {               // longest first.  A wave takes ONE long block at a time, so every routed block may have its own
            if (!T[tier].usable || !routed[tier]) continue;          // wave from the start (r04: 308 long blocks of the config-1 surrogate on 128 waves were 2.5 s)
            hipStream_t st = e->aux[used_aux];
            CK(hipStreamWaitEvent(st, e->fork_ev, 0));
            { int rc = launch(tier, list[tier], routed[tier], st, true, tier == 1? 2 * (uint64_t) ctx->n_cu : 0); if (rc) return rc; }
            CK(hipEventRecord(e->aux_ev[used_aux], st));
            ++used_aux;
            done[tier] = routed[tier];
        }
    }
    // nothing routed: the first usable tier takes everything
    const int first_tier = side_by_side || T[0].usable? 0 : next_usable(0);
    { int rc = launch(first_tier, nullptr, 0, ctx->stream, side_by_side); if (rc) return rc; }
    // 2. what a tier left over (frames or paths outgrew its carve-up; or, with nothing routed, everything too long) goes round again.  The first round starts as
    //    soon as the FIRST tier is done -- its left-overs are the deep searches, the longest chains of dependent steps of the batch, and they should not wait
    //    for the long blocks on the side streams --, later rounds when everything launched so far is done, until a round leaves nothing over.
    bool waited_aux = used_aux == 0;
    for (int round = 0; ; ++round) {
        CK(hipMemcpyAsync(cnts, cur, sizeof(cnts), hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        if (round == 0) n_big = cnts[1] + cnts[2] + routed[3];   // blocks the first tier did not finish: routed past it, or left over by it
        bool any = false;
        for (int tier = first_tier + 1; tier <= LAST; ++tier) {
            if (!T[tier].usable || cnts[tier] <= done[tier]) continue;
            { int rc = launch(tier, list[tier] + done[tier], cnts[tier] - done[tier], ctx->stream, false); if (rc) return rc; }
            done[tier] = cnts[tier];
            any = true;
        }
        if (!any && waited_aux) break;
        if (!waited_aux) { for (int i = 0; i < used_aux; ++i) CK(hipStreamWaitEvent(ctx->stream, e->aux_ev[i], 0)); waited_aux = true; }
    }
    if (kn.stages) { int rc = ec_memo_report(ctx, e, mlog); if (rc) return rc; }
    return OATK_OK;
}

// ---- the phases around the solve, in the order oatk_hip_ec_correct runs them; each works on ctx->stream and leaves what the next one reads in EcState ----
// a wave per read (ec.hpp: ECR_READS_PER_BLOCK reads to a workgroup)
static inline dim3 ec_read_blocks(uint64_t nr) { return dim3((unsigned) ((nr + ECR_READS_PER_BLOCK - 1) / ECR_READS_PER_BLOCK > 0? (nr + ECR_READS_PER_BLOCK - 1) / ECR_READS_PER_BLOCK : 1)); }

// the arcs that survive, squeezed, each with what the search needs about its target (ec.hpp: EcLiveArc); whether the live graph branches anywhere
static int ec_live_arcs(oatk_hip_ctx *ctx, EcState *e, EcLive &lv, bool &graph_branches)
{
    const uint64_t nv = e->g_n_vtx, na = e->g_n_arc;
    uint64_t n_live = 0;
    EENSURE(g_flags, 64);
    CK(hipMemsetAsync(e->g_flags.as<uint32_t>() + 8, 0, 12, ctx->stream));         // [8] a live vertex without its k-mer here, [9] the live graph branches, [10] a block beyond a read's staging entries
    EENSURE(live32, (na + 1) * 4); EENSURE(lidx_p, (2 * nv + 1) * 4); EENSURE(lidx_n, (2 * nv + 1) * 4);
    if (na) hipLaunchKernelGGL(ec_live_flag_kernel, grid256(na), dim3(256), 0, ctx->stream, na, (const uint8_t *) e->arc_del.p, e->live32.as<uint32_t>());
    { int rc = prim_scan_total_u32(ctx, e->live32, e->live64, e->live_off, na, &n_live); if (rc) return rc; }
    if (n_live >= 0xFFFFFFFFULL) { ctx->err = "error correction: more than 2^32 live arcs"; return OATK_E_ARG; }
    EENSURE(larc, (n_live + 1) * sizeof(EcLiveArc));
    e->n_live = n_live;
    hipLaunchKernelGGL(ec_live_idx_kernel, grid256(2 * nv), dim3(256), 0, ctx->stream, 2 * nv, e->idx_p.as<uint64_t>(), e->idx_n.as<uint32_t>(),
                       e->live_off.as<uint64_t>(), e->lidx_p.as<uint32_t>(), e->lidx_n.as<uint32_t>(), e->g_flags.as<uint32_t>() + 9);
    if (na) hipLaunchKernelGGL(ec_live_arc_kernel, grid256(na), dim3(256), 0, ctx->stream, na, (const uint8_t *) e->arc_del.p, e->live_off.as<uint64_t>(),
                               e->arc_w.as<uint64_t>(), e->arc_ls.as<uint32_t>(), e->vtx_hs_off.as<uint64_t>(), e->vtx_mpos.as<uint32_t>(),
                               e->lidx_p.as<uint32_t>(), e->lidx_n.as<uint32_t>(), e->larc.as<EcLiveArc>(), e->g_flags.as<uint32_t>() + 8);
    uint32_t fl[2] = {0, 0};
    CK(hipMemcpyAsync(fl, e->g_flags.as<uint32_t>() + 8, 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    const uint32_t no_src = fl[0];
    graph_branches = fl[1] != 0;
    if (no_src && ctx->n_occ) { ctx->err = "error correction: a live vertex has no k-mer on this shard (import it: oatk_hip_ec_import_kmers)"; return OATK_E_STATE; }
    lv.idx_p = e->lidx_p.as<uint32_t>(), lv.idx_n = e->lidx_n.as<uint32_t>(), lv.arc = e->larc.as<EcLiveArc>();
    return OATK_OK;
}

// the blocks of every read as the solver's work list (e->work, e->seg, e->blk_off), what the reads keep between their blocks (e->copy_n, e->keep_all), and with
// keep_seq a slot per block for its consensus
static int ec_list_blocks(oatk_hip_ctx *ctx, EcState *e, const EcReads &rd, const EcLive &lv, bool keep_seq, double max_edist, uint64_t &n_work)
{
    const uint64_t nr = ctx->n_reads, nocc = ctx->n_occ;
    EENSURE(n_blocks, (nr + 1) * 4);
    EENSURE(new_n, (nr + 1) * 4); EENSURE(copy_n, (nr + 1) * 4); EENSURE(keep_all, nr + 1);
    // One walk over the chains: it counts a read's blocks and stages their descriptors, n + 1 entries per read of n syncmers (ec.hpp: ec_stage_blocks_wave_kernel).
    // The staging array is val_occ, which nothing holds before the chains are assembled and which is of this size once they are (a buffer of its own would be
    // another 8 bytes per chain entry, 0.4 GB at 2 M reads).  Its last reader is ec_fill_work_kernel below; the assembly (ec_assemble_chains) is its next writer.
    const uint64_t stage_cap = nocc + nr + 1;
    e->staged_over = 0;
    static_assert(sizeof(EcSeg) == 8, "a staging entry is one val_occ entry");
    EENSURE(val_occ, stage_cap * sizeof(EcSeg));
    hipLaunchKernelGGL(ec_stage_blocks_wave_kernel, ec_read_blocks(nr), dim3(256), 0, ctx->stream, rd, (const uint8_t *) e->scm_del.p, e->n_blocks.as<uint32_t>(), e->copy_n.as<uint32_t>(),
                       e->keep_all.as<uint8_t>(), e->val_occ.as<EcSeg>(), stage_cap, e->g_flags.as<uint32_t>() + 10);
    CK(hipMemcpyAsync(&e->staged_over, e->g_flags.as<uint32_t>() + 10, 4, hipMemcpyDeviceToHost, ctx->stream));       // (waited for with the scan's total)
    n_work = 0;
    { int rc = prim_scan_total_u32(ctx, e->n_blocks, e->n_blocks64, e->blk_off, nr, &n_work); if (rc) return rc; }
    if (e->staged_over) { ctx->err = "error correction: a read has more error blocks than syncmers + 1 (the block walk's staging array)"; return OATK_E_STATE; }
    EENSURE(work, (n_work + 1) * sizeof(EcWork)); EENSURE(out, (n_work + 1) * sizeof(EcBlockOut));
    e->n_work = n_work;
    EENSURE(seg, (n_work + 1) * sizeof(EcSeg));
    hipLaunchKernelGGL(ec_fill_work_kernel, grid256(nr), dim3(256), 0, ctx->stream, rd, lv, e->blk_off.as<uint64_t>(), (const EcSeg *) e->val_occ.as<EcSeg>(), e->work.as<EcWork>(), e->seg.as<EcSeg>());
    // a fixed slot per block for its optimum consensus (oatk_hip_ec_keep_seq): no atomics, no overflow, and the same addresses whichever launch finishes a block
    if (keep_seq) {
        uint64_t slot_words = 0;
        EENSURE(slot_w, (n_work + 1) * 4); EENSURE(qend, (n_work + 1) * 4);
        if (n_work) hipLaunchKernelGGL(ec_slot_words_kernel, grid256(n_work), dim3(256), 0, ctx->stream, e->work.as<EcWork>(), n_work, max_edist, e->slot_w.as<uint32_t>());
        { int rc = prim_scan_total_u32(ctx, e->slot_w, e->slot_w64, e->slot_off, n_work, &slot_words); if (rc) return rc; }
        EENSURE(slots, (slot_words + 4) * 4);
    }
    return OATK_OK;
}

// the corrected chains (e->new_k, new_m, new_s behind e->new_off) and the (syncmer, occurrence) pairs of the refreshed table (e->key_id, e->val_occ): the block
// statistics, the chains' lengths and then the chains from the blocks' descriptors and outcomes, nobody walking a chain again (ec.hpp: EcSeg)
static int ec_assemble_chains(oatk_hip_ctx *ctx, EcState *e, const EcKnobs &kn, const EcReads &rd, const uint64_t *scm_s, uint64_t n_work, uint64_t &tot)
{
    const uint64_t nr = ctx->n_reads;
    EENSURE(new_n, (nr + 1) * 4);
    CK(hipMemsetAsync(e->stats.p, 0, 16 * 8, ctx->stream));
    EcAssembleArgs aa;
    aa.rd = rd, aa.scm_del = (const uint8_t *) e->scm_del.p, aa.scm_s = scm_s, aa.blk_off = e->blk_off.as<uint64_t>();
    aa.out = e->out.as<EcBlockOut>(), aa.path_pool = e->path_pool.as<uint64_t>(), aa.new_n = e->new_n.as<uint32_t>(), aa.new_off = nullptr;
    aa.new_k_mer = nullptr, aa.new_s_mer = nullptr, aa.new_m_pos = nullptr, aa.old_s_mer = ctx->pos_smer.as<uint64_t>();
    aa.stats = (unsigned long long *) e->stats.p, aa.pass = 1, aa.seg = e->seg.as<EcSeg>(), aa.keep_all = e->keep_all.as<uint8_t>();
    if (n_work) hipLaunchKernelGGL(ec_block_stats_kernel, dim3((unsigned) (n_work / 256 + 1 < 512? n_work / 256 + 1 : 512)), dim3(256), 0, ctx->stream, e->work.as<EcWork>(),
                                   e->out.as<EcBlockOut>(), n_work, (unsigned long long *) e->stats.p);
    hipLaunchKernelGGL(ec_new_n_seg_kernel, grid256(nr), dim3(256), 0, ctx->stream, nr, e->copy_n.as<uint32_t>(), e->blk_off.as<uint64_t>(), e->seg.as<EcSeg>(), e->out.as<EcBlockOut>(), e->new_n.as<uint32_t>());
    tot = 0;
    { int rc = prim_scan_total_u32(ctx, e->new_n, e->new_n64, e->new_off, nr, &tot); if (rc) return rc; }
    e->new_tot = tot;
    EENSURE(new_k, (tot + 1) * 8); EENSURE(new_m, (tot + 1) * 4); EENSURE(new_s, (tot + 1) * 8);
    // (val_occ held the block walk's staging entries until ec_fill_work_kernel had read them, ec_list_blocks: nothing may write it between the two)
    EENSURE(key_id, (tot + 1) * 4); EENSURE(key_sorted, (tot + 1) * 4); EENSURE(val_occ, (tot + 1) * 8); EENSURE(occ, (tot + 1) * 8);
    aa.new_off = e->new_off.as<uint64_t>(), aa.new_k_mer = e->new_k.as<uint64_t>(), aa.new_m_pos = e->new_m.as<uint32_t>(), aa.new_s_mer = e->new_s.as<uint64_t>();
    aa.key_id = e->key_id.as<uint32_t>(), aa.val_occ = e->val_occ.as<uint64_t>(), aa.sid0 = ctx->sid0;
    if (kn.assemble_pairs) hipLaunchKernelGGL(ec_assemble_pair_kernel, dim3((unsigned) ((nr + 7) / 8 > 0? (nr + 7) / 8 : 1)), dim3(256), 0, ctx->stream, aa);      // four waves, two reads each
    else hipLaunchKernelGGL(ec_assemble_seg_kernel, ec_read_blocks(nr), dim3(256), 0, ctx->stream, aa);
    return OATK_OK;
}

// update_syncmer_db (syncerr.c:769-814) from the `tot` pairs the assembly left: occurrence lists (e->occ behind e->occ_off), coverage, marks; `chk` is the
// coverage summed up, which the caller holds against tot
static int ec_refresh_table(oatk_hip_ctx *ctx, EcState *e, uint64_t tot, uint64_t &chk)
{
    const uint64_t nv = e->g_n_vtx;
    EENSURE(cov, (nv + 1) * 4); EENSURE(fwd, (nv + 1) * 4);
    CK(hipMemsetAsync(e->cov.p, 0, (nv + 1) * 4, ctx->stream));
    CK(hipMemsetAsync(e->fwd.p, 0, (nv + 1) * 4, ctx->stream));
    if (tot) {
        unsigned id_bits = 1;   // the keys are syncmer ids: the passes stop at the id's highest bit
        while (id_bits < 32 && (nv - 1) >> id_bits) ++id_bits;
        // stable: occurrences of one syncmer stay in (sid, idx) order (syncerr.c:796-805)
        PRIM(rocprim::radix_sort_pairs, e->key_id.as<uint32_t>(), e->key_sorted.as<uint32_t>(), e->val_occ.as<uint64_t>(), e->occ.as<uint64_t>(), tot, 0, id_bits, ctx->stream);
        // coverage and forward-strand counts per syncmer from the sorted lists: one pass over the runs (cov and fwd are zero: runs that cross a wave's tile add up)
        hipLaunchKernelGGL(ec_cov_runs_kernel, grid256(tot), dim3(256), 0, ctx->stream, tot, e->key_sorted.as<uint32_t>(), e->occ.as<uint64_t>(), e->cov.as<uint32_t>(), e->fwd.as<uint32_t>());
    }
    hipLaunchKernelGGL(ec_del_kernel, grid256(nv), dim3(256), 0, ctx->stream, nv, e->fwd.as<uint32_t>(), e->scm_del.as<uint8_t>());
    chk = 0;
    return prim_scan_total_u32(ctx, e->cov, e->cov64, e->occ_off, nv, &chk);
}

}  // namespace oatk

// the rest of read_error_correction (syncerr.c:819): blocks, search, corrected chains, refreshed table
extern "C" int oatk_hip_ec_correct(oatk_hip_ctx *ctx, double max_edist)
{
    using namespace oatk;
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->ec || !ctx->ec->marked) { ctx->err = "oatk_hip_ec_correct needs oatk_hip_ec_mark"; return OATK_E_STATE; }
    CK(hipSetDevice(ctx->device));
    EcState *e = ctx->ec;
    e->done = false, e->cseq_done = false;
    const bool keep_seq = e->keep_seq;                     // (sharded reads too: a rank corrects its own reads, and the slots are per block of this handle)
    e->seq_kept = false;
    const EcKnobs kn = ec_knobs_read();
    EC_VIEWS();
    (void) nv; (void) na; (void) nr;
    // ---- live arcs, blocks ----
    EcLive lv;
    bool graph_branches = true;
    { int rc = ec_live_arcs(ctx, e, lv, graph_branches); if (rc) return rc; }
    uint64_t n_work = 0;
    { int rc = ec_list_blocks(ctx, e, rd, lv, keep_seq, max_edist, n_work); if (rc) return rc; }
    t_end(ctx, OATK_T_EC_MARK);
    t_begin(ctx, OATK_T_EC_SOLVE);

    // ---- solve ----
    // Which solver (r06).  A search is a walk when no vertex of the live graph has two arcs out: one candidate per level, as many levels as the block is long -- nothing
    // to bound.  Round 4's tiers do such a batch 1.2 - 2.5 ms faster at config 3 (14.7 against 15.9 - 17.3 ms; tools/solverbench.py, DESIGN.md 7): there every search
    // is one, the light graph of a random genome at 30 x has 15 350 arcs and not one vertex with two (tools/graph_branching.py).  With a single branching vertex the
    // classes with budgets and the second stage run: the config-1 surrogate has 304, and its searches are what they were built for (0.23 s against 3.2).
    const bool heavy = kn.heavy < 0? graph_branches : kn.heavy != 0;
    uint64_t pool_cap = 2 * nocc + (uint64_t) 16384 * ECW_POOL_CHUNK + 4096;
    EENSURE(cursor, 512 + 192 * 8); EENSURE(stats, 16 * 8);              // (behind the 64 counters: three per launch of the wave solver, OATK_DEBUG_EC_STAGES)
    uint64_t n_big = 0;
    uint32_t max_hl = 0;                 // the longest read of the batch, once the slab tier has needed it
    for (;;) {
        EENSURE(path_pool, pool_cap * 8);
        CK(hipMemsetAsync(e->cursor.p, 0, 512 + 192 * 8, ctx->stream));
        EcwArgs base = {};               // what every launch shares; each sets the rest of its own
        base.lv = lv, base.rd = rd, base.work = e->work.as<EcWork>(), base.n_work = n_work, base.max_edist = max_edist;
        base.out = e->out.as<EcBlockOut>(), base.path_pool = e->path_pool.as<uint64_t>(), base.pool_cap = pool_cap;
        base.memo = kn.memo, base.regroup = kn.regroup;
        base.pool_cursor = (unsigned long long *) e->cursor.p;       // [0] pool, then the lists' and work queues' counters; [63] blocks that outgrew the slabs
        if (keep_seq) {
            CK(hipMemsetAsync(e->qend.p, 0, (n_work + 1) * 4, ctx->stream));
            base.seq_qend = e->qend.as<uint32_t>(), base.seq_slots = e->slots.as<uint32_t>(), base.seq_slot_off = e->slot_off.as<uint64_t>();
        }
        if (kn.stages) fprintf(stderr, "[ec stages] the live graph %s: %s\n", graph_branches? "branches" : "does not branch", heavy? "classes with budgets, second stage" : "round 4's tiers");
        { int rc = heavy? ec_solve_classes(ctx, e, kn, base, max_hl, n_big) : ec_solve_tiers(ctx, e, kn, base, max_hl, n_big); if (rc) return rc; }
        unsigned long long fin = 0, used = 0;
        CK(hipMemcpyAsync(&fin, base.pool_cursor + 63, 8, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        if (fin) { ctx->err = "error correction: a block outgrew the large scratch slab (DFS deeper than 4 MiB of frames)"; return OATK_E_NOMEM; }
        CK(hipMemcpyAsync(&used, e->cursor.p, 8, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        if (used <= pool_cap) break;
        pool_cap = used + used / 4 + 4096;          // the pool overflowed: grow it and solve again
    }

    // ---- corrected chains, refreshed table ----
    t_end(ctx, OATK_T_EC_SOLVE);
    t_begin(ctx, OATK_T_EC_REFRESH);
    uint64_t tot = 0, chk = 0;
    { int rc = ec_assemble_chains(ctx, e, kn, rd, g.scm_s, n_work, tot); if (rc) return rc; }
    { int rc = ec_refresh_table(ctx, e, tot, chk); if (rc) return rc; }
    unsigned long long st[16];
    CK(hipMemcpyAsync(st, e->stats.p, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
    t_end(ctx, OATK_T_EC_REFRESH);
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    t_collect(ctx, OATK_T_EC_MARK, OATK_T_EC_REFRESH);
    for (int i = 0; i < 11; ++i) e->stats_h[i] = st[i];
    e->stats_h[11] = n_big;
    if (chk != tot) { ctx->err = "error correction: coverage does not add up"; return OATK_E_STATE; }
    e->done = true, e->seq_kept = keep_seq, e->seq_global = e->global;
    return OATK_OK;
}

extern "C" int oatk_hip_ec_keep_seq(oatk_hip_ctx *ctx, int on)
{
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->ec) ctx->ec = new EcState();
    ctx->ec->keep_seq = on != 0;
    return OATK_OK;
}

// the corrected reads' sequences from what a correction with the switch on left resident (ec_seq.hpp): lengths, offsets, then the strings
extern "C" int oatk_hip_ec_corrected_reads(oatk_hip_ctx *ctx, uint64_t *n_bases)
{
    using namespace oatk;
    if (!ctx) return OATK_E_NODEV;
    EcState *e = ctx->ec;
    // (a change of id space drops the correction as a scan does -- oatk_hip_ec_set_global, api.hip: scan_reset_downstream --; named here because the blocks and slots
    //  of the old space are still allocated and must never be read against the new one)
    if (e && e->seq_kept && e->seq_global != e->global) {
        ctx->err = e->global? "oatk_hip_ec_corrected_reads: the resident correction was made on one handle's ids and the handle is sharded now (correct again: oatk_hip_ec_sharded)"
                            : "oatk_hip_ec_corrected_reads: the resident correction was made on sharded reads (global ids) and the handle is not sharded any more (correct again)";
        return OATK_E_STATE;
    }
    if (!e || !e->done || !e->seq_kept || !ctx->scanned) { ctx->err = "oatk_hip_ec_corrected_reads needs a correction of the resident batch made with oatk_hip_ec_keep_seq"; return OATK_E_STATE; }
    CK(hipSetDevice(ctx->device));
    e->cseq_done = false;          // (a call that fails half-way leaves nothing readable)
    EC_VIEWS();
    (void) g;
    const uint64_t n_work = e->n_work;
    // OATK_DEBUG_EC_STAGES: the two passes' durations on stderr (tests/ec_seq_time.py)
    const bool stages = getenv("OATK_DEBUG_EC_STAGES") != nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    if (stages) for (int i = 0; i < 3; ++i) CK(hipEventCreate(&ev[i]));
    EENSURE(sblk, (n_work + nr + 1) * sizeof(EcSeqBlk)); EENSURE(clen, (nr + 1) * 4); EENSURE(cbytes, (nr + 1) * 4);
    if (stages) CK(hipEventRecord(ev[0], ctx->stream));
    if (nr) hipLaunchKernelGGL(ec_cseq_len_kernel, grid256(nr), dim3(256), 0, ctx->stream, rd, e->blk_off.as<uint64_t>(), e->work.as<EcWork>(), e->out.as<EcBlockOut>(), e->qend.as<uint32_t>(),
                               e->sblk.as<EcSeqBlk>(), e->clen.as<uint32_t>(), e->cbytes.as<uint32_t>());
    uint64_t bytes = 0;
    { int rc = prim_scan_total_u32(ctx, e->cbytes, e->cbytes64, e->coff, nr, &bytes); if (rc) return rc; }
    EENSURE(cseq, bytes + 16);
    if (stages) CK(hipEventRecord(ev[1], ctx->stream));
    EcSeqArgs sa;
    sa.rd = rd, sa.blk_off = e->blk_off.as<uint64_t>(), sa.sb = e->sblk.as<EcSeqBlk>(), sa.slots = e->slots.as<uint32_t>(), sa.slot_off = e->slot_off.as<uint64_t>();
    sa.coff = e->coff.as<uint64_t>(), sa.cseq = e->cseq.as<uint8_t>();
    if (nr) hipLaunchKernelGGL(ec_cseq_write_kernel, dim3((unsigned) ((nr + 3) / 4)), dim3(256), 0, ctx->stream, sa);
    if (stages) {
        float ms_len = 0.f, ms_write = 0.f;
        CK(hipEventRecord(ev[2], ctx->stream));
        CK(hipEventSynchronize(ev[2]));
        CK(hipEventElapsedTime(&ms_len, ev[0], ev[1]));
        CK(hipEventElapsedTime(&ms_write, ev[1], ev[2]));
        for (int i = 0; i < 3; ++i) (void) hipEventDestroy(ev[i]);
        fprintf(stderr, "[ec stages] corrected reads: lengths + offsets %.3f ms, strings %.3f ms (%llu reads, %llu blocks, %llu bytes written)\n", ms_len, ms_write,
                (unsigned long long) nr, (unsigned long long) n_work, (unsigned long long) bytes);
    }
    if (n_bases) {
        // (bases, not bytes: the offsets count every read's pad)
        std::vector<uint32_t> cl(nr);
        if (nr) CK(hipMemcpyAsync(cl.data(), e->clen.p, nr * 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        uint64_t s = 0;
        for (uint64_t i = 0; i < nr; ++i) s += cl[i];
        *n_bases = s;
    }
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    e->cseq_bytes = bytes, e->cseq_done = true;
    return OATK_OK;
}

extern "C" int oatk_hip_ec(oatk_hip_ctx *ctx, const oatk_ec_graph_t *hg, double max_edist, uint32_t err_mer_c, uint32_t max_err_c,
                           uint32_t err_arc_c, double max_arc_f)
{
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->counted) { ctx->err = "oatk_hip_ec needs a resident scan + count"; return OATK_E_STATE; }
    if (!hg && !(ctx->ec && ctx->ec->graph_resident)) { ctx->err = "oatk_hip_ec(NULL graph) needs oatk_hip_ec_graph first"; return OATK_E_STATE; }
    CK(hipSetDevice(ctx->device));
    if (!ctx->ec) ctx->ec = new EcState();
    int rc;
    if (hg) {
        if (hg->n_vtx != ec_n_vtx(ctx)) { ctx->err = "EC graph must have one vertex per syncmer of the resident count"; return OATK_E_ARG; }
        // the marking starts from clean flags, as it does on the graph make_syncmer_graph(…, 0, 0.) returns
        for (uint64_t i = 0; i < hg->n_arc; ++i) if (hg->arc_del[i]) { ctx->err = "an EC graph that already carries deleted arcs is not supported"; return OATK_E_ARG; }
        if ((rc = ec_upload_graph(ctx, hg)) != OATK_OK) return rc;
    }
    if ((rc = oatk_hip_ec_mark(ctx, err_mer_c, max_err_c, err_arc_c, max_arc_f)) != OATK_OK) return rc;
    return oatk_hip_ec_correct(ctx, max_edist);
}

#ifdef ECF_PROF2
// development builds: the per-arc phase profile of the second stage's kernels (ec_fused.hpp), read and cleared
extern "C" int oatk_hip_debug_ecf_prof2(oatk_hip_ctx *ctx, unsigned long long *out120)
{
    if (!ctx) return OATK_E_NODEV;
    CK(hipSetDevice(ctx->device));
    CK(hipDeviceSynchronize());
    CK(hipMemcpyFromSymbol(out120, HIP_SYMBOL(oatk::ecf_prof2), 140 * 8));
    unsigned long long z[140] = {0};
    CK(hipMemcpyToSymbol(HIP_SYMBOL(oatk::ecf_prof2), z, 140 * 8));
    return OATK_OK;
}
#endif
