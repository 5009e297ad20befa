// oatk_amd/csrc/api_cons.inc -- C ABI of the device syncmer consensus (include/oatk_hip_cons.h); part of api.hip, after api_ec.inc.
#include "../../include/oatk_hip_cons.h"
#include "consensus.hpp"

struct ConsState {
    DevBuf flag, flag64, slot_of, sel, slot, rl, tot, m_seq, first, nch, ch_off;
    uint64_t n_sel = 0, n_scm = 0;
    int K = 0;
    bool done = false;
    // sharded reads: every selected syncmer's own k-mer (api_consstr.inc: oatk_hip_consensus_strings_sharded makes it once per consensus)
    DevBuf kmer;
    uint64_t kmer_stride = 0;
    bool kmer_valid = false;
    hipEvent_t kmer_ev[2] = {nullptr, nullptr};
    float kmer_ms = 0.f;
    ~ConsState() { for (hipEvent_t e : kmer_ev) if (e) (void) hipEventDestroy(e); }
};

static void cons_state_free(oatk_hip_ctx *ctx)
{
    delete ctx->cons;          // (its buffers free themselves: ~DevBuf)
    ctx->cons = nullptr;
}

static int cons_buffer(oatk_hip_ctx *ctx, int which, const void **d_ptr, uint64_t *bytes)
{
    ConsState *c = ctx->cons;
    if (!c || !c->done) { ctx->err = "unknown buffer id, or consensus results requested before oatk_hip_consensus"; return OATK_E_STATE; }
    switch (which) {
        case OATK_BUF_CONS_SEL: *d_ptr = c->sel.p, *bytes = c->n_sel * 4; break;
        case OATK_BUF_CONS_SLOT: *d_ptr = c->slot.p, *bytes = c->n_scm * 4; break;
        case OATK_BUF_CONS_RL: *d_ptr = c->rl.p, *bytes = c->n_sel * (uint64_t) c->K * 4; break;
        case OATK_BUF_CONS_MSEQ: *d_ptr = c->m_seq.p, *bytes = c->n_sel * 4; break;
        case OATK_BUF_CONS_FIRST: *d_ptr = c->first.p, *bytes = c->n_sel * 8; break;
        case OATK_BUF_CONS_TOT: *d_ptr = c->tot.p, *bytes = c->n_sel * (uint64_t) c->K * 8; break;
        default: ctx->err = "unknown buffer id"; return OATK_E_ARG;
    }
    return OATK_OK;
}

#define CENSURE(buf, bytes) ENSURE_IN(c, "cons.", buf, bytes)

// run-length totals of the syncmers listed in c->sel[0..n_sel)
static int cons_run(oatk_hip_ctx *ctx, ConsState *c, uint64_t n_sel)
{
    using namespace oatk;
    const bool after_ec = ctx->ec && ctx->ec->done;
    EcState *e = ctx->ec;
    CENSURE(rl, (n_sel * (uint64_t) ctx->K + 1) * 4); CENSURE(tot, (n_sel * (uint64_t) ctx->K + 1) * 8); CENSURE(m_seq, (n_sel + 1) * 4); CENSURE(first, (n_sel + 1) * 8);
    if (n_sel) {
        if (n_sel > 0x7FFFFFFFULL) { ctx->err = "too many syncmers selected for consensus"; return OATK_E_ARG; }
        ConsArgs a;
        a.n_sel = n_sel, a.sel = c->sel.as<uint32_t>(), a.sid0 = ctx->sid0, a.off = ctx->d_off, a.ho_rl = ctx->ho_rl.as<uint8_t>(), a.K = ctx->K;
        a.occ_off = after_ec? e->occ_off.as<uint64_t>() : ctx->scm_occ_off.as<uint64_t>();
        a.occ = after_ec? e->occ.as<uint64_t>() : ctx->scm_occ.as<uint64_t>();
        a.chain_off = after_ec? e->new_off.as<uint64_t>() : ctx->scm_off.as<uint64_t>();
        a.k_mer = after_ec? e->new_k.as<uint64_t>() : ctx->pos_kid.as<uint64_t>();
        a.m_pos = after_ec? e->new_m.as<uint32_t>() : ctx->pos_mpos.as<uint32_t>();
        a.lrl_key = ctx->lrl_sorted_in_2? ctx->lrl_key2.as<uint64_t>() : ctx->lrl_key.as<uint64_t>();
        a.lrl_val = ctx->lrl_sorted_in_2? ctx->lrl_val2.as<uint32_t>() : ctx->lrl_val.as<uint32_t>();
        a.n_lrl = ctx->tot_lrl;
        a.cons_rl = c->rl.as<uint32_t>(), a.cons_tot = (unsigned long long *) c->tot.p, a.m_seq = c->m_seq.as<uint32_t>(), a.first_occ = c->first.as<uint64_t>();
        // workgroups: one per CONS_CHUNK occurrences of a syncmer (consensus.hpp)
        CENSURE(nch, (n_sel + 2) * 8); CENSURE(ch_off, (n_sel + 2) * 8);
        hipLaunchKernelGGL(cons_chunks_kernel, dim3((unsigned) ((n_sel + 1 + 255) / 256)), dim3(256), 0, ctx->stream, n_sel, a.sel, a.occ_off, c->nch.as<uint64_t>());
        uint64_t n_wg = 0;
        { int rc = prim_scan_total(ctx, ctx->tmp, c->nch.as<uint64_t>(), c->ch_off.as<uint64_t>(), n_sel, &n_wg); if (rc) return rc; }
        if (n_wg > 0x7FFFFFFFULL) { ctx->err = "too many occurrences selected for consensus"; return OATK_E_ARG; }
        a.ch_off = c->ch_off.as<uint64_t>(), a.n_wg = n_wg;
        if (n_wg > n_sel) hipLaunchKernelGGL(cons_zero_shared_kernel, dim3((unsigned) n_sel), dim3(256), 0, ctx->stream, a);
        hipLaunchKernelGGL(cons_rl_kernel, dim3((unsigned) n_wg), dim3(256), 0, ctx->stream, a);
        if (n_wg > n_sel) hipLaunchKernelGGL(cons_finish_shared_kernel, dim3((unsigned) n_sel), dim3(256), 0, ctx->stream, a);
    }
    return OATK_OK;
}

extern "C" int oatk_hip_consensus_ids(oatk_hip_ctx *ctx, const uint32_t *d_ids, uint64_t n)
{
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->counted) { ctx->err = "oatk_hip_consensus_ids needs a resident scan + count"; return OATK_E_STATE; }
    const bool global = ctx->ec && ctx->ec->global;
    if (global && !ctx->ec->done) { ctx->err = "oatk_hip_consensus_ids: with sharded reads, after oatk_hip_ec_correct"; return OATK_E_STATE; }
    CK(hipSetDevice(ctx->device));
    if (!ctx->cons) ctx->cons = new ConsState();
    ConsState *c = ctx->cons;
    c->done = false, c->kmer_valid = false;
    c->n_scm = 0, c->K = ctx->K, c->n_sel = n;          // CONS_SLOT is not kept for a caller-chosen list
    CENSURE(sel, (n + 1) * 4);
    if (n) CK(hipMemcpyAsync(c->sel.p, d_ids, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    { int rc = cons_run(ctx, c, n); if (rc) return rc; }
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    c->done = true;
    return OATK_OK;
}

// the syncmers the consensus is made for: not deleted, seen at least min_cov times (and at all); c->sel the list, c->slot its inverse over all ns
static int cons_select(oatk_hip_ctx *ctx, ConsState *c, uint64_t ns, const uint32_t *cov, const uint8_t *del, uint32_t min_cov, uint64_t *n_sel_out)
{
    using namespace oatk;
    CENSURE(flag, (ns + 1) * 4); CENSURE(slot, (ns + 1) * 4);
    hipLaunchKernelGGL(cons_flag_kernel, grid256(ns), dim3(256), 0, ctx->stream, ns, cov, del, min_cov, c->flag.as<uint32_t>());
    uint64_t n_sel = 0;
    { int rc = prim_scan_total_u32(ctx, c->flag, c->flag64, c->slot_of, ns, &n_sel); if (rc) return rc; }      // exclusive scan of the flags = slots
    c->n_sel = n_sel;
    CENSURE(sel, (n_sel + 1) * 4);
    hipLaunchKernelGGL(cons_select_kernel, grid256(ns), dim3(256), 0, ctx->stream, ns, c->flag.as<uint32_t>(), c->slot_of.as<uint64_t>(), c->sel.as<uint32_t>(),
                       c->slot.as<uint32_t>());
    *n_sel_out = n_sel;
    return OATK_OK;
}

extern "C" int oatk_hip_consensus(oatk_hip_ctx *ctx, uint32_t min_cov)
{
    using namespace oatk;
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->counted) { ctx->err = "oatk_hip_consensus needs a resident scan + count"; return OATK_E_STATE; }
    if (ctx->ec && ctx->ec->global) { ctx->err = "oatk_hip_consensus: reads are sharded; oatk_hip_consensus_sharded adds the shards' totals up (include/oatk_hip_multi.h)"; return OATK_E_STATE; }
    CK(hipSetDevice(ctx->device));
    if (!ctx->cons) ctx->cons = new ConsState();
    ConsState *c = ctx->cons;
    c->done = false, c->kmer_valid = false;
    const bool after_ec = ctx->ec && ctx->ec->done;
    EcState *e = ctx->ec;
    const uint64_t ns = ctx->n_scm_total;
    c->n_scm = ns, c->K = ctx->K, c->n_sel = 0;
    if (ns == 0) { c->done = true; return OATK_OK; }
    const uint32_t *cov = after_ec? e->cov.as<uint32_t>() : ctx->scm_cov.as<uint32_t>();
    const uint8_t *del = after_ec? e->scm_del.as<uint8_t>() : (const uint8_t *) nullptr;
    uint64_t n_sel = 0;
    { int rc = cons_select(ctx, c, ns, cov, del, min_cov, &n_sel); if (rc) return rc; }
    { int rc = cons_run(ctx, c, n_sel); if (rc) return rc; }
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    c->done = true;
    return OATK_OK;
}
