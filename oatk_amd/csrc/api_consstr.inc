// oatk_amd/csrc/api_consstr.inc -- C ABI of the consensus strings on the device (include/oatk_hip_cons.h: oatk_hip_consensus_strings); part of api.hip, after
// api_cons.inc, whose resident tables it reads.
#include "cons_str.hpp"

struct ConsStrState {
    DevBuf seq_off, piece_v, piece_beg, want, piece_len, piece_bad, piece_put, piece_at, str, str_off, str_len, status, scan_tmp;
    uint64_t n_seq = 0, n_piece = 0, total = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};      // length kernel, fill kernel: begin and end
    float ms[2] = {0.f, 0.f};
    bool done = false;
    ~ConsStrState() { for (hipEvent_t e : ev) if (e) (void) hipEventDestroy(e); }
};

static void consstr_state_free(oatk_hip_ctx *ctx)
{
    delete ctx->cstr;          // (its buffers free themselves: ~DevBuf)
    ctx->cstr = nullptr;
}

static int consstr_buffer(oatk_hip_ctx *ctx, int which, const void **d_ptr, uint64_t *bytes)
{
    ConsStrState *g = ctx->cstr;
    if (!g || !g->done) { ctx->err = "consensus strings requested before oatk_hip_consensus_strings"; return OATK_E_STATE; }
    switch (which) {
        case OATK_BUF_CONS_STR: *d_ptr = g->str.p, *bytes = g->total; break;
        case OATK_BUF_CONS_STR_OFF: *d_ptr = g->str_off.p, *bytes = (g->n_seq + 1) * 8; break;
        case OATK_BUF_CONS_STR_LEN: *d_ptr = g->str_len.p, *bytes = g->n_seq * 8; break;
        case OATK_BUF_CONS_STR_STATUS: *d_ptr = g->status.p, *bytes = g->n_seq; break;
        default: ctx->err = "unknown buffer id"; return OATK_E_ARG;
    }
    return OATK_OK;
}

#define SENSURE(buf, bytes) ENSURE_IN(g, "consstr.", buf, bytes)

// the plan as the kernels will index it: offsets ascending from 0 to n_piece, every syncmer known, every beg below k
static const char *consstr_plan_error(const oatk_cons_plan_t *p, uint64_t n_scm, int k)
{
    if (p->n_seq && !p->seq_off) return "oatk_hip_consensus_strings: no sequence offsets";
    if (p->n_piece && (!p->piece_v || !p->piece_beg)) return "oatk_hip_consensus_strings: no pieces";
    if (p->n_seq == 0) return p->n_piece? "oatk_hip_consensus_strings: pieces without a sequence" : nullptr;
    if (p->seq_off[0] != 0 || p->seq_off[p->n_seq] != p->n_piece) return "oatk_hip_consensus_strings: the sequence offsets do not run from 0 to n_piece";
    for (uint64_t s = 0; s < p->n_seq; ++s)
        if (p->seq_off[s] > p->seq_off[s + 1]) return "oatk_hip_consensus_strings: the sequence offsets descend";
    for (uint64_t i = 0; i < p->n_piece; ++i) {
        if ((p->piece_v[i] >> 1) >= n_scm) return "oatk_hip_consensus_strings: a piece names a syncmer that does not exist";
        if (p->piece_beg[i] >= k) return "oatk_hip_consensus_strings: a piece begins at or behind position k (the reference asserts beg < k)";
    }
    return nullptr;
}

// the consensus tables and this handle's reads as a piece is opened from them (cons_str_core.hpp); T.kmer stays unset
static oatk_cstr::Tables consstr_tables(oatk_hip_ctx *ctx, ConsState *c)
{
    const bool after_ec = ctx->ec && ctx->ec->done;      // the chains cons_run handed to cons_rl_kernel: CONS_FIRST indexes them
    EcState *e = ctx->ec;
    oatk_cstr::Tables T;
    T.n_scm = c->n_scm, T.k = c->K, T.slot = c->slot.as<uint32_t>(), T.rl = c->rl.as<uint32_t>(), T.m_seq = c->m_seq.as<uint32_t>();
    T.first = c->first.as<uint64_t>(), T.sid0 = ctx->sid0, T.off = ctx->d_off, T.hoco_s = ctx->hoco_s.as<uint8_t>();
    T.chain_off = after_ec? e->new_off.as<uint64_t>() : ctx->scm_off.as<uint64_t>();
    T.m_pos = after_ec? e->new_m.as<uint32_t>() : ctx->pos_mpos.as<uint32_t>();
    return T;
}

// the string phases of a checked plan over the tables T: what oatk_hip_consensus_strings and oatk_hip_consensus_strings_sharded (api_consstr_multi.inc) both run
static int consstr_run(oatk_hip_ctx *ctx, const oatk_cons_plan_t *plan, int hoco_seq, const oatk_cstr::Tables &T, uint64_t *total_bytes, uint64_t *n_refused)
{
    using namespace oatk;
    CK(hipSetDevice(ctx->device));
    if (!ctx->cstr) ctx->cstr = new ConsStrState();
    ConsStrState *g = ctx->cstr;
    g->done = false, g->ms[0] = g->ms[1] = 0.f;
    const uint64_t ns = plan->n_seq, np = plan->n_piece;
    if (np > 0x7FFFFFFFULL * CSTR_WAVES || ns >= 0x7FFFFFFFULL * CSTR_WAVES) { ctx->err = "oatk_hip_consensus_strings: too many pieces"; return OATK_E_ARG; }
    SENSURE(seq_off, (ns + 1) * 8); SENSURE(piece_v, (np + 1) * 8); SENSURE(piece_beg, (np + 1) * 4); SENSURE(want, ns + 1);
    SENSURE(piece_len, (np + 1) * 8); SENSURE(piece_bad, np + 1); SENSURE(piece_put, (np + 1) * 8); SENSURE(piece_at, (np + 1) * 8);
    SENSURE(str_off, (ns + 1) * 8); SENSURE(str_len, (ns + 1) * 8); SENSURE(status, ns + 1);
    const uint64_t zero = 0;
    CK(hipMemcpyAsync(g->seq_off.p, ns? (const void *) plan->seq_off : (const void *) &zero, (ns + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (np) {
        CK(hipMemcpyAsync(g->piece_v.p, plan->piece_v, np * 8, hipMemcpyHostToDevice, ctx->stream));
        CK(hipMemcpyAsync(g->piece_beg.p, plan->piece_beg, np * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    if (ns && plan->want_bytes) CK(hipMemcpyAsync(g->want.p, plan->want_bytes, ns, hipMemcpyHostToDevice, ctx->stream));

    CstrArgs a;
    a.T = T;
    a.n_seq = ns, a.n_piece = np, a.seq_off = g->seq_off.as<uint64_t>(), a.piece_v = g->piece_v.as<uint64_t>(), a.piece_beg = g->piece_beg.as<int32_t>();
    a.want = plan->want_bytes? g->want.as<uint8_t>() : nullptr, a.hoco_seq = hoco_seq;
    a.piece_len = g->piece_len.as<uint64_t>(), a.piece_bad = g->piece_bad.as<uint8_t>(), a.piece_put = g->piece_put.as<uint64_t>(), a.piece_at = g->piece_at.as<uint64_t>();
    a.str_off = g->str_off.as<uint64_t>(), a.str_len = g->str_len.as<uint64_t>(), a.status = g->status.as<uint8_t>(), a.str = nullptr, a.total = 0;
    const bool timing = ctx->timing;
    if (timing) for (hipEvent_t &ev : g->ev) if (!ev) CK(hipEventCreate(&ev));
    const dim3 piece_grid((unsigned) ((np + CSTR_WAVES - 1) / CSTR_WAVES)), seq_grid((unsigned) ((ns + 1 + CSTR_WAVES - 1) / CSTR_WAVES));
    if (timing) CK(hipEventRecord(g->ev[0], ctx->stream));
    if (np) hipLaunchKernelGGL(cstr_len_kernel, piece_grid, dim3(64 * CSTR_WAVES), 0, ctx->stream, a);
    if (timing) CK(hipEventRecord(g->ev[1], ctx->stream));
    hipLaunchKernelGGL(cstr_seq_kernel, seq_grid, dim3(64 * CSTR_WAVES), 0, ctx->stream, a);
    uint64_t total = 0;
    { int rc = prim_scan_total(ctx, g->scan_tmp, g->piece_put.as<uint64_t>(), g->piece_at.as<uint64_t>(), np, &total); if (rc) return rc; }
    hipLaunchKernelGGL(cstr_off_kernel, grid256(ns + 1), dim3(256), 0, ctx->stream, a);
    SENSURE(str, total + 1);
    a.str = g->str.as<uint8_t>(), a.total = total;
    if (timing) CK(hipEventRecord(g->ev[2], ctx->stream));
    if (np && total) hipLaunchKernelGGL(cstr_fill_kernel, piece_grid, dim3(64 * CSTR_WAVES), 0, ctx->stream, a);
    if (timing) CK(hipEventRecord(g->ev[3], ctx->stream));
    std::vector<uint8_t> st(ns);                         // graph-sized: how many sequences were refused
    if (ns) CK(hipMemcpyAsync(st.data(), g->status.p, ns, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    if (timing) { CK(hipEventElapsedTime(&g->ms[0], g->ev[0], g->ev[1])); CK(hipEventElapsedTime(&g->ms[1], g->ev[2], g->ev[3])); }
    uint64_t refused = 0;
    for (uint8_t x : st) refused += x != 0;
    g->n_seq = ns, g->n_piece = np, g->total = total, g->done = true;
    if (total_bytes) *total_bytes = total;
    if (n_refused) *n_refused = refused;
    return OATK_OK;
}

extern "C" int oatk_hip_consensus_strings(oatk_hip_ctx *ctx, const oatk_cons_plan_t *plan, int hoco_seq, uint64_t *total_bytes, uint64_t *n_refused)
{
    if (!ctx) return OATK_E_NODEV;
    if (!plan) { ctx->err = "oatk_hip_consensus_strings: no plan"; return OATK_E_ARG; }
    if (ctx->ec && ctx->ec->global) {
        ctx->err = "oatk_hip_consensus_strings: reads are sharded; oatk_hip_consensus_strings_sharded makes the strings from all shards (include/oatk_hip_multi.h)";
        return OATK_E_STATE;
    }
    ConsState *c = ctx->cons;
    if (!ctx->counted || !c || !c->done || (c->n_scm == 0 && c->n_sel != 0)) {      // (oatk_hip_consensus_ids keeps no CONS_SLOT)
        ctx->err = "oatk_hip_consensus_strings needs oatk_hip_consensus done on the resident batch";
        return OATK_E_STATE;
    }
    if (const char *why = consstr_plan_error(plan, c->n_scm, c->K)) { ctx->err = why; return OATK_E_ARG; }
    return consstr_run(ctx, plan, hoco_seq, consstr_tables(ctx, c), total_bytes, n_refused);
}

extern "C" int oatk_hip_consensus_strings_times(oatk_hip_ctx *ctx, float *ms2, uint64_t *n_piece)
{
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->cstr || !ctx->cstr->done) { ctx->err = "oatk_hip_consensus_strings_times: no strings made yet"; return OATK_E_STATE; }
    ms2[0] = ctx->cstr->ms[0], ms2[1] = ctx->cstr->ms[1];
    if (n_piece) *n_piece = ctx->cstr->n_piece;
    return OATK_OK;
}
