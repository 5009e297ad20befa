// oatk_amd/csrc/api_consstr_multi.inc -- the consensus strings for reads sharded over several handles (include/oatk_hip_multi.h:
// oatk_hip_consensus_strings_sharded); part of api.hip, after api_consstr.inc (whose string phases it runs) and api_multi_tail.inc (whose consensus it reads).
//
// After oatk_hip_consensus_sharded CONS_SLOT, CONS_RL, CONS_MSEQ and CONS_FIRST are the same on every rank, but the bases of a syncmer's first uncorrected
// occurrence lie in the reads of one rank only.  So once per consensus every rank writes the k-mers it holds into a table of all selected slots, zeros elsewhere
// (cons_str.hpp: cstr_kmer_kernel), and one all-reduce (sum, 64-bit: a row has one non-zero contributor, so nothing carries) leaves the whole table on every
// rank.  From then on the strings are a local matter: the same plan over the same tables gives the same bytes everywhere.

static int conskmer_buffer(oatk_hip_ctx *ctx, const void **d_ptr, uint64_t *bytes)
{
    ConsState *c = ctx->cons;
    if (!c || !c->done || !c->kmer_valid) { ctx->err = "CONS_KMER: after oatk_hip_consensus_strings_sharded, until the next consensus"; return OATK_E_STATE; }
    *d_ptr = c->kmer.p, *bytes = c->n_sel * c->kmer_stride;
    return OATK_OK;
}

// the k-mer table of the consensus at hand: one kernel, one collective
static int conskmer_make(oatk_hip_ctx *ctx, oatk_comm *c, ConsState *cs)
{
    using namespace oatk;
    const uint64_t stride = 8 * (((uint64_t) cs->K + 31) / 32), n_sel = cs->n_sel;
    if (!cs->kmer.ensure(n_sel * stride + 8, ctx->stream)) { ctx->err = "hipMalloc failed for cons.kmer"; return OATK_E_NOMEM; }
    cs->kmer_stride = stride, cs->kmer_ms = 0.f;
    if (n_sel) {
        CstrKmerArgs a;
        a.T = consstr_tables(ctx, cs), a.n_sel = n_sel, a.n_reads = ctx->n_reads, a.row_words = (uint32_t) (stride / 4), a.kmer = cs->kmer.as<uint32_t>();
        const bool timing = ctx->timing;
        if (timing) for (hipEvent_t &ev : cs->kmer_ev) if (!ev) CK(hipEventCreate(&ev));
        if (timing) CK(hipEventRecord(cs->kmer_ev[0], ctx->stream));
        hipLaunchKernelGGL(cstr_kmer_kernel, dim3((unsigned) ((n_sel + CSTR_WAVES - 1) / CSTR_WAVES)), dim3(64 * CSTR_WAVES), 0, ctx->stream, a);
        if (timing) CK(hipEventRecord(cs->kmer_ev[1], ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        CK(hipGetLastError());
        if (timing) CK(hipEventElapsedTime(&cs->kmer_ms, cs->kmer_ev[0], cs->kmer_ev[1]));
    }
    { int rc = comm_allreduce(ctx, c, cs->kmer.p, n_sel * (stride / 8), true, false); if (rc) return rc; }      // (n_sel is the same on every rank)
    cs->kmer_valid = true;
    return OATK_OK;
}

static int consensus_strings_sharded_impl(oatk_hip_ctx *ctx, oatk_comm *c, const oatk_cons_plan_t *plan, int hoco_seq, uint64_t *total_bytes, uint64_t *n_refused)
{
    int rc;
    if ((rc = comm_check(ctx, c, "oatk_hip_consensus_strings_sharded")) != OATK_OK) return rc;
    MultiState *m = ctx->multi;
    ConsState *cs = ctx->cons;
    if (!m || !m->ec_done) { ctx->err = "oatk_hip_consensus_strings_sharded: the reads of this handle are not sharded (oatk_hip_ec_sharded)"; return OATK_E_STATE; }
    if (!cs || !cs->done || (cs->n_scm == 0 && cs->n_sel != 0)) {                  // (oatk_hip_consensus_ids keeps no CONS_SLOT)
        ctx->err = "oatk_hip_consensus_strings_sharded: after oatk_hip_consensus_sharded";
        return OATK_E_STATE;
    }
    CK(hipSetDevice(ctx->device));
    // the one collective does not look at the plan: ranks that disagree about it, or of which some hold a bad one, still meet here
    if (!cs->kmer_valid && (rc = conskmer_make(ctx, c, cs)) != OATK_OK) return rc;
    const char *why = plan? consstr_plan_error(plan, cs->n_scm, cs->K) : "oatk_hip_consensus_strings_sharded: no plan";
    if (why) { ctx->err = why; c->agreed = true; return OATK_E_ARG; }              // (a local verdict with no collective behind it: nobody waits, the communicator lives)
    oatk_cstr::Tables T = consstr_tables(ctx, cs);
    T.kmer = cs->kmer.as<uint8_t>(), T.kmer_stride = cs->kmer_stride;
    rc = consstr_run(ctx, plan, hoco_seq, T, total_bytes, n_refused);
    if (rc != OATK_OK) c->agreed = true;                                           // (local as well)
    return rc;
}

extern "C" int oatk_hip_consensus_strings_sharded(oatk_hip_ctx *ctx, oatk_comm *c, const oatk_cons_plan_t *plan, int hoco_seq, uint64_t *total_bytes, uint64_t *n_refused)
{
    if (!ctx) return OATK_E_NODEV;
    if (!c) { ctx->err = "oatk_hip_consensus_strings_sharded: no communicator"; return OATK_E_ARG; }
    return comm_finish(c, consensus_strings_sharded_impl(ctx, c, plan, hoco_seq, total_bytes, n_refused));
}

extern "C" int oatk_hip_consensus_kmer_time(oatk_hip_ctx *ctx, float *ms, uint64_t *table_bytes)
{
    if (!ctx) return OATK_E_NODEV;
    ConsState *c = ctx->cons;
    if (!c || !c->done || !c->kmer_valid) { ctx->err = "oatk_hip_consensus_kmer_time: no k-mer table made yet"; return OATK_E_STATE; }
    if (ms) *ms = c->kmer_ms;
    if (table_bytes) *table_bytes = c->n_sel * c->kmer_stride;
    return OATK_OK;
}
