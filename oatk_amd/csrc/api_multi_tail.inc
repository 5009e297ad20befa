// oatk_amd/csrc/api_multi_tail.inc -- sharded reads up to the graph hand-off (include/oatk_hip_multi.h, second half); part of api.hip, after
// api_multi.inc.
//
// After oatk_hip_ec_sharded every rank holds the corrected chains of ITS reads in global ids and its hash range of the refreshed table.  What the
// host program does next (run_syncasm.c:131-303) consumes things that are properties of ALL reads: one syncmer_db_t with per-syncmer occurrence lists
// in (sid, idx) order (syncmer.c:1353-1360, syncerr.c:796-805), the assembly graph (syncasm.c:203-299), the consensus sums (:888-1003), the pair
// distance tables (:477-582) and the statistics (syncmer.c:867-1028).  Each gets a collective form here whose traffic does not grow with the number
// of ranks beyond what the result itself weighs:
//
//   oatk_hip_gather_table          the table on `root`: owners' ranges concatenated (hash, s-mer, coverage, del), every rank's occurrence words
//                                  with their global ids sent to root once and sorted there (stable: rank order is sid order)
//   oatk_hip_asm_graph_sharded     dense coverage / del from the owners (all-gather of 5 bytes per syncmer), every rank's adjacent pairs between
//                                  two KEPT vertices sorted and run-length encoded locally, the (key, count) lists all-gathered, the graph built
//                                  from the weighted keys on every rank (identical)
//   oatk_hip_consensus_sharded     per-rank run-length totals of the selected syncmers, one all-reduce (sum) of totals and counts, one (min) of
//                                  the first occurrences
//   oatk_hip_overlap_hist_sharded  pairs between kept vertices as weighted segments (key, distance, calls) in rank order = call order
//   oatk_hip_stat_sharded          s-mer / k-mer multiplicities by KEY RANGE: local (key, count) lists go to the range's owner, owners merge and
//                                  histogram, the 1001-bin histograms are all-reduced
#include <rocprim/device/device_reduce_by_key.hpp>

enum {
    MX_DCOV = 0, MX_DDEL, MX_T_GID, MX_T_OCC, MX_GKID, MX_R_GID, MX_R_OCC, MX_R_GID2, MX_R_OCC2, MX_G_H, MX_G_S, MX_G_COV, MX_G_DEL, MX_G_COV64, MX_G_OFF,
    MX_K1, MX_K2, MX_U, MX_C, MX_NR, MX_UA, MX_CA, MX_SEGK, MX_SEGV, MX_SKA, MX_SVA, MX_HEAD, MX_HPOS, MX_IOTA, MX_ZERO,
    MX_ST_SORT, MX_ST_U, MX_ST_C, MX_ST_NR, MX_ST_RU, MX_ST_RC, MX_ST_SU, MX_ST_SC, MX_ST_OU, MX_ST_OC, MX_ST_HIST, MX_ST_CALL, MX_COUNT_
};
static_assert(MX_COUNT_ <= 64, "MultiState::x is too small");

#define XENSURE(id, bytes) ENSURE_IN(m, "multi.", x[id], bytes)

// rank r's n_mine items of `width` bytes land on `root` back to back in rank order (dst is grown there); *n_all on every rank
static int comm_gather_root(oatk_hip_ctx *ctx, oatk_comm *c, const void *d_src, uint64_t n_mine, uint32_t width, DevBuf &dst, uint64_t *n_all, int root)
{
    uint64_t cnt[64], tot = 0, off = 0;
    { int rc = comm_allgather_u64(ctx, c, n_mine, cnt); if (rc) return rc; }
    for (int r = 0; r < c->n; ++r) tot += cnt[r];
    *n_all = tot;
    const bool me_root = c->rank == root;
    if (me_root && !dst.ensure(tot * width + 64, ctx->stream)) { ctx->err = "hipMalloc failed (gather to root)"; return OATK_E_NOMEM; }
    if (c->grp) {
        c->grp->ptr[c->rank] = d_src;
        CK(hipStreamSynchronize(ctx->stream));
        GWAIT(c);
        if (me_root) {
            for (int r = 0; r < c->n; off += cnt[r] * width, ++r)
                if (cnt[r]) CK(hipMemcpyAsync((uint8_t *) dst.p + off, c->grp->ptr[r], cnt[r] * width, hipMemcpyDeviceToDevice, ctx->stream));
            CK(hipStreamSynchronize(ctx->stream));
        }
        GWAIT(c);
        return OATK_OK;
    }
    if (me_root) {
        for (int r = 0; r < c->n; ++r) { if (r == root) break; off += cnt[r] * width; }
        if (n_mine) CK(hipMemcpyAsync((uint8_t *) dst.p + off, d_src, n_mine * width, hipMemcpyDeviceToDevice, ctx->stream));
        off = 0;
    }
    NCK(g_rccl.GroupStart());
    if (me_root) {
        for (int r = 0; r < c->n; off += cnt[r] * width, ++r)
            if (r != root && cnt[r]) NCK(g_rccl.Recv((uint8_t *) dst.p + off, cnt[r] * width, ncclUint8, r, c->nccl, ctx->stream));
    } else if (n_mine) NCK(g_rccl.Send(d_src, n_mine * width, ncclUint8, root, c->nccl, ctx->stream));
    NCK(g_rccl.GroupEnd());
    CK(hipStreamSynchronize(ctx->stream));
    return OATK_OK;
}

// the chains as counted, in global ids: per slot the id (for the occurrence lists), the occurrence word sid << 32 | idx << 1 | rev (the low 64 bits
// of the record the reference sorts, syncmer.c:1410) and sr_t.k_mer as collect_syncmer_from_reads leaves it (id << 1, :1378)
__global__ void mgt_slot_kernel(uint64_t n_reads, const uint64_t *scm_off, const uint64_t *kid, const uint32_t *m_pos, const uint32_t *l2g, uint64_t sid0,
                                uint32_t *gid, uint64_t *occ, uint64_t *gkid)
{
    const uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const uint64_t o = scm_off[r], n = scm_off[r + 1] - o;
    for (uint64_t j = 0; j < n; ++j) {
        const uint32_t g = l2g[kid[o + j] >> 1];
        gid[o + j] = g, gkid[o + j] = (uint64_t) g << 1;
        occ[o + j] = (sid0 + r) << 32 | j << 1 | (uint64_t) (m_pos[o + j] & 1u);
    }
}
__global__ void mgt_widen_kernel(const uint32_t *in, uint64_t *out, uint64_t n)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) out[i] = i < n? in[i] : 0;
}
// an adjacent pair counts for the graph only if both its ends are vertices (syncasm.c:226-233, :269-272); all != 0: every pair is kept
__global__ void mgt_pair_keep_kernel(uint64_t n, const uint64_t *keys, const uint32_t *cov, const uint8_t *del, uint32_t min_cov, uint64_t *out, int all)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = keys[i];
    if (all || k == EGR_INVALID) { out[i] = k; return; }
    const uint64_t a = (k >> 32) >> 1, b = (k & 0xFFFFFFFFULL) >> 1;
    out[i] = (del[a] | del[b]) || cov[a] < min_cov || cov[b] < min_cov? EGR_INVALID : k;
}
__global__ void mgt_seg_head_kernel(uint64_t n, const uint64_t *skeys, const uint32_t *sdist, uint8_t *head)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) head[i] = skeys[i] != EGR_INVALID && (i == 0 || skeys[i] != skeys[i - 1] || sdist[i] != sdist[i - 1]);
}
// where the fillers (sorted behind every pair) start: the last segment ends there (egr_seg_emit_kernel)
__global__ void mgt_first_invalid_kernel(const uint64_t *skeys, uint64_t n, uint64_t *out)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (skeys[mid] != EGR_INVALID) lo = mid + 1; else hi = mid; }
    *out = lo;
}
__global__ void mgt_cons_final_kernel(uint64_t n_sel, int K, const unsigned long long *tot, const uint32_t *m_seq, uint32_t *rl)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_sel * (uint64_t) K) return;
    const uint32_t mm = m_seq[i / (uint64_t) K];
    rl[i] = mm? (uint32_t) lround((double) tot[i] / (double) mm) : 0u;          // syncasm.c:994
}

// coverage and deletion marks of the whole refreshed table on every rank: the owners' ranges, all-gathered (5 bytes per syncmer)
static int mgt_dense(oatk_hip_ctx *ctx, oatk_comm *c, MultiState *m)
{
    uint64_t bytes[64];
    const uint64_t ng = m->n_global;
    XENSURE(MX_DCOV, (ng + 1) * 4); XENSURE(MX_DDEL, ng + 8);
    for (int r = 0; r < c->n; ++r) bytes[r] = (m->first_id[r + 1] - m->first_id[r]) * 4;
    { int rc = comm_allgatherv(ctx, c, m->ec_cov.p, bytes, m->x[MX_DCOV].p); if (rc) return rc; }
    for (int r = 0; r < c->n; ++r) bytes[r] = m->first_id[r + 1] - m->first_id[r];
    return comm_allgatherv(ctx, c, m->ec_del.p, bytes, m->x[MX_DDEL].p);
}

// ---------------------------------------------------------------- the table on one rank ----------------------------------------------------------------

static int gather_table_impl(oatk_hip_ctx *ctx, oatk_comm *c, int root)
{
    using namespace oatk;
    int rc;
    if ((rc = comm_check(ctx, c, "oatk_hip_gather_table")) != OATK_OK) return rc;
    if (root < 0 || root >= c->n) { ctx->err = "oatk_hip_gather_table: no such rank"; c->agreed = true; return OATK_E_ARG; }      // (the same argument on every rank: everybody refuses, nobody waits -- the communicator stays usable)
    MultiState *m = ctx->multi;
    if (!m || !m->merged) { ctx->err = "oatk_hip_gather_table needs oatk_hip_merge_counts"; return OATK_E_STATE; }
    CK(hipSetDevice(ctx->device));
    EcState *e = ctx->ec;
    const bool after = m->ec_done;
    const uint64_t ng = m->n_global, no = m->n_owned, nr = ctx->n_reads;
    const bool me_root = c->rank == root;
    m->table_root = -1;

    // 1. occurrences with their global ids.  After the correction update_syncmer_db's lists are resident, sorted by id (api_ec.inc); before it the
    //    counted chains are walked once, which also leaves every read's k_mer array as the reference's count leaves it
    const uint32_t *d_gid = nullptr;
    const uint64_t *d_occ = nullptr;
    uint64_t n_mine = 0, n_all = 0, chk = 0;
    if (after) {
        n_mine = e->new_tot, d_gid = e->key_sorted.as<uint32_t>(), d_occ = e->occ.as<uint64_t>();
    } else {
        n_mine = ctx->n_occ;
        XENSURE(MX_T_GID, (n_mine + 1) * 4); XENSURE(MX_T_OCC, (n_mine + 1) * 8); XENSURE(MX_GKID, (n_mine + 1) * 8);
        if (n_mine) hipLaunchKernelGGL(mgt_slot_kernel, grid256(nr), dim3(256), 0, ctx->stream, nr, ctx->scm_off.as<uint64_t>(), ctx->pos_kid.as<uint64_t>(), ctx->pos_mpos.as<uint32_t>(),
                                       m->l2g.as<uint32_t>(), ctx->sid0, m->x[MX_T_GID].as<uint32_t>(), m->x[MX_T_OCC].as<uint64_t>(), m->x[MX_GKID].as<uint64_t>());
        d_gid = m->x[MX_T_GID].as<uint32_t>(), d_occ = m->x[MX_T_OCC].as<uint64_t>();
        m->gkid_n = n_mine;
    }
    if ((rc = comm_gather_root(ctx, c, d_gid, n_mine, 4, m->x[MX_R_GID], &n_all, root)) != OATK_OK) return rc;
    if ((rc = comm_gather_root(ctx, c, d_occ, n_mine, 8, m->x[MX_R_OCC], &chk, root)) != OATK_OK) return rc;
    // 2. the owners' ranges in rank order are the table (the zero vector stands in for `del` before the correction)
    if (!after) { XENSURE(MX_ZERO, no + 8); CK(hipMemsetAsync(m->x[MX_ZERO].p, 0, no + 8, ctx->stream)); }
    if ((rc = comm_gather_root(ctx, c, m->own_h.p, no, 8, m->x[MX_G_H], &chk, root)) != OATK_OK) return rc;
    if ((rc = comm_gather_root(ctx, c, m->own_s.p, no, 8, m->x[MX_G_S], &chk, root)) != OATK_OK) return rc;
    if ((rc = comm_gather_root(ctx, c, after? m->ec_cov.p : m->own_cov.p, no, 4, m->x[MX_G_COV], &chk, root)) != OATK_OK) return rc;
    if ((rc = comm_gather_root(ctx, c, after? m->ec_del.p : m->x[MX_ZERO].p, no, 1, m->x[MX_G_DEL], &chk, root)) != OATK_OK) return rc;
    int bad = OATK_OK;
    if (me_root) {
        if (chk != ng) { ctx->err = "oatk_hip_gather_table: the ranges do not add up to the table"; bad = OATK_E_STATE; }
        // 3. lists per syncmer: one stable sort by id -- the ranks' parts arrive in rank order, which is sid order
        XENSURE(MX_R_GID2, (n_all + 1) * 4); XENSURE(MX_R_OCC2, (n_all + 1) * 8); XENSURE(MX_G_COV64, (ng + 2) * 8); XENSURE(MX_G_OFF, (ng + 2) * 8);
        if (!bad && n_all) {
            unsigned id_bits = 1;
            while (id_bits < 32 && (ng - 1) >> id_bits) ++id_bits;
            PRIM(rocprim::radix_sort_pairs, m->x[MX_R_GID].as<uint32_t>(), m->x[MX_R_GID2].as<uint32_t>(), m->x[MX_R_OCC].as<uint64_t>(), m->x[MX_R_OCC2].as<uint64_t>(), n_all, 0, id_bits,
                 ctx->stream);
        }
        if (!bad) {
            hipLaunchKernelGGL(mgt_widen_kernel, grid256(ng + 1), dim3(256), 0, ctx->stream, m->x[MX_G_COV].as<uint32_t>(), m->x[MX_G_COV64].as<uint64_t>(), ng);
            PRIM(rocprim::exclusive_scan, m->x[MX_G_COV64].as<uint64_t>(), m->x[MX_G_OFF].as<uint64_t>(), (uint64_t) 0, ng + 1, rocprim::plus<uint64_t>(), ctx->stream);
            uint64_t tot = 0;
            CK(hipMemcpyAsync(&tot, m->x[MX_G_OFF].as<uint64_t>() + ng, 8, hipMemcpyDeviceToHost, ctx->stream));
            CK(hipStreamSynchronize(ctx->stream));
            if (tot != n_all) { ctx->err = "oatk_hip_gather_table: coverage and occurrence lists disagree"; bad = OATK_E_STATE; }
        }
    }
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    if ((rc = comm_agree(ctx, c, bad, "oatk_hip_gather_table")) != OATK_OK) return rc;
    m->table_root = root, m->table_occ = n_all;
    return OATK_OK;
}

extern "C" int oatk_hip_gather_table(oatk_hip_ctx *ctx, oatk_comm *c, int root)
{
    if (!ctx) return OATK_E_NODEV;
    if (!c) { ctx->err = "oatk_hip_gather_table: no communicator"; return OATK_E_ARG; }
    return comm_finish(c, gather_table_impl(ctx, c, root));
}

static int multi_tail_buffer(oatk_hip_ctx *ctx, int which, const void **d_ptr, uint64_t *bytes)
{
    MultiState *m = ctx->multi;
    if (which == OATK_BUF_MG_POS_GKID) {
        if (!m || !m->merged || m->ec_done || !m->x[MX_GKID].p) { ctx->err = "MG_POS_GKID: after oatk_hip_gather_table, before the correction"; return OATK_E_STATE; }
        *d_ptr = m->x[MX_GKID].p, *bytes = m->gkid_n * 8;
        return OATK_OK;
    }
    if (!m || m->table_root != m->rank) { ctx->err = "the gathered table lives on the root rank of oatk_hip_gather_table"; return OATK_E_STATE; }
    const uint64_t ng = m->n_global;
    switch (which) {
        case OATK_BUF_MG_G_H: *d_ptr = m->x[MX_G_H].p, *bytes = ng * 8; break;
        case OATK_BUF_MG_G_S: *d_ptr = m->x[MX_G_S].p, *bytes = ng * 8; break;
        case OATK_BUF_MG_G_COV: *d_ptr = m->x[MX_G_COV].p, *bytes = ng * 4; break;
        case OATK_BUF_MG_G_DEL: *d_ptr = m->x[MX_G_DEL].p, *bytes = ng; break;
        case OATK_BUF_MG_G_OCC_OFF: *d_ptr = m->x[MX_G_OFF].p, *bytes = (ng + 1) * 8; break;
        case OATK_BUF_MG_G_OCC: *d_ptr = m->table_occ? m->x[MX_R_OCC2].p : nullptr, *bytes = m->table_occ * 8; break;
        default: ctx->err = "unknown buffer id"; return OATK_E_ARG;
    }
    return OATK_OK;
}

// ---------------------------------------------------------------- the assembly graph ----------------------------------------------------------------

static int asm_graph_sharded_impl(oatk_hip_ctx *ctx, oatk_comm *c, uint32_t min_k_cov, double min_a_cov_f, uint64_t *n_vtx, uint64_t *n_arc)
{
    using namespace oatk;
    int rc;
    if ((rc = comm_check(ctx, c, "oatk_hip_asm_graph_sharded")) != OATK_OK) return rc;
    MultiState *m = ctx->multi;
    if (!m || !m->ec_done) { ctx->err = "oatk_hip_asm_graph_sharded: after oatk_hip_ec_sharded"; return OATK_E_STATE; }
    CK(hipSetDevice(ctx->device));
    if ((rc = mgt_dense(ctx, c, m)) != OATK_OK) return rc;
    const uint32_t *d_cov = m->x[MX_DCOV].as<uint32_t>();
    const uint8_t *d_del = m->x[MX_DDEL].as<uint8_t>();
    // this rank's pairs between two vertices, sorted and counted
    const void *keys = nullptr;
    uint64_t n = 0, n_runs = 0;
    if ((rc = oatk_hip_asm_pairs(ctx, &keys, &n)) != OATK_OK) return rc;
    XENSURE(MX_K1, (n + 1) * 8); XENSURE(MX_K2, (n + 1) * 8); XENSURE(MX_U, (n + 1) * 8); XENSURE(MX_C, (n + 1) * 4); XENSURE(MX_NR, 64);
    if (n) {
        if (n >= 0xFFFFFFFFULL) { ctx->err = "more than 2^32 adjacent pairs on one rank"; return OATK_E_ARG; }
        hipLaunchKernelGGL(mgt_pair_keep_kernel, grid256(n), dim3(256), 0, ctx->stream, n, (const uint64_t *) keys, d_cov, d_del, min_k_cov, m->x[MX_K1].as<uint64_t>(), 0);
        if ((rc = prim_sort_runs(ctx, m->x[MX_K1].as<uint64_t>(), m->x[MX_K2].as<uint64_t>(), (void *) nullptr, (void *) nullptr, n, 0, 64, m->x[MX_U].as<uint64_t>(), m->x[MX_C].as<uint32_t>(),
                                 m->x[MX_NR].as<uint32_t>())) != OATK_OK) return rc;
        uint32_t nrn = 0;
        uint64_t last = 0;
        CK(hipMemcpyAsync(&nrn, m->x[MX_NR].p, 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        if (nrn) {
            CK(hipMemcpyAsync(&last, m->x[MX_U].as<uint64_t>() + (nrn - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
            CK(hipStreamSynchronize(ctx->stream));
        }
        n_runs = nrn && last == EGR_INVALID? nrn - 1 : nrn;            // the fillers sort behind every pair and stay at home
    }
    uint64_t n_all = 0, chk = 0;
    if ((rc = comm_gather_cols(ctx, c, {{m->x[MX_U].p, &m->x[MX_UA], 8}}, n_runs, &n_all)) != OATK_OK) return rc;
    if ((rc = comm_gather_cols(ctx, c, {{m->x[MX_C].p, &m->x[MX_CA], 4}}, n_runs, &chk)) != OATK_OK) return rc;
    // the same weighted keys on every rank: the same graph, the same verdict
    rc = ag_build(ctx, m->x[MX_UA].as<uint64_t>(), m->x[MX_CA].as<uint32_t>(), n_all, m->n_global, d_cov, d_del, min_k_cov, min_a_cov_f, n_vtx, n_arc);
    if (rc == OATK_E_SPLIT) c->agreed = true;
    return rc;
}

extern "C" int oatk_hip_asm_graph_sharded(oatk_hip_ctx *ctx, oatk_comm *c, uint32_t min_k_cov, double min_a_cov_f, uint64_t *n_vtx, uint64_t *n_arc)
{
    if (!ctx) return OATK_E_NODEV;
    if (!c) { ctx->err = "oatk_hip_asm_graph_sharded: no communicator"; return OATK_E_ARG; }
    return comm_finish(c, asm_graph_sharded_impl(ctx, c, min_k_cov, min_a_cov_f, n_vtx, n_arc));
}

// ---------------------------------------------------------------- consensus sums ----------------------------------------------------------------

static int cons_select(oatk_hip_ctx *ctx, ConsState *cs, uint64_t ns, const uint32_t *cov, const uint8_t *del, uint32_t min_cov, uint64_t *n_sel_out);

static int consensus_sharded_impl(oatk_hip_ctx *ctx, oatk_comm *c, uint32_t min_cov)
{
    using namespace oatk;
    int rc;
    if ((rc = comm_check(ctx, c, "oatk_hip_consensus_sharded")) != OATK_OK) return rc;
    MultiState *m = ctx->multi;
    if (!m || !m->ec_done) { ctx->err = "oatk_hip_consensus_sharded: after oatk_hip_ec_sharded"; return OATK_E_STATE; }
    CK(hipSetDevice(ctx->device));
    if ((rc = mgt_dense(ctx, c, m)) != OATK_OK) return rc;
    if (!ctx->cons) ctx->cons = new ConsState();
    ConsState *cs = ctx->cons;
    cs->done = false, cs->kmer_valid = false;
    const uint64_t ng = m->n_global;
    uint64_t n_sel = 0;
    cs->n_scm = ng, cs->K = ctx->K, cs->n_sel = 0;
    if (ng == 0) { cs->done = true; return OATK_OK; }
    if ((rc = cons_select(ctx, cs, ng, m->x[MX_DCOV].as<uint32_t>(), m->x[MX_DDEL].as<uint8_t>(), min_cov, &n_sel)) != OATK_OK) return rc;      // the same list on every rank
    if ((rc = cons_run(ctx, cs, n_sel)) != OATK_OK) return rc;
    CK(hipStreamSynchronize(ctx->stream));
    // totals and counts are sums over the shards; the first uncorrected occurrence is the smallest word (sid in the top bits; ~0 = none here)
    const uint64_t nk = n_sel * (uint64_t) ctx->K;
    if ((rc = comm_allreduce(ctx, c, cs->tot.p, nk, true, false)) != OATK_OK) return rc;
    if ((rc = comm_allreduce(ctx, c, cs->m_seq.p, n_sel, false, false)) != OATK_OK) return rc;
    if ((rc = comm_allreduce(ctx, c, cs->first.p, n_sel, true, true)) != OATK_OK) return rc;
    if (nk) hipLaunchKernelGGL(mgt_cons_final_kernel, dim3((unsigned) ((nk + 255) / 256)), dim3(256), 0, ctx->stream, n_sel, ctx->K, (const unsigned long long *) cs->tot.p,
                               cs->m_seq.as<uint32_t>(), cs->rl.as<uint32_t>());
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    cs->done = true;
    return OATK_OK;
}

extern "C" int oatk_hip_consensus_sharded(oatk_hip_ctx *ctx, oatk_comm *c, uint32_t min_cov)
{
    if (!ctx) return OATK_E_NODEV;
    if (!c) { ctx->err = "oatk_hip_consensus_sharded: no communicator"; return OATK_E_ARG; }
    return comm_finish(c, consensus_sharded_impl(ctx, c, min_cov));
}

// ---------------------------------------------------------------- pair-distance tables ----------------------------------------------------------------

static int overlap_hist_sharded_impl(oatk_hip_ctx *ctx, oatk_comm *c, uint32_t min_cov, uint64_t *n_pairs, uint64_t *n_entries)
{
    using namespace oatk;
    int rc;
    if ((rc = comm_check(ctx, c, "oatk_hip_overlap_hist_sharded")) != OATK_OK) return rc;
    MultiState *m = ctx->multi;
    if (!m || !m->ec_done) { ctx->err = "oatk_hip_overlap_hist_sharded: after oatk_hip_ec_sharded"; return OATK_E_STATE; }
    CK(hipSetDevice(ctx->device));
    if ((rc = mgt_dense(ctx, c, m)) != OATK_OK) return rc;
    const void *keys = nullptr, *dist = nullptr;
    uint64_t n = 0, n_seg = 0;
    if ((rc = oatk_hip_overlap_pairs(ctx, &keys, &dist, &n)) != OATK_OK) return rc;
    if (!ctx->ovl) ctx->ovl = new OvlState();
    OvlState *g = ctx->ovl;
    XENSURE(MX_K1, (n + 1) * 8); XENSURE(MX_HEAD, n + 8); XENSURE(MX_HPOS, (n + 1) * 4); XENSURE(MX_IOTA, (n + 1) * 4); XENSURE(MX_NR, 64);
    if (n) {
        if (n >= 0xFFFFFFFFULL) { ctx->err = "more than 2^32 adjacent pairs on one rank"; return OATK_E_ARG; }
        OENSURE(keys2, (n + 1) * 8); OENSURE(dist2, (n + 1) * 4);
        hipLaunchKernelGGL(mgt_pair_keep_kernel, grid256(n), dim3(256), 0, ctx->stream, n, (const uint64_t *) keys, m->x[MX_DCOV].as<uint32_t>(), m->x[MX_DDEL].as<uint8_t>(), min_cov,
                           m->x[MX_K1].as<uint64_t>(), min_cov == 0);
        // stable: a key's distances stay in (read, slot) order, so a segment is a run of consecutive calls
        PRIM(rocprim::radix_sort_pairs, m->x[MX_K1].as<uint64_t>(), g->keys2.as<uint64_t>(), (uint32_t *) const_cast<void *>(dist), g->dist2.as<uint32_t>(), n, 0, 64, ctx->stream);
        hipLaunchKernelGGL(mgt_seg_head_kernel, grid256(n), dim3(256), 0, ctx->stream, n, g->keys2.as<uint64_t>(), g->dist2.as<uint32_t>(), m->x[MX_HEAD].as<uint8_t>());
        hipLaunchKernelGGL(mg_iota_kernel, grid256(n), dim3(256), 0, ctx->stream, m->x[MX_IOTA].as<uint32_t>(), n);
        hipLaunchKernelGGL(mgt_first_invalid_kernel, dim3(1), dim3(1), 0, ctx->stream, g->keys2.as<uint64_t>(), n, m->x[MX_NR].as<uint64_t>() + 4);
        if ((rc = mg_select_u32(ctx, m, m->x[MX_IOTA].as<uint32_t>(), m->x[MX_HEAD].as<uint8_t>(), n, m->x[MX_HPOS], &n_seg)) != OATK_OK) return rc;
    }
    uint64_t n_valid = 0;
    if (n) { CK(hipMemcpyAsync(&n_valid, m->x[MX_NR].as<uint64_t>() + 4, 8, hipMemcpyDeviceToHost, ctx->stream)); CK(hipStreamSynchronize(ctx->stream)); }
    XENSURE(MX_SEGK, (n_seg + 1) * 8); XENSURE(MX_SEGV, (n_seg + 1) * 8);
    if (n_seg) hipLaunchKernelGGL(egr_seg_emit_kernel, grid256(n_seg), dim3(256), 0, ctx->stream, n_seg, n_valid, m->x[MX_HPOS].as<uint32_t>(), g->keys2.as<uint64_t>(), g->dist2.as<uint32_t>(),
                                  m->x[MX_SEGK].as<uint64_t>(), m->x[MX_SEGV].as<uint64_t>());
    uint64_t n_all = 0, chk = 0;
    if ((rc = comm_gather_cols(ctx, c, {{m->x[MX_SEGK].p, &m->x[MX_SKA], 8}}, n_seg, &n_all)) != OATK_OK) return rc;        // rank order = call order
    if ((rc = comm_gather_cols(ctx, c, {{m->x[MX_SEGV].p, &m->x[MX_SVA], 8}}, n_seg, &chk)) != OATK_OK) return rc;
    rc = ovl_build(ctx, m->x[MX_SKA].as<uint64_t>(), nullptr, m->x[MX_SVA].as<uint64_t>(), n_all, n_pairs, n_entries);
    if (rc == OATK_E_SPLIT) c->agreed = true;           // (identical input on every rank)
    return rc;
}

extern "C" int oatk_hip_overlap_hist_sharded(oatk_hip_ctx *ctx, oatk_comm *c, uint32_t min_cov, uint64_t *n_pairs, uint64_t *n_entries)
{
    if (!ctx) return OATK_E_NODEV;
    if (!c) { ctx->err = "oatk_hip_overlap_hist_sharded: no communicator"; return OATK_E_ARG; }
    return comm_finish(c, overlap_hist_sharded_impl(ctx, c, min_cov, n_pairs, n_entries));
}

// ---------------------------------------------------------------- statistics ----------------------------------------------------------------

// where the part of a sorted key list that rank r owns begins: owner(key) = floor(key * n / bound), so rank r starts at ceil(r * bound / n)
__global__ void mgs_bounds_kernel(const uint64_t *keys, uint64_t nk, int n, const uint64_t *split, uint64_t *off)
{
    const int r = threadIdx.x;
    if (r > n) return;
    if (r == n) { off[r] = nk; return; }
    uint64_t lo = 0, hi = nk;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (keys[mid] < split[r]) lo = mid + 1; else hi = mid; }
    off[r] = lo;
}

// multiplicities of one key list over all ranks: the histogram (kh_ctab_cnt, syncmer.c:648-667), the number of distinct keys and -- only when no key
// occurs exactly once -- the stale variable the reference reports then (api_stat.inc: StatKhl), which needs every distinct key's count in key order
static int stat_sharded_one(oatk_hip_ctx *ctx, oatk_comm *c, MultiState *m, const uint64_t *d_keys, uint64_t n, uint64_t bound, int64_t *hist_out, uint64_t *uniq_out,
                            int64_t *no_singleton)
{
    using namespace oatk;
    int rc;
    const int nrk = c->n;
    uint32_t n_runs = 0;
    XENSURE(MX_ST_SORT, (n + 1) * 8); XENSURE(MX_ST_U, (n + 1) * 8); XENSURE(MX_ST_C, (n + 1) * 4); XENSURE(MX_ST_NR, 1024 * 8); XENSURE(MX_ST_HIST, (OATK_STAT_MAX_DEPTH + 2) * 8);
    if (n) {
        if ((rc = prim_sort_runs(ctx, const_cast<uint64_t *>(d_keys), m->x[MX_ST_SORT].as<uint64_t>(), (void *) nullptr, (void *) nullptr, n, 0, 64, m->x[MX_ST_U].as<uint64_t>(),
                                 m->x[MX_ST_C].as<uint32_t>(), m->x[MX_ST_NR].as<uint32_t>())) != OATK_OK) return rc;
        CK(hipMemcpyAsync(&n_runs, m->x[MX_ST_NR].p, 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
    }
    // ranges of the key space: contiguous parts of the sorted distinct list go to their owners, whose parts in rank order are the global key order
    uint64_t split[65] = {0}, send_off[65] = {0}, recv_off[65] = {0};
    for (int r = 0; r < nrk; ++r) split[r] = (uint64_t) ((((unsigned __int128) (uint64_t) r * bound) + (uint64_t) (nrk - 1)) / (uint64_t) nrk);
    uint64_t *d_plan = m->x[MX_ST_NR].as<uint64_t>() + 8;
    CK(hipMemcpyAsync(d_plan, split, sizeof(split), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(mgs_bounds_kernel, dim3(1), dim3(128), 0, ctx->stream, m->x[MX_ST_U].as<uint64_t>(), (uint64_t) n_runs, nrk, d_plan, d_plan + 65);
    CK(hipMemcpyAsync(send_off, d_plan + 65, (size_t) (nrk + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    if ((rc = comm_plan(ctx, c, send_off, recv_off)) != OATK_OK) return rc;
    const uint64_t nrecv = recv_off[nrk];
    {   // (an owner's view: the verdict has to be everybody's)
        const int too_large = nrecv >= 0xFFFFFFFFULL? OATK_E_ARG : OATK_OK;
        if (too_large) ctx->err = "oatk_hip_stat_sharded: more than 2^32 distinct keys in one range";
        if ((rc = comm_agree(ctx, c, too_large, "oatk_hip_stat_sharded")) != OATK_OK) return rc;
    }
    XENSURE(MX_ST_RU, (nrecv + 1) * 8); XENSURE(MX_ST_RC, (nrecv + 1) * 4); XENSURE(MX_ST_SU, (nrecv + 1) * 8); XENSURE(MX_ST_SC, (nrecv + 1) * 4);
    XENSURE(MX_ST_OU, (nrecv + 1) * 8); XENSURE(MX_ST_OC, (nrecv + 1) * 4);
    if ((rc = comm_exchange_cols(ctx, c, {{m->x[MX_ST_U].p, m->x[MX_ST_RU].p, 8}}, send_off, recv_off)) != OATK_OK) return rc;
    if ((rc = comm_exchange_cols(ctx, c, {{m->x[MX_ST_C].p, m->x[MX_ST_RC].p, 4}}, send_off, recv_off)) != OATK_OK) return rc;
    uint32_t n_own = 0;
    CK(hipMemsetAsync(m->x[MX_ST_HIST].p, 0, (OATK_STAT_MAX_DEPTH + 2) * 8, ctx->stream));
    if (nrecv) {
        PRIM(rocprim::radix_sort_pairs, m->x[MX_ST_RU].as<uint64_t>(), m->x[MX_ST_SU].as<uint64_t>(), m->x[MX_ST_RC].as<uint32_t>(), m->x[MX_ST_SC].as<uint32_t>(), nrecv, 0, 64, ctx->stream);
        PRIM(rocprim::reduce_by_key, m->x[MX_ST_SU].as<uint64_t>(), m->x[MX_ST_SC].as<uint32_t>(), (unsigned int) nrecv, m->x[MX_ST_OU].as<uint64_t>(), m->x[MX_ST_OC].as<uint32_t>(),
             m->x[MX_ST_NR].as<uint32_t>() + 1, rocprim::plus<uint32_t>(), rocprim::equal_to<uint64_t>(), ctx->stream);
        CK(hipMemcpyAsync(&n_own, m->x[MX_ST_NR].as<uint32_t>() + 1, 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        unsigned nb = (n_own + 255) / 256;
        if (nb > 1024) nb = 1024;
        if (nb) hipLaunchKernelGGL(stat_hist_kernel, dim3(nb), dim3(256), 0, ctx->stream, n_own, m->x[MX_ST_OC].as<uint32_t>(), (unsigned long long *) m->x[MX_ST_HIST].p);
    }
    // [0 .. MAX_DEPTH] the histogram, [MAX_DEPTH + 1] the number of distinct keys
    CK(hipMemcpyAsync(m->x[MX_ST_HIST].as<uint64_t>() + (OATK_STAT_MAX_DEPTH + 1), &n_own, 4, hipMemcpyHostToDevice, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    if ((rc = comm_allreduce(ctx, c, m->x[MX_ST_HIST].p, OATK_STAT_MAX_DEPTH + 2, true, false)) != OATK_OK) return rc;
    uint64_t h[OATK_STAT_MAX_DEPTH + 2];
    CK(hipMemcpyAsync(h, m->x[MX_ST_HIST].p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i <= OATK_STAT_MAX_DEPTH; ++i) hist_out[i] = (int64_t) h[i];
    *uniq_out = h[OATK_STAT_MAX_DEPTH + 1];
    *no_singleton = 0;
    if (*uniq_out && hist_out[1] == 0) {                  // (the same test on every rank) replay the reference's count table over every distinct key
        uint64_t n_all = 0;
        if ((rc = comm_gather_cols(ctx, c, {{m->x[MX_ST_OC].p, &m->x[MX_ST_CALL], 4}}, n_own, &n_all)) != OATK_OK) return rc;
        std::vector<uint32_t> cc(n_all);
        if (n_all) CK(hipMemcpyAsync(cc.data(), m->x[MX_ST_CALL].p, (size_t) n_all * 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        StatKhl t;
        for (uint64_t i = 0; i < n_all; ++i) t.put1(cc[i]);
        *no_singleton = t.last_val();
    }
    return OATK_OK;
}

static int stat_sharded_impl(oatk_hip_ctx *ctx, oatk_comm *c, oatk_stat_raw_t *out)
{
    int rc;
    if ((rc = comm_check(ctx, c, "oatk_hip_stat_sharded")) != OATK_OK) return rc;
    if (!ctx->scanned) { ctx->err = "oatk_hip_stat_sharded needs a resident scan"; return OATK_E_STATE; }
    CK(hipSetDevice(ctx->device));
    if (!ctx->multi) ctx->multi = new MultiState();
    MultiState *m = ctx->multi;
    memset(out, 0, sizeof(*out));
    const void *s = nullptr, *k = nullptr;
    uint64_t n = 0;
    int64_t add4[4];
    if (ctx->counted && !(m->ec_done && ctx->ec && ctx->ec->done)) {
        ctx->err = "oatk_hip_stat_sharded: between the count and the correction a shard's k-mer keys are its own ids; call it after the scan or after oatk_hip_ec_sharded";
        return OATK_E_STATE;
    }
    if ((rc = oatk_hip_stat_keys(ctx, &s, &k, &n, add4)) != OATK_OK) return rc;
    XENSURE(MX_ST_NR, 1024 * 8);
    CK(hipMemcpyAsync(m->x[MX_ST_NR].as<uint64_t>() + 200, add4, 32, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = comm_allreduce(ctx, c, m->x[MX_ST_NR].as<uint64_t>() + 200, 4, true, false)) != OATK_OK) return rc;      // (two's complement: the signed sum too)
    CK(hipMemcpyAsync(add4, m->x[MX_ST_NR].as<uint64_t>() + 200, 32, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    out->n_reads = (uint64_t) add4[0], out->n_syncmers = (uint64_t) add4[1], out->sum_dist = add4[2], out->n_dist = (uint64_t) add4[3];
    if (out->n_syncmers == 0) return OATK_OK;             // (a global quantity: every rank returns here or none does)
    // the run-length encodings below count in 32 bits, like the graph and the distance tables of this file: a shard with more keys is refused -- by every rank
    if ((rc = comm_agree(ctx, c, n >= 0xFFFFFFFFULL? OATK_E_ARG : OATK_OK, "oatk_hip_stat_sharded (a shard with 2^32 syncmers or more)")) != OATK_OK) return rc;
    // s-mer codes are canonical s-mer << 1 | bit (below 2^63), k-mer keys are hash >> 1 before the count and global ids afterwards: either way below 2^63
    if ((rc = stat_sharded_one(ctx, c, m, (const uint64_t *) s, n, 1ULL << 63, out->smer_cnt, &out->smer_unique, &out->smer_no_singleton)) != OATK_OK) return rc;
    const bool ids = m->ec_done && ctx->ec && ctx->ec->done;
    return stat_sharded_one(ctx, c, m, (const uint64_t *) k, n, ids? (m->n_global? m->n_global : 1) : 1ULL << 63, out->kmer_cnt, &out->kmer_unique, &out->kmer_no_singleton);
}

extern "C" int oatk_hip_stat_sharded(oatk_hip_ctx *ctx, oatk_comm *c, oatk_stat_raw_t *out)
{
    if (!ctx) return OATK_E_NODEV;
    if (!c) { ctx->err = "oatk_hip_stat_sharded: no communicator"; return OATK_E_ARG; }
    return comm_finish(c, stat_sharded_impl(ctx, c, out));
}
