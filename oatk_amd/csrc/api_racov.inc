// oatk_amd/csrc/api_racov.inc -- C ABI of the coverage estimates from read alignments (include/oatk_hip_racov.h), for one handle and for reads sharded
// by record over several (the collectives of api_multi.inc); part of api.hip, after api_multi_tail.inc.
#include "../../include/oatk_hip_racov.h"
#include "racov.hpp"
#include <rocprim/device/device_segmented_radix_sort.hpp>

struct RcState {
    DevBuf su_off, su_uid, su_pos, scm_cov, utg_off, utg_a, utg_n, idx_p, idx_n, arc_v, arc_w, arc_link, arc_comp, arc_del;
    DevBuf a_sid, a_off, a_s, f_uid, f_ub, f_ue, f_sb, f_se, c_off, c_kmer;              // uploaded alignments and chains
    DevBuf flag, pos, rd_beg, need_c, need_l, need_u, cell_off, lcs_off, u_off, cells, lcs, rec_lb, rec_ln, st_frg, st_lcsb, st_uid, st_beg, st_len;
    DevBuf ma_n, ma_u, nb, cnt, vals, vals2, avg, covs, covt, key, val, key2, val2, seg_beg, seg_end, diff, err, tmp;
    DevBuf blk_a, em_w, em_e, em_fl, em_ef, em_fpos, ev_key, ev_key2, ev_val, ev_val2, ev_bits, ev_score, lv, arc_out;
    DevBuf carry;                                  // sharded: what the previous rank hands on (the EM's sums; the duplet table; the triplet table)
    DevBuf t_grp, t_pslot, t_score, t_have, t_first, t_last;        // the triplet scores (api_multiplex.inc): the groups of keys, every pair's slot, the results
    uint64_t cap_cells = 0;
};

static void rc_state_free(oatk_hip_ctx *ctx)
{
    delete ctx->rc;          // (its buffers free themselves: ~DevBuf)
    ctx->rc = nullptr;
}

#define RC_ENSURE(buf, bytes) ENSURE_IN(g, "racov.", buf, (uint64_t) (bytes) + 64)
#define RC_UPLOAD(buf, src, bytes)                                                                   \
    do {                                                                                           \
        RC_ENSURE(buf, bytes);                                                                       \
        if (bytes) CK(hipMemcpyAsync(g->buf.p, (src), (bytes), hipMemcpyHostToDevice, ctx->stream)); \
    } while (0)
// a rocPRIM call in this area's own temporary, which outlives the call that grew it like the rest of RcState
#define RC_PRIM(fn, ...) PRIM_IN(g->tmp, ctx->stream, "hipMalloc failed for racov.tmp", fn, __VA_ARGS__)
static inline unsigned rc_grid(uint64_t n) { return (unsigned) ((n + 255) / 256 > 0? (n + 255) / 256 : 1); }

// the unitigs' part of the graph, the alignments and (with_chains) the chains into a.  sharded: the handle's reads are one rank's share, and
// its resident chains are served in the global ids the sharded correction left them in
static int rc_bind(oatk_hip_ctx *ctx, RcState *g, const oatk_racov_graph_t *hg, const oatk_racov_reads_t *reads, const oatk_racov_aln_t *aln,
                   bool with_chains, bool sharded, oatk::RcArgs *a)
{
    if (!hg || !hg->su_off || !hg->utg_off) { ctx->err = "racov: no graph"; return OATK_E_ARG; }
    const uint64_t ns = hg->n_scm, nu = hg->n_utg, nsu = hg->su_off[ns], m_scm = hg->utg_off[nu];
    if (nu >= 0xFFFFFFFFull || m_scm >= 0xFFFFFFFFull) { ctx->err = "racov: the graph is too large (2^32 unitigs or syncmer positions)"; return OATK_E_ARG; }
    std::vector<uint32_t> un(nu + 1, 0);
    for (uint64_t i = 0; i < nu; ++i) {
        if (hg->utg_off[i + 1] < hg->utg_off[i] || hg->utg_off[i + 1] - hg->utg_off[i] >= (1ull << 31)) { ctx->err = "racov: bad unitig offsets"; return OATK_E_ARG; }
        un[i] = (uint32_t) (hg->utg_off[i + 1] - hg->utg_off[i]);
    }
    RC_UPLOAD(su_off, hg->su_off, (ns + 1) * 8); RC_UPLOAD(su_uid, hg->su_uid, nsu * 8); RC_UPLOAD(su_pos, hg->su_pos, nsu * 4);
    RC_UPLOAD(utg_off, hg->utg_off, (nu + 1) * 8); RC_UPLOAD(utg_a, hg->utg_a, m_scm * 8); RC_UPLOAD(utg_n, un.data(), (nu + 1) * 4);
    if (hg->scm_cov) RC_UPLOAD(scm_cov, hg->scm_cov, ns * 4);
    memset(a, 0, sizeof(*a));
    a->n_scm = ns, a->n_utg = nu;
    a->su_off = g->su_off.as<uint64_t>(), a->su_uid = g->su_uid.as<uint64_t>(), a->su_pos = g->su_pos.as<uint32_t>(), a->scm_cov = g->scm_cov.as<uint32_t>();
    a->utg_off = g->utg_off.as<uint64_t>(), a->utg_a = g->utg_a.as<uint64_t>(), a->utg_n = g->utg_n.as<uint32_t>();
    if (aln) {
        const uint64_t na = aln->n_aln, nf = aln->n_frg;
        if (na && aln->off[na] != nf) { ctx->err = "racov: alignment offsets do not end at n_frg"; return OATK_E_ARG; }
        RC_UPLOAD(a_sid, aln->sid, na * 4); RC_UPLOAD(a_off, aln->off, (na + 1) * 8); RC_UPLOAD(a_s, aln->s, na * 8);
        RC_UPLOAD(f_uid, aln->uid, nf * 8); RC_UPLOAD(f_ub, aln->u_beg, nf * 4); RC_UPLOAD(f_ue, aln->u_end, nf * 4); RC_UPLOAD(f_sb, aln->s_beg, nf * 4); RC_UPLOAD(f_se, aln->s_end, nf * 4);
        a->n_aln = na, a->sid = g->a_sid.as<uint32_t>(), a->off = g->a_off.as<uint64_t>(), a->s = g->a_s.as<double>();
        a->uid = g->f_uid.as<uint64_t>(), a->ubeg = g->f_ub.as<uint32_t>(), a->uend = g->f_ue.as<uint32_t>(), a->sbeg = g->f_sb.as<uint32_t>(), a->send = g->f_se.as<uint32_t>();
    } else {
        RaState *r = ctx->ra;
        if (!r || !r->done) { ctx->err = "racov: resident alignments requested before oatk_hip_read_alignment"; return OATK_E_STATE; }
        a->n_aln = r->n_aln, a->sid = r->o_sid.as<uint32_t>(), a->off = r->o_off.as<uint64_t>(), a->s = r->o_s.as<double>();
        a->uid = r->o_uid.as<uint64_t>(), a->ubeg = r->o_ubeg.as<uint32_t>(), a->uend = r->o_uend.as<uint32_t>(), a->sbeg = r->o_sbeg.as<uint32_t>(), a->send = r->o_send.as<uint32_t>();
    }
    if (!with_chains) return OATK_OK;
    if (reads) {
        const uint64_t nr = reads->n_reads, nk = reads->off[nr];
        RC_UPLOAD(c_off, reads->off, (nr + 1) * 8); RC_UPLOAD(c_kmer, reads->k_mer, nk * 8);
        a->n_reads = nr, a->chain_off = g->c_off.as<uint64_t>(), a->k_mer = g->c_kmer.as<uint64_t>();
    } else {
        if (!ctx->counted) { ctx->err = "racov: resident chains requested without a resident scan + count"; return OATK_E_STATE; }
        EcState *e = ctx->ec;
        if (e && e->global && !sharded) { ctx->err = "racov: the resident chains of a sharded batch are not served (one handle only)"; return OATK_E_STATE; }
        if (e && e->global && !e->done) { ctx->err = "racov: the resident chains of a sharded batch are in global ids only after oatk_hip_ec_sharded"; return OATK_E_STATE; }
        const bool after_ec = e && e->done;
        a->n_reads = ctx->n_reads;
        a->chain_off = after_ec? e->new_off.as<uint64_t>() : ctx->scm_off.as<uint64_t>();
        a->k_mer = after_ec? e->new_k.as<uint64_t>() : ctx->pos_kid.as<uint64_t>();
    }
    return OATK_OK;
}

static int rc_err(oatk_hip_ctx *ctx, RcState *g)
{
    unsigned int e = 0;
    CK(hipMemcpyAsync(&e, g->err.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    if (e & oatk::RC_ERR_ARC) { ctx->err = "racov: two consecutive fragments of an alignment have no arc between them"; return OATK_E_ARG; }
    if (e & oatk::RC_ERR_FRG) { ctx->err = "racov: an alignment does not fit the graph or the reads"; return OATK_E_ARG; }
    if (e & oatk::RC_ERR_ROOM) { ctx->err = "racov: make_ma_block outgrew its room (internal)"; return OATK_E_STATE; }
    return OATK_OK;
}

// every unitig's values sorted ascending (qsort with dbl_cmpfunc: the values are >= 0, no NaN from sound input), then its IQR mean
static int rc_iqr(oatk_hip_ctx *ctx, RcState *g, const oatk::RcArgs &a, uint64_t m_scm, int drop_zero)
{
    if (m_scm) {
        RC_PRIM(rocprim::segmented_radix_sort_keys, g->vals.as<double>(), g->vals2.as<double>(), (unsigned) m_scm, (unsigned) a.n_utg,
                a.utg_off, a.utg_off + 1, 0, 64, ctx->stream);
    }
    hipLaunchKernelGGL(oatk::rc_iqr_kernel, dim3(rc_grid(a.n_utg)), dim3(256), 0, ctx->stream, a.n_utg, a.utg_off, g->vals2.as<double>(), drop_zero, g->avg.as<double>());
    return OATK_OK;
}

static RcState *rc_state(oatk_hip_ctx *ctx)
{
    if (!ctx->rc) ctx->rc = new RcState();
    return ctx->rc;
}

extern "C" int oatk_hip_debug_racov_cap(oatk_hip_ctx *ctx, uint64_t cells)
{
    if (!ctx) return OATK_E_NODEV;
    rc_state(ctx)->cap_cells = cells;
    return OATK_OK;
}

// ---- reads sharded by record (oatk_hip_ra_*_coverage_sharded): `c` below is the communicator, NULL for the one-handle calls ----
// every rank's verdict on a step all of them took (comm_agree); one handle: its own
static int rc_verdict(oatk_hip_ctx *ctx, oatk_comm *c, int rc, const char *who) { return c? comm_agree(ctx, c, rc, who) : rc; }
// `bytes` at d_src of rank `root` into d_dst of every rank: an all-gather to which only root contributes
static int rc_bcast(oatk_hip_ctx *ctx, oatk_comm *c, int root, const void *d_src, void *d_dst, uint64_t bytes)
{
    uint64_t b[64] = {0};
    b[root] = bytes;
    return comm_allgatherv(ctx, c, d_src, b, d_dst);
}

static int rc_utg_impl(oatk_hip_ctx *ctx, oatk_comm *c, const oatk_racov_graph_t *hg, const oatk_racov_reads_t *reads, const oatk_racov_aln_t *aln,
                       int verbose, double *utg_cov, uint64_t *n_iter)
{
    using namespace oatk;
    const char *who = c? "oatk_hip_ra_utg_coverage_sharded" : "oatk_hip_ra_utg_coverage";
    if (c) { int rc = comm_check(ctx, c, who); if (rc) return rc; }
    if (!utg_cov) { ctx->err = std::string(who) + ": no output"; return OATK_E_ARG; }
    CK(hipSetDevice(ctx->device));
    if (c && !ctx->multi) ctx->multi = new MultiState();                         // (the collectives' scratch)
    RcState *g = rc_state(ctx);
    RcArgs a;
    { int rc = rc_bind(ctx, g, hg, reads, aln, true, c != nullptr, &a); if (rc) return rc; }
    if (!hg->scm_cov) { ctx->err = std::string(who) + ": no syncmer coverage"; return OATK_E_ARG; }
    if (n_iter) *n_iter = 0;
    const uint64_t na = a.n_aln, nu = a.n_utg, m_scm = hg->utg_off[nu];
    if (c) {                                                                     // a rank without alignments still takes part
        uint64_t cnt[64], tot = 0;
        { int rc = comm_allgather_u64(ctx, c, na, cnt); if (rc) return rc; }
        for (int r = 0; r < c->n; ++r) tot += cnt[r];
        if (tot == 0) return OATK_OK;
    } else if (na == 0) return OATK_OK;                                          // :1884-1887, the caller prints the warning
    RC_ENSURE(err, 4);
    CK(hipMemsetAsync(g->err.p, 0, 4, ctx->stream));
    a.err = g->err.as<unsigned int>();
    RC_ENSURE(avg, nu * 8); RC_ENSURE(covs, nu * 8); RC_ENSURE(vals, m_scm * 8); RC_ENSURE(vals2, m_scm * 8);
    if (c) RC_ENSURE(carry, nu * 8);
    // first round (:1921-1952): the counts are integers, their sum over the ranks is exact; everything after it is the same code on the same numbers
    RC_ENSURE(cnt, m_scm * 4);
    CK(hipMemsetAsync(g->cnt.p, 0, m_scm * 4 + 4, ctx->stream));
    hipLaunchKernelGGL(rc_r1_count_kernel, dim3(rc_grid(na) < 4096? rc_grid(na) : 4096), dim3(256), 0, ctx->stream, a, g->cnt.as<unsigned int>());
    if (c) { int rc = comm_allreduce(ctx, c, g->cnt.p, m_scm, false, false); if (rc) return rc; }
    if (m_scm) hipLaunchKernelGGL(rc_u2d_kernel, dim3(rc_grid(m_scm)), dim3(256), 0, ctx->stream, g->cnt.as<unsigned int>(), g->vals.as<double>(), m_scm);
    { int rc = rc_iqr(ctx, g, a, m_scm, 1); if (rc) return rc; }
    // reads: runs of one sid
    RC_ENSURE(flag, (na + 1) * 8); RC_ENSURE(pos, (na + 1) * 8);
    CK(hipMemsetAsync(g->flag.p, 0, (na + 1) * 8, ctx->stream));
    hipLaunchKernelGGL(rc_head_kernel, dim3(rc_grid(na)), dim3(256), 0, ctx->stream, a, g->flag.as<uint64_t>());
    uint64_t nr = 0;
    { int rc = prim_scan_total(ctx, g->tmp, g->flag.as<uint64_t>(), g->pos.as<uint64_t>(), na, &nr); if (rc) return rc; }
    a.n_rd = nr;
    RC_ENSURE(rd_beg, (nr + 1) * 8);
    hipLaunchKernelGGL(rc_runs_kernel, dim3(rc_grid(na + 1)), dim3(256), 0, ctx->stream, a, g->flag.as<uint64_t>(), g->pos.as<uint64_t>(), g->rd_beg.as<uint64_t>());
    a.rd_beg = g->rd_beg.as<uint64_t>();
    // make_ma_block's room: sizes per read, scanned.  `bad` is this rank's verdict on its own reads: with a communicator the ranks agree on it
    // before anything is written, so a refusal is everybody's
    RC_ENSURE(need_c, (nr + 1) * 8); RC_ENSURE(need_l, (nr + 1) * 8); RC_ENSURE(need_u, (nr + 1) * 8);
    RC_ENSURE(cell_off, (nr + 1) * 8); RC_ENSURE(lcs_off, (nr + 1) * 8); RC_ENSURE(u_off, (nr + 1) * 8);
    CK(hipMemsetAsync(g->need_c.p, 0, (nr + 1) * 8, ctx->stream)); CK(hipMemsetAsync(g->need_l.p, 0, (nr + 1) * 8, ctx->stream)); CK(hipMemsetAsync(g->need_u.p, 0, (nr + 1) * 8, ctx->stream));
    hipLaunchKernelGGL(rc_ma_size_kernel, dim3(rc_grid(nr)), dim3(256), 0, ctx->stream, a, g->need_c.as<uint64_t>(), g->need_l.as<uint64_t>(), g->need_u.as<uint64_t>());
    int bad = rc_err(ctx, g);
    uint64_t tot_c = 0, tot_l = 0, tot_u = 0;
    if (!bad) {
        { int rc = prim_scan_total(ctx, g->tmp, g->need_c.as<uint64_t>(), g->cell_off.as<uint64_t>(), nr, &tot_c); if (rc) return rc; }
        { int rc = prim_scan_total(ctx, g->tmp, g->need_l.as<uint64_t>(), g->lcs_off.as<uint64_t>(), nr, &tot_l); if (rc) return rc; }
        { int rc = prim_scan_total(ctx, g->tmp, g->need_u.as<uint64_t>(), g->u_off.as<uint64_t>(), nr, &tot_u); if (rc) return rc; }
        const uint64_t cap = g->cap_cells? g->cap_cells : (1ull << 31);
        if (tot_c > cap) {
            char m[192];
            snprintf(m, sizeof(m), "%s: the LCS matrices take %llu cells, over the limit of %llu", who, (unsigned long long) tot_c, (unsigned long long) cap);
            ctx->err = m;
            bad = OATK_E_SPLIT;
        } else if (tot_l >= 0xFFFFFFFFull || tot_u >= 0xFFFFFFFFull) { ctx->err = std::string(who) + ": more than 2^32 blocks"; bad = OATK_E_SPLIT; }
    }
    if (!bad) {
        RC_ENSURE(cells, tot_c * 4); RC_ENSURE(lcs, tot_l * 8); RC_ENSURE(rec_lb, na * 4); RC_ENSURE(rec_ln, na * 4); RC_ENSURE(st_frg, na * 4); RC_ENSURE(st_lcsb, na * 4);
        RC_ENSURE(st_uid, na * 4); RC_ENSURE(st_beg, na * 8); RC_ENSURE(st_len, na * 8); RC_ENSURE(ma_n, tot_l * 4); RC_ENSURE(ma_u, tot_u * 4); RC_ENSURE(nb, nr * 4);
        a.cell_off = g->cell_off.as<uint64_t>(), a.lcs_off = g->lcs_off.as<uint64_t>(), a.blk_off = g->lcs_off.as<uint64_t>(), a.u_off = g->u_off.as<uint64_t>();
        a.cells = g->cells.as<int32_t>(), a.lcs = g->lcs.as<uint64_t>(), a.rec_lb = g->rec_lb.as<uint32_t>(), a.rec_ln = g->rec_ln.as<uint32_t>();
        a.st_frg = g->st_frg.as<uint32_t>(), a.st_lcsb = g->st_lcsb.as<uint32_t>(), a.st_uid = g->st_uid.as<uint32_t>(), a.st_beg = g->st_beg.as<uint64_t>(), a.st_len = g->st_len.as<uint64_t>();
        a.ma_n = g->ma_n.as<uint32_t>(), a.ma_u = g->ma_u.as<uint32_t>(), a.nb = g->nb.as<uint32_t>();
        hipLaunchKernelGGL(rc_ma_kernel, dim3(rc_grid(nr)), dim3(256), 0, ctx->stream, a);
        bad = rc_err(ctx, g);
    }
    { int rc = rc_verdict(ctx, c, bad, who); if (rc) return rc; }
    // the contributions, by unitig in the reference's order
    RC_ENSURE(key, tot_u * 4); RC_ENSURE(val, tot_u * 4); RC_ENSURE(key2, tot_u * 4); RC_ENSURE(val2, tot_u * 4); RC_ENSURE(seg_beg, nu * 8); RC_ENSURE(seg_end, nu * 8); RC_ENSURE(covt, tot_l * 8);
    CK(hipMemsetAsync(g->key.p, 0xFF, tot_u * 4, ctx->stream));
    CK(hipMemsetAsync(g->seg_beg.p, 0, nu * 8, ctx->stream)); CK(hipMemsetAsync(g->seg_end.p, 0, nu * 8, ctx->stream));
    RC_ENSURE(blk_a, tot_l * 4);
    hipLaunchKernelGGL(rc_contrib_kernel, dim3(rc_grid(nr)), dim3(256), 0, ctx->stream, a, g->key.as<uint32_t>(), g->val.as<uint32_t>(), g->blk_a.as<uint32_t>());
    if (tot_u) {
        RC_PRIM(rocprim::radix_sort_pairs, g->key.as<uint32_t>(), g->key2.as<uint32_t>(), g->val.as<uint32_t>(), g->val2.as<uint32_t>(),
                tot_u, 0, 32, ctx->stream);
        hipLaunchKernelGGL(rc_segments_kernel, dim3(rc_grid(tot_u)), dim3(256), 0, ctx->stream, tot_u, nu, g->key2.as<uint32_t>(), g->seg_beg.as<uint64_t>(), g->seg_end.as<uint64_t>());
    }
    // the integral addends' prefix sums and the places of the fractional ones (rc_em_kernel)
    RC_ENSURE(em_w, (tot_u + 1) * 8); RC_ENSURE(em_e, (tot_u + 1) * 8); RC_ENSURE(em_fl, (tot_u + 1) * 8); RC_ENSURE(em_ef, (tot_u + 1) * 8);
    CK(hipMemsetAsync(g->em_w.p, 0, (tot_u + 1) * 8, ctx->stream)); CK(hipMemsetAsync(g->em_fl.p, 0, (tot_u + 1) * 8, ctx->stream));
    if (tot_u) hipLaunchKernelGGL(rc_em_prep_kernel, dim3(rc_grid(tot_u)), dim3(256), 0, ctx->stream, tot_u, nu, g->key2.as<uint32_t>(), g->val2.as<uint32_t>(),
                                  g->blk_a.as<uint32_t>(), g->ma_n.as<uint32_t>(), g->em_w.as<uint64_t>(), g->em_fl.as<uint64_t>());
    uint64_t tot_w = 0, n_frac = 0;
    { int rc = prim_scan_total(ctx, g->tmp, g->em_w.as<uint64_t>(), g->em_e.as<uint64_t>(), tot_u, &tot_w); if (rc) return rc; }
    { int rc = prim_scan_total(ctx, g->tmp, g->em_fl.as<uint64_t>(), g->em_ef.as<uint64_t>(), tot_u, &n_frac); if (rc) return rc; }
    RC_ENSURE(em_fpos, (n_frac + 1) * 8);
    if (tot_u) hipLaunchKernelGGL(rc_fpos_kernel, dim3(rc_grid(tot_u)), dim3(256), 0, ctx->stream, tot_u, g->em_fl.as<uint64_t>(), g->em_ef.as<uint64_t>(), g->em_fpos.as<uint64_t>());
    // the EM (:1983-2011).  Sharded: the ranks' contributions are consecutive stretches of the reference's (read, block, member) order, so
    // rank r's sums go on from rank r - 1's (the carry) and the last rank's are everybody's; the update and diff are then the same code on
    // the same numbers, and every rank leaves the loop at the same iteration
    RC_ENSURE(diff, 8);
    const bool talk = verbose > 2 && (!c || c->rank == 0);
    const double *d_sums = c? g->carry.as<double>() : g->covs.as<double>();
    uint64_t it;
    for (it = 0; it < 1000; ++it) {                                               // EM_MAX_ITER
        hipLaunchKernelGGL(rc_covt_kernel, dim3(rc_grid(nr)), dim3(256), 0, ctx->stream, a, g->avg.as<double>(), g->covt.as<double>());
        for (int r = 0; r < (c? c->n : 1); ++r) {
            if (!c || c->rank == r)
                hipLaunchKernelGGL(rc_em_kernel, dim3(rc_grid(nu)), dim3(256), 0, ctx->stream, nu, g->seg_beg.as<uint64_t>(), g->seg_end.as<uint64_t>(), g->val2.as<uint32_t>(),
                                   g->covt.as<double>(), g->ma_n.as<uint32_t>(), g->avg.as<double>(), g->em_e.as<uint64_t>(), g->em_ef.as<uint64_t>(),
                                   g->em_fpos.as<uint64_t>(), r? g->carry.as<double>() : nullptr, g->covs.as<double>());
            if (c) { int rc = rc_bcast(ctx, c, r, g->covs.p, g->carry.p, nu * 8); if (rc) return rc; }
        }
        hipLaunchKernelGGL(rc_diff_kernel, dim3(1), dim3(256), 0, ctx->stream, nu, g->utg_n.as<uint32_t>(), d_sums, g->avg.as<double>(), g->diff.as<double>());
        double diff = 0.;
        CK(hipMemcpyAsync(&diff, g->diff.p, 8, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        if (talk) fprintf(stderr, "[M::%s] unitig coverage estimation iteration %lu: diff = %.6f\n", "scg_ra_utg_coverage", (unsigned long) it, diff);
        if (diff < DBL_EPSILON) break;
    }
    if (talk) fprintf(stderr, "[M::%s] unitig coverage estimation ended at iteration %lu\n", "scg_ra_utg_coverage", (unsigned long) it);
    // third round (:2020-2044): the graph and avg only, the same on every rank
    if (m_scm) CK(hipMemsetAsync(g->vals.p, 0, m_scm * 8, ctx->stream));
    hipLaunchKernelGGL(rc_r3_kernel, dim3(rc_grid(a.n_scm)), dim3(256), 0, ctx->stream, a, g->avg.as<double>(), g->vals.as<double>());
    { int rc = rc_iqr(ctx, g, a, m_scm, 0); if (rc) return rc; }
    { int rc = rc_verdict(ctx, c, rc_err(ctx, g), who); if (rc) return rc; }
    if (nu) CK(hipMemcpyAsync(utg_cov, g->avg.p, nu * 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    if (n_iter) *n_iter = it;
    return OATK_OK;
}

static int rc_arc_impl(oatk_hip_ctx *ctx, oatk_comm *c, const oatk_racov_graph_t *hg, const oatk_racov_aln_t *aln, double *arc_cov)
{
    using namespace oatk;
    const char *who = c? "oatk_hip_ra_arc_coverage_sharded" : "oatk_hip_ra_arc_coverage";
    if (c) { int rc = comm_check(ctx, c, who); if (rc) return rc; }
    if (!arc_cov) { ctx->err = std::string(who) + ": no output"; return OATK_E_ARG; }
    CK(hipSetDevice(ctx->device));
    if (c && !ctx->multi) ctx->multi = new MultiState();
    RcState *g = rc_state(ctx);
    RcArgs a;
    { int rc = rc_bind(ctx, g, hg, nullptr, aln, false, c != nullptr, &a); if (rc) return rc; }
    const uint64_t nu = hg->n_utg, n_arc = hg->n_arc;
    if (n_arc && (!hg->idx_p || !hg->arc_v || !hg->arc_w || !hg->arc_link || !hg->arc_comp || !hg->arc_del)) { ctx->err = std::string(who) + ": no arcs"; return OATK_E_ARG; }
    uint64_t n_link = 0;
    for (uint64_t i = 0; i < n_arc; ++i) if (hg->arc_link[i] + 1 > n_link) n_link = hg->arc_link[i] + 1;
    if (n_link >= (1ull << 40)) { ctx->err = std::string(who) + ": link ids beyond 2^40"; return OATK_E_ARG; }
    RC_UPLOAD(idx_p, hg->idx_p, 2 * nu * 8); RC_UPLOAD(idx_n, hg->idx_n, 2 * nu * 8);
    RC_UPLOAD(arc_v, hg->arc_v, n_arc * 8); RC_UPLOAD(arc_w, hg->arc_w, n_arc * 8); RC_UPLOAD(arc_link, hg->arc_link, n_arc * 8);
    RC_UPLOAD(arc_comp, hg->arc_comp, n_arc); RC_UPLOAD(arc_del, hg->arc_del, n_arc);
    RcArcArgs q;
    q.idx_p = g->idx_p.as<uint64_t>(), q.idx_n = g->idx_n.as<uint64_t>(), q.arc_v = g->arc_v.as<uint64_t>(), q.arc_w = g->arc_w.as<uint64_t>();
    q.arc_link = g->arc_link.as<uint64_t>(), q.arc_comp = g->arc_comp.as<uint8_t>(), q.arc_del = g->arc_del.as<uint8_t>(), q.n_arc = n_arc, q.n_link = n_link;
    RC_ENSURE(err, 4);
    CK(hipMemsetAsync(g->err.p, 0, 4, ctx->stream));
    a.err = g->err.as<unsigned int>();
    const uint64_t na = a.n_aln;
    uint64_t nf = 0;
    if (na) {
        CK(hipMemcpyAsync(&nf, a.off + na, 8, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
    }
    // the duplet table: per link both keys' values (2 n_link doubles), then which were put (2 n_link bytes) -- one stretch of memory, so that
    // it travels as one piece
    const uint64_t tab = 2 * n_link * 8 + 2 * n_link;
    RC_ENSURE(lv, tab + 16);
    if (c) RC_ENSURE(carry, tab + 16);
    CK(hipMemsetAsync(g->lv.p, 0, tab + 16, ctx->stream));
    int bad = OATK_OK;
    if (nf) {
        RC_ENSURE(ev_key, nf * 8); RC_ENSURE(ev_key2, nf * 8); RC_ENSURE(ev_val, nf * 4); RC_ENSURE(ev_val2, nf * 4); RC_ENSURE(ev_bits, nf); RC_ENSURE(ev_score, nf * 8);
        CK(hipMemsetAsync(g->ev_key.p, 0xFF, nf * 8, ctx->stream));
        CK(hipMemsetAsync(g->ev_val.p, 0, nf * 4, ctx->stream));
        hipLaunchKernelGGL(rc_duplet_kernel, dim3(rc_grid(na) < 4096? rc_grid(na) : 4096), dim3(256), 0, ctx->stream, a, q, g->ev_key.as<uint64_t>(), g->ev_val.as<uint32_t>(),
                           g->ev_bits.as<uint8_t>(), g->ev_score.as<double>());
        bad = rc_err(ctx, g);
        if (!bad) {
            RC_PRIM(rocprim::radix_sort_pairs, g->ev_key.as<uint64_t>(), g->ev_key2.as<uint64_t>(), g->ev_val.as<uint32_t>(),
                    g->ev_val2.as<uint32_t>(), nf, 0, 64, ctx->stream);
        }
    }
    { int rc = rc_verdict(ctx, c, bad, who); if (rc) return rc; }               // a missing arc on any rank is everybody's refusal
    // A rank's events sorted stably by link are a stretch of the reference's put order for that link: rank r replays its own on top of the
    // table as rank r - 1 left it, and the last rank's table is everybody's
    for (int r = 0; r < (c? c->n : 1); ++r) {
        if (!c || c->rank == r) {
            if (r && tab) CK(hipMemcpyAsync(g->lv.p, g->carry.p, tab, hipMemcpyDeviceToDevice, ctx->stream));
            if (nf) hipLaunchKernelGGL(rc_link_kernel, dim3(rc_grid(nf)), dim3(256), 0, ctx->stream, nf, n_link, g->ev_key2.as<uint64_t>(), g->ev_val2.as<uint32_t>(),
                                       g->ev_bits.as<uint8_t>(), g->ev_score.as<double>(), g->lv.as<double>(), g->lv.as<uint8_t>() + 2 * n_link * 8);
        }
        if (c) { int rc = rc_bcast(ctx, c, r, g->lv.p, g->carry.p, tab); if (rc) return rc; }
    }
    const uint8_t *d_tab = c? g->carry.as<uint8_t>() : g->lv.as<uint8_t>();
    RC_ENSURE(arc_out, n_arc * 8);
    if (n_arc) hipLaunchKernelGGL(rc_arc_out_kernel, dim3(rc_grid(n_arc)), dim3(256), 0, ctx->stream, q, (const double *) d_tab, d_tab + 2 * n_link * 8, g->arc_out.as<double>());
    { int rc = rc_err(ctx, g); if (rc) return rc; }
    if (n_arc) CK(hipMemcpyAsync(arc_cov, g->arc_out.p, n_arc * 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return OATK_OK;
}

extern "C" int oatk_hip_ra_utg_coverage(oatk_hip_ctx *ctx, const oatk_racov_graph_t *hg, const oatk_racov_reads_t *reads, const oatk_racov_aln_t *aln,
                                        int verbose, double *utg_cov, uint64_t *n_iter)
{
    if (!ctx) return OATK_E_NODEV;
    return rc_utg_impl(ctx, nullptr, hg, reads, aln, verbose, utg_cov, n_iter);
}

extern "C" int oatk_hip_ra_arc_coverage(oatk_hip_ctx *ctx, const oatk_racov_graph_t *hg, const oatk_racov_aln_t *aln, double *arc_cov)
{
    if (!ctx) return OATK_E_NODEV;
    return rc_arc_impl(ctx, nullptr, hg, aln, arc_cov);
}

extern "C" int oatk_hip_ra_utg_coverage_sharded(oatk_hip_ctx *ctx, oatk_comm *c, const oatk_racov_graph_t *hg, const oatk_racov_reads_t *reads,
                                                const oatk_racov_aln_t *aln, int verbose, double *utg_cov, uint64_t *n_iter)
{
    if (!ctx) return OATK_E_NODEV;
    if (!c) { ctx->err = "oatk_hip_ra_utg_coverage_sharded: no communicator"; return OATK_E_ARG; }
    return comm_finish(c, rc_utg_impl(ctx, c, hg, reads, aln, verbose, utg_cov, n_iter));
}

extern "C" int oatk_hip_ra_arc_coverage_sharded(oatk_hip_ctx *ctx, oatk_comm *c, const oatk_racov_graph_t *hg, const oatk_racov_aln_t *aln, double *arc_cov)
{
    if (!ctx) return OATK_E_NODEV;
    if (!c) { ctx->err = "oatk_hip_ra_arc_coverage_sharded: no communicator"; return OATK_E_ARG; }
    return comm_finish(c, rc_arc_impl(ctx, c, hg, aln, arc_cov));
}
