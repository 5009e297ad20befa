// oatk_amd/csrc/api_multiplex.inc -- C ABI of the spanning-triplet scores of scg_multiplex (include/oatk_hip_racov.h), for one handle and for reads
// sharded by record over several; part of api.hip, after api_racov.inc whose state, binding and collectives it shares.
#include "triplet.hpp"
#include <algorithm>

// the pairs scg_multiplex looks up (syncasm.c:1181-1240) from the flattened graph, in its order; false: the arc index points outside the arcs
static bool rc_tri_pairs(const oatk_racov_graph_t *hg, std::vector<uint64_t> &off, std::vector<uint64_t> &p_in, std::vector<uint64_t> &p_out)
{
    const uint64_t nu = hg->n_utg, n_arc = hg->n_arc;
    std::vector<uint64_t> l_in;
    off.assign(nu + 1, 0);
    for (uint64_t i = 0; i < nu; ++i) {
        off[i] = p_in.size();
        if (hg->vtx_del && hg->vtx_del[i]) continue;
        const uint64_t v1 = i << 1;
        for (int side = 0; side < 2; ++side) if (hg->idx_p[v1 | side] > n_arc || hg->idx_n[v1 | side] > n_arc - hg->idx_p[v1 | side]) return false;
        l_in.clear();
        for (uint64_t s = hg->idx_p[v1 | 1], e = s + hg->idx_n[v1 | 1]; s < e; ++s) {
            if (hg->arc_del[s]) continue;
            const uint64_t id = hg->arc_link[s] << 1 | hg->arc_comp[s];
            l_in.push_back((hg->arc_v[s] ^ 1) != hg->arc_w[s]? id ^ 1 : id);          // asmg_comp_arc_id
        }
        for (uint64_t x : l_in)
            for (uint64_t t = hg->idx_p[v1], e = t + hg->idx_n[v1]; t < e; ++t)
                if (!hg->arc_del[t]) p_in.push_back(x), p_out.push_back(hg->arc_link[t] << 1 | hg->arc_comp[t]);
    }
    off[nu] = p_in.size();
    return true;
}

static int rc_tri_impl(oatk_hip_ctx *ctx, oatk_comm *c, const oatk_racov_graph_t *hg, const oatk_racov_aln_t *aln, uint64_t *pair_off, uint64_t n_pair_cap,
                       uint64_t *n_pair, uint64_t *pair_in, uint64_t *pair_out, double *score, uint8_t *have)
{
    using namespace oatk;
    const char *who = c? "oatk_hip_ra_triplet_scores_sharded" : "oatk_hip_ra_triplet_scores";
    if (c) { int rc = comm_check(ctx, c, who); if (rc) return rc; }
    if (!pair_off || !n_pair || (n_pair_cap && (!pair_in || !pair_out || !score || !have))) { ctx->err = std::string(who) + ": no output"; return OATK_E_ARG; }
    CK(hipSetDevice(ctx->device));
    if (c && !ctx->multi) ctx->multi = new MultiState();
    RcState *g = rc_state(ctx);
    RcArgs a;
    { int rc = rc_bind(ctx, g, hg, nullptr, aln, false, c != nullptr, &a); if (rc) return rc; }
    const uint64_t nu = hg->n_utg, n_arc = hg->n_arc, m_scm = hg->utg_off[nu];
    if (nu && (!hg->idx_p || !hg->idx_n)) { ctx->err = std::string(who) + ": no arc index"; return OATK_E_ARG; }
    if (n_arc && (!hg->arc_v || !hg->arc_w || !hg->arc_link || !hg->arc_comp || !hg->arc_del)) { ctx->err = std::string(who) + ": no arcs"; return OATK_E_ARG; }
    for (uint64_t i = 0; i < n_arc; ++i) if (hg->arc_link[i] >> 32) { ctx->err = std::string(who) + ": link ids beyond 2^32"; return OATK_E_ARG; }
    // the pairs, and the groups of keys they name (graph-sized work, the same on every rank)
    std::vector<uint64_t> off, p_in, p_out;
    if (!rc_tri_pairs(hg, off, p_in, p_out)) { ctx->err = std::string(who) + ": the arc index points outside the arcs"; return OATK_E_ARG; }
    const uint64_t np = p_in.size();
    std::vector<uint64_t> grp(np);
    for (uint64_t p = 0; p < np; ++p) grp[p] = rc_tri_group(p_in[p], p_out[p]);
    std::sort(grp.begin(), grp.end());
    grp.erase(std::unique(grp.begin(), grp.end()), grp.end());
    const uint64_t ng = grp.size();
    if (ng >= (1ull << 28)) { ctx->err = std::string(who) + ": more than 2^28 groups of triplet keys"; return OATK_E_ARG; }
    std::vector<uint32_t> pslot(np);
    for (uint64_t p = 0; p < np; ++p) {
        const uint64_t gk = rc_tri_group(p_in[p], p_out[p]);
        pslot[p] = (uint32_t) (8 * (uint64_t) (std::lower_bound(grp.begin(), grp.end(), gk) - grp.begin()) + rc_tri_slot(p_in[p], p_out[p], gk >> 32));
    }
    RC_UPLOAD(idx_p, hg->idx_p, 2 * nu * 8); RC_UPLOAD(idx_n, hg->idx_n, 2 * nu * 8);
    RC_UPLOAD(arc_v, hg->arc_v, n_arc * 8); RC_UPLOAD(arc_w, hg->arc_w, n_arc * 8); RC_UPLOAD(arc_link, hg->arc_link, n_arc * 8);
    RC_UPLOAD(arc_comp, hg->arc_comp, n_arc); RC_UPLOAD(arc_del, hg->arc_del, n_arc);
    RC_UPLOAD(t_grp, grp.data(), ng * 8); RC_UPLOAD(t_pslot, pslot.data(), np * 4);
    RcArcArgs q;
    q.idx_p = g->idx_p.as<uint64_t>(), q.idx_n = g->idx_n.as<uint64_t>(), q.arc_v = g->arc_v.as<uint64_t>(), q.arc_w = g->arc_w.as<uint64_t>();
    q.arc_link = g->arc_link.as<uint64_t>(), q.arc_comp = g->arc_comp.as<uint8_t>(), q.arc_del = g->arc_del.as<uint8_t>(), q.n_arc = n_arc, q.n_link = 0;
    RC_ENSURE(err, 4);
    CK(hipMemsetAsync(g->err.p, 0, 4, ctx->stream));
    a.err = g->err.as<unsigned int>();
    const uint64_t na = a.n_aln;
    uint64_t nf = 0;
    if (na) {
        CK(hipMemcpyAsync(&nf, a.off + na, 8, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
    }
    // the table: per group eight values, then the eight flags of every group -- one stretch of memory, so that it travels as one piece
    const uint64_t tab = ng * 64 + ng * 8;
    RC_ENSURE(lv, tab + 16);
    if (c) RC_ENSURE(carry, tab + 16);
    CK(hipMemsetAsync(g->lv.p, 0, tab + 16, ctx->stream));
    int bad = OATK_OK;
    if (np > n_pair_cap) {
        char m[160];
        snprintf(m, sizeof(m), "%s: room for %llu pairs, the graph has %llu", who, (unsigned long long) n_pair_cap, (unsigned long long) np);
        ctx->err = m;
        bad = OATK_E_NOMEM;
    } else if (nf >> 31) { ctx->err = std::string(who) + ": 2^31 fragments or more"; bad = OATK_E_ARG; }
    else if (nf) {
        // which unitig positions hold a unique syncmer, as prefix sums
        RC_ENSURE(flag, (m_scm + 1) * 8); RC_ENSURE(pos, (m_scm + 1) * 8);
        CK(hipMemsetAsync(g->flag.p, 0, (m_scm + 1) * 8, ctx->stream));
        if (m_scm) hipLaunchKernelGGL(rc_tri_uniq_kernel, dim3(rc_grid(m_scm)), dim3(256), 0, ctx->stream, a, m_scm, g->flag.as<uint64_t>());
        uint64_t n_uq = 0;
        { int rc = prim_scan_total(ctx, g->tmp, g->flag.as<uint64_t>(), g->pos.as<uint64_t>(), m_scm, &n_uq); if (rc) return rc; }
        // two contributions per event, sorted by slot; what the replay needs beside them does not depend on the table it goes on from
        RC_ENSURE(ev_key, nf * 8); RC_ENSURE(ev_key2, nf * 8); RC_ENSURE(ev_val, nf * 8); RC_ENSURE(ev_val2, nf * 8); RC_ENSURE(ev_score, nf * 8);
        RC_ENSURE(t_first, ng * 32); RC_ENSURE(t_last, ng * 32);
        CK(hipMemsetAsync(g->ev_key.p, 0xFF, nf * 8, ctx->stream));
        CK(hipMemsetAsync(g->ev_val.p, 0, nf * 8, ctx->stream));
        CK(hipMemsetAsync(g->t_first.p, 0xFF, ng * 32, ctx->stream));
        hipLaunchKernelGGL(rc_triplet_kernel, dim3(rc_grid(na) < 4096? rc_grid(na) : 4096), dim3(256), 0, ctx->stream, a, q, g->pos.as<uint64_t>(), g->t_grp.as<uint64_t>(), ng,
                           g->ev_key.as<uint32_t>(), g->ev_val.as<uint32_t>(), g->t_first.as<uint32_t>(), g->ev_score.as<double>());
        bad = rc_err(ctx, g);
        if (!bad) {
            const uint64_t nc = 2 * nf;
            RC_PRIM(rocprim::radix_sort_pairs, g->ev_key.as<uint32_t>(), g->ev_key2.as<uint32_t>(), g->ev_val.as<uint32_t>(),
                    g->ev_val2.as<uint32_t>(), nc, 0, 32, ctx->stream);
            RC_ENSURE(em_w, (nc + 1) * 8); RC_ENSURE(em_e, (nc + 1) * 8); RC_ENSURE(em_fl, (nc + 1) * 8); RC_ENSURE(em_ef, (nc + 1) * 8);
            CK(hipMemsetAsync(g->em_w.p, 0, (nc + 1) * 8, ctx->stream)); CK(hipMemsetAsync(g->em_fl.p, 0, (nc + 1) * 8, ctx->stream));
            hipLaunchKernelGGL(rc_tri_prep_kernel, dim3(rc_grid(nc)), dim3(256), 0, ctx->stream, nc, g->ev_key2.as<uint32_t>(), g->ev_val2.as<uint32_t>(), g->ev_score.as<double>(),
                               g->em_w.as<uint64_t>(), g->em_fl.as<uint64_t>());
            uint64_t n_one = 0, n_frac = 0;
            { int rc = prim_scan_total(ctx, g->tmp, g->em_w.as<uint64_t>(), g->em_e.as<uint64_t>(), nc, &n_one); if (rc) return rc; }
            { int rc = prim_scan_total(ctx, g->tmp, g->em_fl.as<uint64_t>(), g->em_ef.as<uint64_t>(), nc, &n_frac); if (rc) return rc; }
            RC_ENSURE(em_fpos, (n_frac + 1) * 8);
            hipLaunchKernelGGL(rc_fpos_kernel, dim3(rc_grid(nc)), dim3(256), 0, ctx->stream, nc, g->em_fl.as<uint64_t>(), g->em_ef.as<uint64_t>(), g->em_fpos.as<uint64_t>());
        }
    }
    { int rc = rc_verdict(ctx, c, bad, who); if (rc) { if (rc == OATK_E_NOMEM) *n_pair = np; return rc; } }     // a missing arc on any rank is everybody's refusal
    // A rank's contributions sorted stably by slot are a stretch of the reference's put order for every key: rank r replays its own on top of
    // the table as rank r - 1 left it, and the last rank's table is everybody's
    for (int r = 0; r < (c? c->n : 1); ++r) {
        if (!c || c->rank == r) {
            if (r && tab) CK(hipMemcpyAsync(g->lv.p, g->carry.p, tab, hipMemcpyDeviceToDevice, ctx->stream));
            if (nf && ng) {
                uint8_t *have8 = g->lv.as<uint8_t>() + ng * 64;
                CK(hipMemsetAsync(g->t_last.p, 0, ng * 32, ctx->stream));
                hipLaunchKernelGGL(rc_tri_assign_kernel, dim3(rc_grid(nf)), dim3(256), 0, ctx->stream, nf, g->ev_key.as<uint32_t>(), g->t_first.as<uint32_t>(), have8, g->t_last.as<uint32_t>());
                hipLaunchKernelGGL(rc_tri_replay_kernel, dim3(rc_grid(2 * nf)), dim3(256), 0, ctx->stream, 2 * nf, g->ev_key2.as<uint32_t>(), g->ev_val2.as<uint32_t>(), g->ev_score.as<double>(),
                                   g->t_last.as<uint32_t>(), g->em_e.as<uint64_t>(), g->em_ef.as<uint64_t>(), g->em_fpos.as<uint64_t>(), g->lv.as<double>(), have8);
            }
        }
        if (c) { int rc = rc_bcast(ctx, c, r, g->lv.p, g->carry.p, tab); if (rc) return rc; }
    }
    const uint8_t *d_tab = c? g->carry.as<uint8_t>() : g->lv.as<uint8_t>();
    RC_ENSURE(t_score, np * 8); RC_ENSURE(t_have, np);
    if (np) hipLaunchKernelGGL(rc_tri_out_kernel, dim3(rc_grid(np)), dim3(256), 0, ctx->stream, np, g->t_pslot.as<uint32_t>(), (const double *) d_tab, d_tab + ng * 64,
                               g->t_score.as<double>(), g->t_have.as<uint8_t>());
    std::vector<double> h_score(np);
    std::vector<uint8_t> h_have(np);
    if (np) {
        CK(hipMemcpyAsync(h_score.data(), g->t_score.p, np * 8, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipMemcpyAsync(h_have.data(), g->t_have.p, np, hipMemcpyDeviceToHost, ctx->stream));
    }
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    // everything went well: only now the caller's arrays are written
    memcpy(pair_off, off.data(), (nu + 1) * 8);
    if (np) {
        memcpy(pair_in, p_in.data(), np * 8), memcpy(pair_out, p_out.data(), np * 8);
        memcpy(score, h_score.data(), np * 8), memcpy(have, h_have.data(), np);
    }
    *n_pair = np;
    return OATK_OK;
}

extern "C" int oatk_hip_ra_triplet_scores(oatk_hip_ctx *ctx, const oatk_racov_graph_t *hg, const oatk_racov_aln_t *aln, uint64_t *pair_off, uint64_t n_pair_cap,
                                          uint64_t *n_pair, uint64_t *pair_in, uint64_t *pair_out, double *score, uint8_t *have)
{
    if (!ctx) return OATK_E_NODEV;
    return rc_tri_impl(ctx, nullptr, hg, aln, pair_off, n_pair_cap, n_pair, pair_in, pair_out, score, have);
}

extern "C" int oatk_hip_ra_triplet_scores_sharded(oatk_hip_ctx *ctx, oatk_comm *c, const oatk_racov_graph_t *hg, const oatk_racov_aln_t *aln, uint64_t *pair_off,
                                                  uint64_t n_pair_cap, uint64_t *n_pair, uint64_t *pair_in, uint64_t *pair_out, double *score, uint8_t *have)
{
    if (!ctx) return OATK_E_NODEV;
    if (!c) { ctx->err = "oatk_hip_ra_triplet_scores_sharded: no communicator"; return OATK_E_ARG; }
    return comm_finish(c, rc_tri_impl(ctx, c, hg, aln, pair_off, n_pair_cap, n_pair, pair_in, pair_out, score, have));
}
