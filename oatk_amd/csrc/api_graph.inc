// oatk_amd/csrc/api_graph.inc -- C ABI of the assembly graph built on the device (include/oatk_hip_graph.h); part of api.hip,
// after api_ec.inc (shares its scan helper and the arc unpacking of ecgraph.hpp).
#include "../../include/oatk_hip_graph.h"
#include "asmgraph.hpp"
#include <rocprim/device/device_reduce_by_key.hpp>

struct AgState {
    DevBuf keys, keys2, ukeys, counts, nruns, nout, nout64, outoff, akey, aval, skey, sval;
    DevBuf del, keep, keep64, vidx, vtx_scm, vtx_cov, idx_p, idx_n, arc_v, arc_w, arc_ls, arc_cov, arc_comp, arc_del, flags;
    DevBuf opens, opens64, open_rank, comp_idx, link, wgt2;
    uint64_t n_scm = 0, n_vtx = 0, n_arc = 0;
    bool done = false;
};

static void ag_state_free(oatk_hip_ctx *ctx)
{
    delete ctx->ag;          // (its buffers free themselves: ~DevBuf)
    ctx->ag = nullptr;
}

static int ag_buffer(oatk_hip_ctx *ctx, int which, const void **d_ptr, uint64_t *bytes)
{
    AgState *g = ctx->ag;
    if (!g || !g->done) { ctx->err = "assembly graph requested before oatk_hip_asm_graph"; return OATK_E_STATE; }
    const uint64_t nv = g->n_vtx, na = g->n_arc;
    switch (which) {
        case OATK_BUF_AG_SCM_DEL: *d_ptr = g->del.p, *bytes = g->n_scm; break;
        case OATK_BUF_AG_VTX_SCM: *d_ptr = g->vtx_scm.p, *bytes = nv * 4; break;
        case OATK_BUF_AG_VTX_COV: *d_ptr = g->vtx_cov.p, *bytes = nv * 4; break;
        case OATK_BUF_AG_IDX_P: *d_ptr = g->idx_p.p, *bytes = 2 * nv * 8; break;
        case OATK_BUF_AG_IDX_N: *d_ptr = g->idx_n.p, *bytes = 2 * nv * 4; break;
        case OATK_BUF_AG_ARC_V: *d_ptr = g->arc_v.p, *bytes = na * 8; break;
        case OATK_BUF_AG_ARC_W: *d_ptr = g->arc_w.p, *bytes = na * 8; break;
        case OATK_BUF_AG_ARC_COV: *d_ptr = g->arc_cov.p, *bytes = na * 4; break;
        case OATK_BUF_AG_ARC_COMP: *d_ptr = g->arc_comp.p, *bytes = na; break;
        case OATK_BUF_AG_ARC_LINK: *d_ptr = g->link.p, *bytes = na * 8; break;
        default: ctx->err = "unknown buffer id"; return OATK_E_ARG;
    }
    return OATK_OK;
}

#define AGENSURE(buf, bytes) ENSURE_IN(g, "graph.", buf, bytes)

// canonical keys of this batch's adjacent pairs: the corrected chains after oatk_hip_ec, the counted ones otherwise
extern "C" int oatk_hip_asm_pairs(oatk_hip_ctx *ctx, const void **d_keys, uint64_t *n_pairs)
{
    using namespace oatk;
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->counted) { ctx->err = "oatk_hip_asm_pairs needs a resident scan + count"; return OATK_E_STATE; }
    CK(hipSetDevice(ctx->device));
    if (!ctx->ag) ctx->ag = new AgState();
    AgState *g = ctx->ag;
    EcState *e = ctx->ec;
    const bool after_ec = e && e->done;
    const uint64_t nr = ctx->n_reads, nocc = after_ec? e->new_tot : ctx->n_occ;
    AGENSURE(keys, (nocc + 1) * 8);
    if (nocc) hipLaunchKernelGGL(agr_pair_keys_kernel, dim3((unsigned) ((nr + 255) / 256)), dim3(256), 0, ctx->stream, nr,
                                 after_ec? e->new_off.as<uint64_t>() : ctx->scm_off.as<uint64_t>(),
                                 after_ec? e->new_k.as<uint64_t>() : ec_chains(ctx),
                                 after_ec? e->new_m.as<uint32_t>() : ctx->pos_mpos.as<uint32_t>(), g->keys.as<uint64_t>());
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    *d_keys = g->keys.p, *n_pairs = nocc;
    return OATK_OK;
}

// d_wgt == nullptr: every key stands for one adjacency; otherwise key i stands for d_wgt[i] of them (what shards exchange: their own keys sorted and
// run-length encoded, include/oatk_hip_multi.h)
static int ag_build(oatk_hip_ctx *ctx, const uint64_t *d_keys, const uint32_t *d_wgt, uint64_t nocc, uint64_t ns, const uint32_t *d_cov,
                    const uint8_t *d_del, uint32_t min_k_cov, double min_a_cov_f, uint64_t *n_vtx, uint64_t *n_arc)
{
    using namespace oatk;
    if (!ctx) return OATK_E_NODEV;
    if (nocc >= 0xFFFFFFFFULL) { ctx->err = "more than 2^32 adjacent pairs"; return OATK_E_ARG; }
    if (ns >= 0x7FFFFFFFULL) { ctx->err = "too many syncmers for 32-bit oriented vertex ids"; return OATK_E_ARG; }
    if (!(min_a_cov_f >= 0.)) { ctx->err = "oatk_hip_asm_graph: min_a_cov_f must be >= 0"; return OATK_E_ARG; }
    if (ns && !d_cov) { ctx->err = "oatk_hip_asm_graph: no coverage array"; return OATK_E_ARG; }
    CK(hipSetDevice(ctx->device));
    if (!ctx->ag) ctx->ag = new AgState();
    AgState *g = ctx->ag;
    g->done = false;
    AGENSURE(flags, 64);
    CK(hipMemsetAsync(g->flags.p, 0, 64, ctx->stream));

    // 1. vertices: coverage filter, squeeze (syncasm.c:226-233, graph.c:153-173)
    uint64_t nv = 0;
    AGENSURE(del, ns + 8); AGENSURE(keep, (ns + 1) * 4);
    if (ns) hipLaunchKernelGGL(agr_vtx_filter_kernel, grid256(ns), dim3(256), 0, ctx->stream, ns, d_cov, d_del, min_k_cov, g->del.as<uint8_t>(), g->keep.as<uint32_t>());
    { int rc = prim_scan_total_u32(ctx, g->keep, g->keep64, g->vidx, ns, &nv); if (rc) return rc; }
    AGENSURE(vtx_scm, (nv + 1) * 4); AGENSURE(vtx_cov, (nv + 1) * 4);
    if (ns) hipLaunchKernelGGL(agr_vtx_squeeze_kernel, grid256(ns), dim3(256), 0, ctx->stream, ns, g->del.as<uint8_t>(), g->vidx.as<uint64_t>(), d_cov,
                               g->vtx_scm.as<uint32_t>(), g->vtx_cov.as<uint32_t>());
    AGENSURE(idx_p, (2 * nv + 1) * 8); AGENSURE(idx_n, (2 * nv + 1) * 4);
    CK(hipMemsetAsync(g->idx_p.p, 0, (2 * nv + 1) * 8, ctx->stream));
    CK(hipMemsetAsync(g->idx_n.p, 0, (2 * nv + 1) * 4, ctx->stream));

    // 2. the arc counter (syncasm.c:242-261): sort the canonical keys, one run = one key with its count
    uint64_t na = 0;
    uint32_t n_runs = 0;
    if (nocc) {
        AGENSURE(keys2, (nocc + 1) * 8); AGENSURE(ukeys, (nocc + 1) * 8); AGENSURE(counts, (nocc + 1) * 4); AGENSURE(nruns, 64);
        uint64_t *keys_in = const_cast<uint64_t *>(d_keys);
        if (d_wgt) {
            AGENSURE(wgt2, (nocc + 1) * 4);
            uint32_t *wgt_in = const_cast<uint32_t *>(d_wgt);
            PRIM(rocprim::radix_sort_pairs, keys_in, g->keys2.as<uint64_t>(), wgt_in, g->wgt2.as<uint32_t>(), nocc, 0, 64, ctx->stream);
            PRIM(rocprim::reduce_by_key, g->keys2.as<uint64_t>(), g->wgt2.as<uint32_t>(), (unsigned int) nocc, g->ukeys.as<uint64_t>(), g->counts.as<uint32_t>(), g->nruns.as<uint32_t>(),
                 rocprim::plus<uint32_t>(), rocprim::equal_to<uint64_t>(), ctx->stream);
        } else {
            int rc = prim_sort_runs(ctx, keys_in, g->keys2.as<uint64_t>(), (void *) nullptr, (void *) nullptr, nocc, 0, 64, g->ukeys.as<uint64_t>(), g->counts.as<uint32_t>(), g->nruns.as<uint32_t>());
            if (rc) return rc;
        }
        CK(hipMemcpyAsync(&n_runs, g->nruns.p, 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        // 3. the arc filter, arcs + complements in the squeezed numbering (syncasm.c:264-282, graph.c:175-200)
        AGENSURE(nout, ((uint64_t) n_runs + 1) * 4);
        hipLaunchKernelGGL(agr_expand_count_kernel, grid256(n_runs), dim3(256), 0, ctx->stream, (uint64_t) n_runs, g->ukeys.as<uint64_t>(), g->counts.as<uint32_t>(),
                           d_cov, g->del.as<uint8_t>(), min_a_cov_f, g->nout.as<uint32_t>());
        { int rc = prim_scan_total_u32(ctx, g->nout, g->nout64, g->outoff, n_runs, &na); if (rc) return rc; }
        AGENSURE(akey, (na + 1) * 8); AGENSURE(aval, (na + 1) * 8); AGENSURE(skey, (na + 1) * 8); AGENSURE(sval, (na + 1) * 8);
        if (na) {
            hipLaunchKernelGGL(agr_expand_kernel, grid256(n_runs), dim3(256), 0, ctx->stream, (uint64_t) n_runs, g->ukeys.as<uint64_t>(), g->counts.as<uint32_t>(),
                               g->nout.as<uint32_t>(), g->outoff.as<uint64_t>(), g->vidx.as<uint64_t>(), g->akey.as<uint64_t>(), g->aval.as<uint64_t>());
            // 4. (v, w) order, asmg_arc_sort graph.c:70-83
            PRIM(rocprim::radix_sort_pairs, g->akey.as<uint64_t>(), g->skey.as<uint64_t>(), g->aval.as<uint64_t>(), g->sval.as<uint64_t>(), na, 0, 64, ctx->stream);
        }
    }
    AGENSURE(arc_v, (na + 1) * 8); AGENSURE(arc_w, (na + 1) * 8); AGENSURE(arc_ls, (na + 1) * 4); AGENSURE(arc_cov, (na + 1) * 4); AGENSURE(arc_del, na + 8);
    AGENSURE(arc_comp, na + 8); AGENSURE(link, (na + 1) * 8);
    if (na) {
        // 5. arrays, index, symmetry flags (graph.c:85-113, :205-233)
        EgrArcs a;
        a.n_arc = na, a.arc_v = g->arc_v.as<uint64_t>(), a.arc_w = g->arc_w.as<uint64_t>(), a.arc_ls = g->arc_ls.as<uint32_t>(), a.arc_cov = g->arc_cov.as<uint32_t>();
        a.arc_comp = g->arc_comp.as<uint8_t>(), a.arc_del = g->arc_del.as<uint8_t>(), a.idx_p = g->idx_p.as<uint64_t>(), a.idx_n = g->idx_n.as<uint32_t>();
        a.flags = g->flags.as<uint32_t>();
        hipLaunchKernelGGL(egr_unpack_kernel, grid256(na), dim3(256), 0, ctx->stream, a, (const uint64_t *) g->skey.p, (const uint64_t *) g->sval.p);
        // 6. link ids (graph.c:126-146)
        AGENSURE(opens, (na + 1) * 4); AGENSURE(comp_idx, (na + 1) * 8);
        hipLaunchKernelGGL(agr_link_first_kernel, grid256(na), dim3(256), 0, ctx->stream, na, (const uint64_t *) g->skey.p, g->opens.as<uint32_t>(), g->comp_idx.as<uint64_t>());
        uint64_t n_link = 0;
        { int rc = prim_scan_total_u32(ctx, g->opens, g->opens64, g->open_rank, na, &n_link); if (rc) return rc; }
        hipLaunchKernelGGL(agr_link_assign_kernel, grid256(na), dim3(256), 0, ctx->stream, na, g->opens.as<uint32_t>(), g->comp_idx.as<uint64_t>(),
                           g->open_rank.as<uint64_t>(), g->link.as<uint64_t>());
    }
    uint32_t fl[4] = {0, 0, 0, 0};
    CK(hipMemcpyAsync(fl, g->flags.p, sizeof(fl), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    if (fl[0]) { ctx->err = "assembly graph has duplicate arcs (a syncmer adjacent to itself on both strands): the reference's order is unspecified"; return OATK_E_SPLIT; }
    if (debug_refuse(ctx, 2, "oatk_hip_asm_graph")) return OATK_E_SPLIT;
    g->n_scm = ns, g->n_vtx = nv, g->n_arc = na;
    g->done = true;
    if (n_vtx) *n_vtx = nv;
    if (n_arc) *n_arc = na;
    return OATK_OK;
}

extern "C" int oatk_hip_asm_graph_from_pairs(oatk_hip_ctx *ctx, const uint64_t *d_keys, uint64_t nocc, uint64_t ns, const uint32_t *d_cov,
                                             const uint8_t *d_del, uint32_t min_k_cov, double min_a_cov_f, uint64_t *n_vtx, uint64_t *n_arc)
{
    return ag_build(ctx, d_keys, nullptr, nocc, ns, d_cov, d_del, min_k_cov, min_a_cov_f, n_vtx, n_arc);
}

extern "C" int oatk_hip_asm_graph(oatk_hip_ctx *ctx, uint32_t min_k_cov, double min_a_cov_f, uint64_t *n_vtx, uint64_t *n_arc)
{
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->counted) { ctx->err = "oatk_hip_asm_graph needs a resident scan + count"; return OATK_E_STATE; }
    EcState *e = ctx->ec;
    const bool after_ec = e && e->done;
    if (after_ec && e->global) { ctx->err = "oatk_hip_asm_graph: reads are sharded; gather the pairs and call oatk_hip_asm_graph_from_pairs"; return OATK_E_STATE; }
    const void *k = nullptr;
    uint64_t n = 0;
    int rc = oatk_hip_asm_pairs(ctx, &k, &n);
    if (rc) return rc;
    return oatk_hip_asm_graph_from_pairs(ctx, (const uint64_t *) k, n, ctx->n_scm_total, after_ec? e->cov.as<uint32_t>() : ctx->scm_cov.as<uint32_t>(),
                                         after_ec? e->scm_del.as<uint8_t>() : nullptr, min_k_cov, min_a_cov_f, n_vtx, n_arc);
}
