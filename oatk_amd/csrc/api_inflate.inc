// oatk_amd/csrc/api_inflate.inc -- C ABI of the device BGZF inflater (include/oatk_hip_ingest.h); part of api.hip.
#include "inflate.hpp"
#include "ingest_names.hpp"

struct InfState {
    DevBuf members, status, res, x2n, comp, name_len, name_off, name_out;
    std::vector<uint8_t> h_names;
    bool x2n_ready = false;
    uint32_t last_byte = 0;
};

static void inf_state_free(oatk_hip_ctx *ctx)
{
    delete ctx->inf;          // (its buffers free themselves: ~DevBuf)
    ctx->inf = nullptr;
}

#define FENSURE(buf, bytes) ENSURE_IN(g, "inflate.", buf, bytes)

extern "C" int oatk_hip_inflate_bgzf(oatk_hip_ctx *ctx, const uint8_t *d_comp, uint64_t comp_bytes, const oatk_bgzf_member_t *h_members, uint64_t n,
                                     uint8_t *d_text, uint64_t text_cap, uint64_t *n_bad, uint8_t *h_status)
{
    using namespace oatk;
    if (!ctx) return OATK_E_NODEV;
    if (n_bad) *n_bad = 0;
    if (n == 0) return OATK_OK;
    if (!h_members || !d_comp || !d_text) { ctx->err = "oatk_hip_inflate_bgzf: null argument"; return OATK_E_ARG; }
    if (n >= 0x7FFFFFFFULL) { ctx->err = "oatk_hip_inflate_bgzf: more than 2^31 members in one call"; return OATK_E_ARG; }
    // the table, before anything is launched on its word: members inside the compressed bytes, outputs ascending, disjoint and inside the text
    uint64_t text_end = 0, last = n;
    for (uint64_t i = 0; i < n; ++i) {
        const oatk_bgzf_member_t &M = h_members[i];
        const bool ok = M.in_len <= oatk_inf::MAX_MEMBER && M.out_len <= oatk_inf::MAX_MEMBER && M.in_off <= comp_bytes && M.in_len <= comp_bytes - M.in_off
                        && M.out_off >= text_end && M.out_off <= text_cap && M.out_len <= text_cap - M.out_off;
        if (!ok) { ctx->err = "oatk_hip_inflate_bgzf: member " + std::to_string(i) + " of the table lies outside the buffers, overlaps the one before it or is larger than 64 KiB"; return OATK_E_ARG; }
        text_end = M.out_off + M.out_len;
        if (M.out_len) last = i;
    }
    CK(hipSetDevice(ctx->device));
    if (!ctx->inf) ctx->inf = new InfState();
    InfState *g = ctx->inf;
    FENSURE(members, n * sizeof(oatk_bgzf_member_t)); FENSURE(status, n); FENSURE(res, 16); FENSURE(x2n, 32 * 4);
    if (!g->x2n_ready) {
        uint32_t t[32];
        oatk_inf::crc_x2n_table(t);
        CK(hipMemcpyAsync(g->x2n.p, t, sizeof(t), hipMemcpyHostToDevice, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));          // (t lives on this stack frame)
        g->x2n_ready = true;
    }
    CK(hipMemcpyAsync(g->members.p, h_members, n * sizeof(oatk_bgzf_member_t), hipMemcpyHostToDevice, ctx->stream));
    CK(hipMemsetAsync(g->res.p, 0, 16, ctx->stream));
    hipLaunchKernelGGL(bgzf_inflate_kernel, dim3((unsigned) n), dim3(64), 0, ctx->stream, d_comp, g->members.as<oatk_bgzf_member_t>(), d_text,
                       g->x2n.as<uint32_t>(), g->status.as<uint8_t>(), g->res.as<uint32_t>(), last);
    CK(hipGetLastError());
    uint32_t res[2] = {0, 0};
    CK(hipMemcpyAsync(res, g->res.p, sizeof(res), hipMemcpyDeviceToHost, ctx->stream));
    if (h_status) CK(hipMemcpyAsync(h_status, g->status.p, n, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    g->last_byte = res[1];
    if (n_bad) *n_bad = res[0];
    return OATK_OK;
}

extern "C" int oatk_hip_inflate_bgzf_host(oatk_hip_ctx *ctx, const uint8_t *h_comp, uint64_t comp_bytes, const oatk_bgzf_member_t *h_members, uint64_t n,
                                          uint8_t *d_text, uint64_t text_cap, uint64_t *n_bad, uint8_t *h_status)
{
    if (!ctx) return OATK_E_NODEV;
    if (n_bad) *n_bad = 0;
    if (n == 0) return OATK_OK;
    if (!h_comp) { ctx->err = "oatk_hip_inflate_bgzf_host: null argument"; return OATK_E_ARG; }
    CK(hipSetDevice(ctx->device));
    if (!ctx->inf) ctx->inf = new InfState();
    InfState *g = ctx->inf;
    FENSURE(comp, comp_bytes + 64);
    if (comp_bytes) CK(hipMemcpyAsync(g->comp.p, h_comp, comp_bytes, hipMemcpyHostToDevice, ctx->stream));
    return oatk_hip_inflate_bgzf(ctx, g->comp.as<uint8_t>(), comp_bytes, h_members, n, d_text, text_cap, n_bad, h_status);
}

// the last byte of the text the latest oatk_hip_inflate_bgzf of this context produced (0 when it produced none): a reader needs it for kseq's rule that a file
// which ends without a newline gets one
extern "C" int oatk_hip_inflate_last_byte(oatk_hip_ctx *ctx)
{
    return ctx && ctx->inf? (int) ctx->inf->last_byte : 0;
}

// The names of the records the latest oatk_hip_ingest of this context found in d_text[0, n_bytes) -- the same text it was given -- cut on the device: one kernel takes
// each name's length, a scan places them, one kernel packs them, one copy brings offsets and names to the host.
extern "C" int oatk_hip_ingest_names(oatk_hip_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, const uint8_t **h_packed, const uint64_t **h_off, uint64_t *n_names)
{
    using namespace oatk;
    if (!ctx) return OATK_E_NODEV;
    IngState *ig = ctx->ing;
    if (!ig || !ig->done) { ctx->err = "oatk_hip_ingest_names needs oatk_hip_ingest"; return OATK_E_STATE; }
    if (!h_packed || !h_off) { ctx->err = "oatk_hip_ingest_names: null argument"; return OATK_E_ARG; }
    CK(hipSetDevice(ctx->device));
    if (!ctx->inf) ctx->inf = new InfState();
    InfState *g = ctx->inf;
    const uint64_t n = ig->n_reads;
    if (n_names) *n_names = n;
    g->h_names.assign((size_t) (n + 1) * 8, 0);
    if (n) {
        const dim3 grid((unsigned) ((n + 1 + 255) / 256));
        FENSURE(name_len, (n + 1) * 8); FENSURE(name_off, (n + 1) * 8);
        if (ig->bam) hipLaunchKernelGGL(ing_bam_name_len_kernel, grid, dim3(256), 0, ctx->stream, d_text, n_bytes, ig->hdr_off.as<uint64_t>(), n, g->name_len.as<uint64_t>());
        else hipLaunchKernelGGL(ing_name_len_kernel, grid, dim3(256), 0, ctx->stream, d_text, n_bytes, ig->hdr_off.as<uint64_t>(), n, g->name_len.as<uint64_t>());
        PRIM(rocprim::exclusive_scan, g->name_len.as<const uint64_t>(), g->name_off.as<uint64_t>(), (uint64_t) 0, n + 1, rocprim::plus<uint64_t>(), ctx->stream);
        uint64_t total = 0;
        CK(hipMemcpyAsync(&total, g->name_off.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        FENSURE(name_out, (n + 1) * 8 + total + 8);
        if (ig->bam) hipLaunchKernelGGL(ing_bam_name_copy_kernel, grid, dim3(256), 0, ctx->stream, d_text, ig->hdr_off.as<uint64_t>(), n, g->name_off.as<uint64_t>(), g->name_out.as<uint8_t>());
        else hipLaunchKernelGGL(ing_name_copy_kernel, grid, dim3(256), 0, ctx->stream, d_text, ig->hdr_off.as<uint64_t>(), n, g->name_off.as<uint64_t>(), g->name_out.as<uint8_t>());
        CK(hipGetLastError());
        g->h_names.resize((size_t) ((n + 1) * 8 + total));
        CK(hipMemcpyAsync(g->h_names.data(), g->name_out.p, g->h_names.size(), hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
    }
    *h_off = (const uint64_t *) g->h_names.data();
    *h_packed = g->h_names.data() + (n + 1) * 8;
    return OATK_OK;
}
