// oatk_amd/csrc/api_bam.inc -- C ABI of the device reader of unaligned BAM (include/oatk_hip_ingest.h: oatk_hip_ingest_bam); part of api.hip, behind api_ingest.inc:
// the result is IngState's resident packed stream, in the layout oatk_hip_ingest leaves.
#include "bam.hpp"

// the header, walked on the host over a copy of the chunk's head that grows as l_text and the reference list ask.  *s0: where the first record starts;
// *whole_hdr = false: the chunk ends inside the header
static int bam_header(oatk_hip_ctx *ctx, const uint8_t *d_bam, uint64_t n_bytes, uint64_t *s0, bool *whole_hdr)
{
    std::vector<uint8_t> head;
    uint64_t have = n_bytes < 65536? n_bytes : 65536;
    *s0 = 0, *whole_hdr = false;
    for (;;) {
        head.resize((size_t) have);
        if (have) {
            CK(hipMemcpyAsync(head.data(), d_bam, have, hipMemcpyDeviceToHost, ctx->stream));       // stream-ordered: the bytes may still be on their way
            CK(hipStreamSynchronize(ctx->stream));
        }
        uint64_t len = 0, need = 0;
        const int v = oatk_bam::header_walk(head.data(), have, &len, &need);
        if (v == oatk_bam::HDR_BAD) { ctx->err = "oatk_hip_ingest_bam: not a BAM header (wrong magic or a negative length)"; return OATK_E_ARG; }
        if (v == oatk_bam::HDR_OK) { *s0 = len, *whole_hdr = true; return OATK_OK; }
        if (have == n_bytes) return OATK_OK;                                                         // the chunk ends inside the header
        have = need > 2 * have? need : 2 * have;
        if (have > n_bytes) have = n_bytes;
    }
}

extern "C" int oatk_hip_ingest_bam(oatk_hip_ctx *ctx, const uint8_t *d_bam, uint64_t n_bytes, int header, int final, uint64_t *n_reads, uint64_t *consumed)
{
    using namespace oatk;
    if (!ctx) return OATK_E_NODEV;
    CK(hipSetDevice(ctx->device));
    if (!ctx->ing) ctx->ing = new IngState();
    IngState *g = ctx->ing;
    g->done = false, g->bam = false, g->n_reads = 0, g->seq_bytes = 0;
    g->bam_stats[0] = g->bam_stats[1] = g->bam_stats[2] = 0;
    if (n_reads) *n_reads = 0;
    if (consumed) *consumed = 0;
    if (n_bytes && !d_bam) { ctx->err = "oatk_hip_ingest_bam: null argument"; return OATK_E_ARG; }
    uint64_t s0 = 0;
    if (header) {
        bool whole_hdr = false;
        { int rc = bam_header(ctx, d_bam, n_bytes, &s0, &whole_hdr); if (rc) return rc; }
        if (!whole_hdr) {
            if (final) { ctx->err = "oatk_hip_ingest_bam: BAM stream ends inside its header"; return OATK_E_ARG; }
            g->bam = true, g->done = true;                          // nothing taken: the caller comes back with more
            return OATK_OK;
        }
    }
    g->bam_stats[2] = s0;
    const bool tm = ctx->timing;                                    // phase times for tests/bam_time.py (oatk_hip_ingest_bam_times)
    if (tm && !g->bam_ev_made) { for (hipEvent_t &e : g->bam_ev) CK(hipEventCreate(&e)); g->bam_ev_made = true; }
    auto mark = [&](int i) { if (tm) (void) hipEventRecord(g->bam_ev[i], ctx->stream); };
    mark(0);
    const uint64_t nb = (n_bytes + BAM_BLOCK - 1) / BAM_BLOCK;
    if (nb >= 0x7FFFFFFFULL) { ctx->err = "oatk_hip_ingest_bam: chunk larger than 8 TiB"; return OATK_E_ARG; }

    // ---- candidates ----
    uint64_t m = 0, n_rec = 0;
    GENSURE(flags, 64); GENSURE(info, 64);
    CK(hipMemsetAsync(g->flags.p, 0, 8, ctx->stream));
    CK(hipMemsetAsync(g->flags.as<uint8_t>() + 8, 0xFF, 8, ctx->stream));                           // the first refused record: none
    if (s0 < n_bytes) {
        GENSURE(cnt, (nb + 1) * 4); GENSURE(cnt64, (nb + 1) * 8); GENSURE(blk_off, (nb + 1) * 8);
        hipLaunchKernelGGL(bam_count_cand_kernel, dim3((unsigned) nb), dim3(256), 0, ctx->stream, d_bam, n_bytes, s0, g->cnt.as<uint32_t>());
        hipLaunchKernelGGL(widen_kernel, grid256(nb + 1), dim3(256), 0, ctx->stream, g->cnt.as<uint32_t>(), g->cnt64.as<uint64_t>(), nb);
        PRIM(rocprim::exclusive_scan, g->cnt64.as<const uint64_t>(), g->blk_off.as<uint64_t>(), (uint64_t) 0, nb + 1, rocprim::plus<uint64_t>(), ctx->stream);
        CK(hipMemcpyAsync(&m, g->blk_off.as<uint64_t>() + nb, 8, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        g->bam_stats[0] = m;
        if (m > n_bytes / 16) { ctx->err = "oatk_hip_ingest_bam: more than one byte offset in 16 looks like a record start: not a BAM stream"; return OATK_E_SPLIT; }
        if (m >= 0xFFFFFFFFULL) { ctx->err = "oatk_hip_ingest_bam: more than 2^32 candidate records in one chunk"; return OATK_E_ARG; }
    }
    if (m) {
        GENSURE(bam_cand, (m + 1) * 8); GENSURE(bam_jump, (m + 1) * 4); GENSURE(bam_jump2, (m + 1) * 4); GENSURE(bam_mark, (m + 1) * 8); GENSURE(bam_rank, (m + 1) * 8);
        hipLaunchKernelGGL(bam_fill_cand_kernel, dim3((unsigned) nb), dim3(256), 0, ctx->stream, d_bam, n_bytes, s0, g->blk_off.as<uint64_t>(), g->bam_cand.as<uint64_t>());
        mark(1);
        // ---- successors, reachability from s0 by pointer doubling ----
        hipLaunchKernelGGL(bam_succ_kernel, grid256(m + 1), dim3(256), 0, ctx->stream, d_bam, g->bam_cand.as<uint64_t>(), m, s0, g->bam_jump.as<uint32_t>(), g->bam_mark.as<uint64_t>());
        uint32_t *ja = g->bam_jump.as<uint32_t>(), *jb = g->bam_jump2.as<uint32_t>();
        for (uint64_t reach = 1; reach < m + 1; reach <<= 1) {                                      // ceil(log2(m + 1)) rounds
            hipLaunchKernelGGL(bam_double_kernel, grid256(m + 1), dim3(256), 0, ctx->stream, m, ja, jb, g->bam_mark.as<uint64_t>());
            std::swap(ja, jb);
        }
        mark(2);
        // ---- the marked candidates are the records ----
        PRIM(rocprim::exclusive_scan, g->bam_mark.as<const uint64_t>(), g->bam_rank.as<uint64_t>(), (uint64_t) 0, m + 1, rocprim::plus<uint64_t>(), ctx->stream);
        CK(hipMemcpyAsync(&n_rec, g->bam_rank.as<uint64_t>() + m, 8, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
    }
    g->bam_stats[1] = n_rec;
    GENSURE(bam_rec, (n_rec + 1) * 8);
    if (n_rec) hipLaunchKernelGGL(bam_compact_kernel, grid256(m), dim3(256), 0, ctx->stream, g->bam_cand.as<uint64_t>(), m, g->bam_mark.as<uint64_t>(), g->bam_rank.as<uint64_t>(),
                                  g->bam_rec.as<uint64_t>());
    // ---- where the chain stops ----
    uint64_t stop[2] = {s0, oatk_bam::STOP_CLEAN};
    if (s0 < n_bytes) {
        hipLaunchKernelGGL(bam_stop_kernel, dim3(1), dim3(1), 0, ctx->stream, d_bam, n_bytes, s0, g->bam_rec.as<uint64_t>(), n_rec, g->info.as<uint64_t>());
        CK(hipMemcpyAsync(stop, g->info.p, sizeof(stop), hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
    }
    CK(hipGetLastError());
    if (stop[1] == oatk_bam::STOP_BAD || stop[1] == oatk_bam::STOP_NONE) {                         // (STOP_NONE cannot happen: a record there would be in the chain)
        ctx->err = "oatk_hip_ingest_bam: the bytes at offset " + std::to_string(stop[0]) + " are not a BAM record (block_size out of range, fields larger than the block, or a name without NUL)";
        return OATK_E_ARG;
    }
    if (stop[1] == oatk_bam::STOP_CUT && final) { ctx->err = "oatk_hip_ingest_bam: BAM stream ends inside a record (at offset " + std::to_string(stop[0]) + ")"; return OATK_E_ARG; }

    // ---- per record: length, place in the packed stream; the letters ----
    mark(3);
    GENSURE(len, (n_rec + 1) * 4); GENSURE(padded, (n_rec + 2) * 8); GENSURE(off, (n_rec + 2) * 8); GENSURE(hdr_off, (n_rec + 1) * 8);
    hipLaunchKernelGGL(bam_record_kernel, grid256(n_rec + 1), dim3(256), 0, ctx->stream, d_bam, g->bam_rec.as<uint64_t>(), n_rec, g->len.as<uint32_t>(), g->padded.as<uint64_t>(),
                       g->hdr_off.as<uint64_t>(), g->flags.as<uint32_t>(), (unsigned long long *) (g->flags.as<uint8_t>() + 8));
    PRIM(rocprim::exclusive_scan, g->padded.as<const uint64_t>(), g->off.as<uint64_t>(), (uint64_t) 0, n_rec + 1, rocprim::plus<uint64_t>(), ctx->stream);
    mark(4);
    uint64_t seq_bytes = 0;
    uint32_t fl[4] = {0, 0, 0, 0};
    CK(hipMemcpyAsync(&seq_bytes, g->off.as<uint64_t>() + n_rec, 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(fl, g->flags.p, sizeof(fl), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    if (fl[1]) {
        uint64_t bad = 0, at = 0;
        memcpy(&bad, fl + 2, 8);
        CK(hipMemcpyAsync(&at, g->hdr_off.as<uint64_t>() + bad, 8, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        ctx->err = "oatk_hip_ingest_bam: record " + std::to_string(bad) + " (offset " + std::to_string(at) + ") is reverse-complemented, secondary or supplementary (flag & 0x910): "
                   "samtools fasta would reverse or drop it; this reader takes unaligned BAM only";
        return OATK_E_SPLIT;
    }
    GENSURE(seq, seq_bytes + 64);
    mark(5);
    if (n_rec) hipLaunchKernelGGL(bam_unpack_kernel, dim3((unsigned) ((n_rec + 3) / 4)), dim3(256), 0, ctx->stream, d_bam, g->bam_rec.as<uint64_t>(), n_rec, g->off.as<uint64_t>(),
                                  g->seq.as<uint8_t>());
    mark(6);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 5; ++i) g->bam_ms[i] = 0.f;
    if (tm && m) {
        static const int from[5] = {0, 1, 2, 3, 5}, to[5] = {1, 2, 3, 4, 6};
        for (int i = 0; i < 5; ++i) (void) hipEventElapsedTime(&g->bam_ms[i], g->bam_ev[from[i]], g->bam_ev[to[i]]);
    }
    g->seq_bytes = seq_bytes, g->n_reads = n_rec, g->bam = true, g->done = true;
    if (n_reads) *n_reads = n_rec;
    if (consumed) *consumed = stop[0];
    return OATK_OK;
}

extern "C" int oatk_hip_ingest_bam_host(oatk_hip_ctx *ctx, const uint8_t *h_bam, uint64_t n_bytes, int header, int final, uint64_t *n_reads, uint64_t *consumed)
{
    if (!ctx) return OATK_E_NODEV;
    CK(hipSetDevice(ctx->device));
    if (!ctx->ing) ctx->ing = new IngState();
    IngState *g = ctx->ing;
    g->done = false;
    GENSURE(text, n_bytes + 64);
    if (n_bytes) CK(hipMemcpyAsync(g->text.p, h_bam, n_bytes, hipMemcpyHostToDevice, ctx->stream));
    return oatk_hip_ingest_bam(ctx, g->text.as<uint8_t>(), n_bytes, header, final, n_reads, consumed);
}

extern "C" int oatk_hip_ingest_bam_stats(oatk_hip_ctx *ctx, uint64_t out[3])
{
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->ing || !out) { ctx->err = "oatk_hip_ingest_bam_stats needs oatk_hip_ingest_bam"; return OATK_E_STATE; }
    for (int i = 0; i < 3; ++i) out[i] = ctx->ing->bam_stats[i];
    return OATK_OK;
}

// milliseconds of the phases of the latest oatk_hip_ingest_bam that ran with oatk_hip_set_timing on (zeros otherwise): candidate passes (with the copy of their
// count), successors + doubling rounds, compaction + stop, record kernel + offsets scan, unpack kernel
extern "C" int oatk_hip_ingest_bam_times(oatk_hip_ctx *ctx, float ms[5])
{
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->ing || !ms) { ctx->err = "oatk_hip_ingest_bam_times needs oatk_hip_ingest_bam"; return OATK_E_STATE; }
    for (int i = 0; i < 5; ++i) ms[i] = ctx->ing->bam_ms[i];
    return OATK_OK;
}
