// oatk_amd/csrc/api_ingest.inc -- C ABI of the device record scan (include/oatk_hip_ingest.h); part of api.hip.
#include "../../include/oatk_hip_ingest.h"
#include "ingest.hpp"

struct IngState {
    DevBuf text, cnt, cnt64, blk_off, nl_pos, is_hdr, seq_len, hdr_rank, seq_before, hdr_line, len, padded, off, hdr_off, seq, flags, info;
    DevBuf bam_cand, bam_jump, bam_jump2, bam_mark, bam_rank, bam_rec;      // the record chain of a BAM chunk (api_bam.inc)
    uint64_t n_reads = 0, seq_bytes = 0;
    uint64_t bam_stats[3] = {0, 0, 0};      // candidates, records, header bytes of the latest oatk_hip_ingest_bam
    hipEvent_t bam_ev[7];                   // phase marks of oatk_hip_ingest_bam, made when a call first runs with oatk_hip_set_timing on
    bool bam_ev_made = false;
    float bam_ms[5] = {0, 0, 0, 0, 0};      // candidate passes, successors + doubling, compaction + stop, record kernel + scan, unpack kernel
    bool done = false;
    bool bam = false;             // the resident stream came from oatk_hip_ingest_bam: INGEST_HDR holds record offsets, and a name lies 36 bytes behind one
};

static void ing_state_free(oatk_hip_ctx *ctx)
{
    if (ctx->ing && ctx->ing->bam_ev_made) for (hipEvent_t e : ctx->ing->bam_ev) (void) hipEventDestroy(e);
    delete ctx->ing;          // (its buffers free themselves: ~DevBuf)
    ctx->ing = nullptr;
}

static int ing_buffer(oatk_hip_ctx *ctx, int which, const void **d_ptr, uint64_t *bytes)
{
    IngState *g = ctx->ing;
    if (!g || !g->done) { ctx->err = "ingest results requested before oatk_hip_ingest"; return OATK_E_STATE; }
    switch (which) {
        case OATK_BUF_INGEST_SEQ: *d_ptr = g->seq.p, *bytes = g->seq_bytes; break;
        case OATK_BUF_INGEST_OFF: *d_ptr = g->off.p, *bytes = g->n_reads * 8; break;
        case OATK_BUF_INGEST_LEN: *d_ptr = g->len.p, *bytes = g->n_reads * 4; break;
        case OATK_BUF_INGEST_HDR: *d_ptr = g->hdr_off.p, *bytes = g->n_reads * 8; break;
        default: ctx->err = "unknown buffer id"; return OATK_E_ARG;
    }
    return OATK_OK;
}

#define GENSURE(buf, bytes) ENSURE_IN(g, "ingest.", buf, bytes)

extern "C" int oatk_hip_ingest(oatk_hip_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, int format, int final, uint64_t *n_reads, uint64_t *consumed)
{
    using namespace oatk;
    if (!ctx) return OATK_E_NODEV;
    CK(hipSetDevice(ctx->device));
    if (!ctx->ing) ctx->ing = new IngState();
    IngState *g = ctx->ing;
    g->done = false, g->bam = false, g->n_reads = 0, g->seq_bytes = 0;
    if (n_reads) *n_reads = 0;
    if (consumed) *consumed = 0;
    if (n_bytes == 0) { g->done = true; return OATK_OK; }
    if (format == OATK_FMT_AUTO) {                      // the first character that is not white space
        uint8_t head[256];
        const uint64_t nh = n_bytes < sizeof(head)? n_bytes : sizeof(head);
        CK(hipMemcpyAsync(head, d_text, nh, hipMemcpyDeviceToHost, ctx->stream));       // stream-ordered: the text may still be on its way
        CK(hipStreamSynchronize(ctx->stream));
        uint64_t i = 0;
        while (i < nh && (head[i] == '\n' || head[i] == '\r' || head[i] == ' ' || head[i] == '\t')) ++i;
        format = i < nh && head[i] == '@'? OATK_FMT_FASTQ : OATK_FMT_FASTA;
    }
    if (format != OATK_FMT_FASTA && format != OATK_FMT_FASTQ && format != OATK_FMT_KSEQ) { ctx->err = "oatk_hip_ingest: unknown format"; return OATK_E_ARG; }

    // ---- newline positions ----
    const uint64_t nb = (n_bytes + ING_BLOCK - 1) / ING_BLOCK;
    if (nb >= 0x7FFFFFFFULL) { ctx->err = "oatk_hip_ingest: chunk larger than 8 TiB"; return OATK_E_ARG; }
    GENSURE(cnt, (nb + 1) * 4); GENSURE(cnt64, (nb + 1) * 8); GENSURE(blk_off, (nb + 1) * 8); GENSURE(flags, 64);
    CK(hipMemsetAsync(g->flags.p, 0, 64, ctx->stream));
    hipLaunchKernelGGL(ing_count_nl_kernel, dim3((unsigned) nb), dim3(256), 0, ctx->stream, d_text, n_bytes, g->cnt.as<uint32_t>());
    hipLaunchKernelGGL(widen_kernel, grid256(nb + 1), dim3(256), 0, ctx->stream, g->cnt.as<uint32_t>(), g->cnt64.as<uint64_t>(), nb);
    PRIM(rocprim::exclusive_scan, g->cnt64.as<const uint64_t>(), g->blk_off.as<uint64_t>(), (uint64_t) 0, nb + 1, rocprim::plus<uint64_t>(), ctx->stream);
    uint64_t n_nl = 0;
    uint8_t last = 0;
    CK(hipMemcpyAsync(&n_nl, g->blk_off.as<uint64_t>() + nb, 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(&last, d_text + n_bytes - 1, 1, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    GENSURE(nl_pos, (n_nl + 1) * 8);
    hipLaunchKernelGGL(ing_fill_nl_kernel, dim3((unsigned) nb), dim3(256), 0, ctx->stream, d_text, n_bytes, g->blk_off.as<uint64_t>(), g->nl_pos.as<uint64_t>());
    IngLines l;
    l.text = d_text, l.n_bytes = n_bytes, l.nl_pos = g->nl_pos.as<uint64_t>(), l.n_nl = n_nl;
    l.n_lines = n_nl + (last != '\n');                  // a last line without '\n' counts
    const uint64_t nl = l.n_lines;
    uint64_t n_rec = 0, used = n_bytes;

    if (format == OATK_FMT_FASTA || format == OATK_FMT_KSEQ) {
        GENSURE(is_hdr, (nl + 2) * 8); GENSURE(seq_len, (nl + 2) * 8); GENSURE(hdr_rank, (nl + 2) * 8); GENSURE(seq_before, (nl + 2) * 8);
        uint64_t n_hdr = 0, line_end = nl;
        bool cut_done = false;                          // the line-by-line reading has already left out what may continue in the next chunk
        if (format == OATK_FMT_KSEQ) {
            // ---- kseq_read, line by line (kseq.h:192-235): three numbers per line from the device, the walk over them here ----
            GENSURE(info, (nl + 1) * sizeof(IngLineInfo));
            if (nl) hipLaunchKernelGGL(ing_line_info_kernel, dim3((unsigned) ((nl + 3) / 4)), dim3(256), 0, ctx->stream, l, g->info.as<IngLineInfo>());
            std::vector<IngLineInfo> info(nl);
            std::vector<uint64_t> pos(n_nl), hh(nl + 2, 0), sl(nl + 2, 0);
            if (nl) CK(hipMemcpyAsync(info.data(), g->info.p, nl * sizeof(IngLineInfo), hipMemcpyDeviceToHost, ctx->stream));
            if (n_nl) CK(hipMemcpyAsync(pos.data(), g->nl_pos.p, n_nl * 8, hipMemcpyDeviceToHost, ctx->stream));
            CK(hipStreamSynchronize(ctx->stream));
            enum { SKIP, SEQ, QUAL } st = SKIP;
            uint64_t rec_line = 0, seq_l = 0, qual_l = 0, n_done = 0, cut = nl;      // cut: first line that does not belong to a finished record
            bool bad = false, open = false;             // open: a record has begun and is not finished
            std::vector<uint64_t> rec_lines;            // header lines of finished records
            const uint64_t nlw = final? nl : n_nl;      // a last line without its newline may go on in the next chunk: not looked at yet
            for (uint64_t i = 0; i < nlw && !bad; ++i) {
                const IngLineInfo &x = info[i];
                const bool hdr_char = x.len && (x.c0 == '>' || x.c0 == '@');
                if (st == SKIP) {
                    if (hdr_char) { st = SEQ, open = true, rec_line = i, seq_l = 0; }
                    else if (x.mid) bad = true;                                     // a header character in the middle of skipped text
                } else if (st == SEQ) {
                    if (x.len == 0) continue;                                       // kseq.h:208: empty lines are skipped
                    if (hdr_char) { rec_lines.push_back(rec_line), ++n_done; rec_line = i, seq_l = 0; }      // FASTA record done; the next one begins
                    else if (x.c0 == '+') st = QUAL, qual_l = 0;                    // the rest of the '+' line is skipped (:224)
                    else sl[i] = x.len, seq_l += x.len;
                } else {                                                            // quality: whole lines until it is as long as the sequence (:226)
                    qual_l += x.len;
                    if (qual_l >= seq_l) {
                        if (qual_l != seq_l) { bad = true; break; }                 // kseq returns -2: the reference's reader stops at this file
                        rec_lines.push_back(rec_line), ++n_done;
                        st = SKIP, open = false;
                    }
                }
            }
            if (bad) { ctx->err = "oatk_hip_ingest: text kseq would not read to the end (a quality string longer than its sequence, or a header character inside skipped text)"; return OATK_E_ARG; }
            if (final) {
                if (open && st == SEQ) rec_lines.push_back(rec_line), ++n_done, open = false;      // the last FASTA record ends with the text
                else if (open) { ctx->err = "oatk_hip_ingest: the text ends inside a quality string"; return OATK_E_ARG; }
                cut = nl;
            } else {
                cut = open? rec_line : nlw;             // an unfinished record goes to the next chunk whole
            }
            for (uint64_t t = 0; t < rec_lines.size(); ++t) hh[rec_lines[t]] = 1;
            for (uint64_t i = cut; i < nl; ++i) sl[i] = 0;
            n_hdr = n_done, line_end = cut, cut_done = true;
            used = cut == 0? 0 : (cut - 1 < n_nl? pos[cut - 1] + 1 : n_bytes);
            CK(hipMemcpyAsync(g->is_hdr.p, hh.data(), (nl + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
            CK(hipMemcpyAsync(g->seq_len.p, sl.data(), (nl + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
            CK(hipStreamSynchronize(ctx->stream));      // (the vectors go out of scope)
        } else {
            hipLaunchKernelGGL(ing_line_kernel, grid256(nl + 1), dim3(256), 0, ctx->stream, l, g->is_hdr.as<uint64_t>(), g->seq_len.as<uint64_t>(), g->flags.as<uint32_t>());
        }
        PRIM(rocprim::exclusive_scan, g->is_hdr.as<const uint64_t>(), g->hdr_rank.as<uint64_t>(), (uint64_t) 0, nl + 1, rocprim::plus<uint64_t>(), ctx->stream);
        PRIM(rocprim::exclusive_scan, g->seq_len.as<const uint64_t>(), g->seq_before.as<uint64_t>(), (uint64_t) 0, nl + 1, rocprim::plus<uint64_t>(), ctx->stream);
        if (!cut_done) {
            CK(hipMemcpyAsync(&n_hdr, g->hdr_rank.as<uint64_t>() + nl, 8, hipMemcpyDeviceToHost, ctx->stream));
            CK(hipStreamSynchronize(ctx->stream));
        }
        GENSURE(hdr_line, (n_hdr + 2) * 8);
        hipLaunchKernelGGL(ing_hdr_lines_kernel, grid256(nl), dim3(256), 0, ctx->stream, nl, g->is_hdr.as<uint64_t>(), g->hdr_rank.as<uint64_t>(), g->hdr_line.as<uint64_t>());
        CK(hipMemcpyAsync(g->hdr_line.as<uint64_t>() + n_hdr, &line_end, 8, hipMemcpyHostToDevice, ctx->stream));      // sentinel: end of the last record
        CK(hipStreamSynchronize(ctx->stream));          // (line_end lives on this stack frame)
        n_rec = n_hdr;
        if (cut_done) {
            // nothing: the walk has counted only finished records
        } else if (!final && n_hdr) {                   // the last record may continue in the next chunk: leave it
            n_rec = n_hdr - 1;
            uint64_t hl = 0;
            CK(hipMemcpyAsync(&hl, g->hdr_line.as<uint64_t>() + n_rec, 8, hipMemcpyDeviceToHost, ctx->stream));
            CK(hipStreamSynchronize(ctx->stream));
            line_end = hl;
            uint64_t pos = 0;
            if (hl) {
                CK(hipMemcpyAsync(&pos, g->nl_pos.as<uint64_t>() + hl - 1, 8, hipMemcpyDeviceToHost, ctx->stream));
                CK(hipStreamSynchronize(ctx->stream));
                pos += 1;
            }
            used = pos;
        } else if (!final) {
            used = 0;
        }
        GENSURE(len, (n_rec + 1) * 4); GENSURE(padded, (n_rec + 2) * 8); GENSURE(off, (n_rec + 2) * 8); GENSURE(hdr_off, (n_rec + 1) * 8);
        hipLaunchKernelGGL(ing_record_kernel, grid256(n_rec + 1), dim3(256), 0, ctx->stream, l, n_rec, g->hdr_line.as<uint64_t>(), g->seq_before.as<uint64_t>(),
                           g->len.as<uint32_t>(), g->padded.as<uint64_t>(), g->hdr_off.as<uint64_t>(), g->flags.as<uint32_t>());
        PRIM(rocprim::exclusive_scan, g->padded.as<const uint64_t>(), g->off.as<uint64_t>(), (uint64_t) 0, n_rec + 1, rocprim::plus<uint64_t>(), ctx->stream);
        uint64_t seq_bytes = 0;
        CK(hipMemcpyAsync(&seq_bytes, g->off.as<uint64_t>() + n_rec, 8, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        GENSURE(seq, seq_bytes + 64);
        if (n_rec && line_end) hipLaunchKernelGGL(ing_copy_fasta_kernel, dim3((unsigned) ((line_end + 3) / 4)), dim3(256), 0, ctx->stream, l, line_end,
                                                  g->is_hdr.as<uint64_t>(), g->seq_len.as<uint64_t>(), g->hdr_rank.as<uint64_t>(), g->hdr_line.as<uint64_t>(), g->seq_before.as<uint64_t>(),
                                                  g->off.as<uint64_t>(), g->seq.as<uint8_t>());
        g->seq_bytes = seq_bytes;
    } else {
        const uint64_t whole = final? nl : n_nl;        // lines that are certainly complete
        n_rec = whole / 4;
        if (final && nl % 4)                            // up to three lines behind the last whole record: blank, or the input is truncated
            hipLaunchKernelGGL(ing_fastq_leftover_kernel, dim3(1), dim3(4), 0, ctx->stream, l, 4 * n_rec, g->flags.as<uint32_t>());
        if (!final) {
            uint64_t pos = 0;
            if (n_rec) {
                CK(hipMemcpyAsync(&pos, g->nl_pos.as<uint64_t>() + 4 * n_rec - 1, 8, hipMemcpyDeviceToHost, ctx->stream));
                CK(hipStreamSynchronize(ctx->stream));
                pos += 1;
            }
            used = pos;
        }
        GENSURE(len, (n_rec + 1) * 4); GENSURE(padded, (n_rec + 2) * 8); GENSURE(off, (n_rec + 2) * 8); GENSURE(hdr_off, (n_rec + 1) * 8);
        hipLaunchKernelGGL(ing_fastq_record_kernel, grid256(n_rec + 1), dim3(256), 0, ctx->stream, l, n_rec, g->len.as<uint32_t>(), g->padded.as<uint64_t>(),
                           g->hdr_off.as<uint64_t>(), g->flags.as<uint32_t>());
        PRIM(rocprim::exclusive_scan, g->padded.as<const uint64_t>(), g->off.as<uint64_t>(), (uint64_t) 0, n_rec + 1, rocprim::plus<uint64_t>(), ctx->stream);
        uint64_t seq_bytes = 0;
        CK(hipMemcpyAsync(&seq_bytes, g->off.as<uint64_t>() + n_rec, 8, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        GENSURE(seq, seq_bytes + 64);
        if (n_rec) hipLaunchKernelGGL(ing_copy_fastq_kernel, dim3((unsigned) ((n_rec + 3) / 4)), dim3(256), 0, ctx->stream, l, n_rec, g->off.as<uint64_t>(), g->seq.as<uint8_t>());
        g->seq_bytes = seq_bytes;
    }
    uint32_t fl[4] = {0, 0, 0, 0};
    CK(hipMemcpyAsync(fl, g->flags.p, sizeof(fl), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    if (fl[0]) { ctx->err = "oatk_hip_ingest: a read longer than 2^32 bases"; return OATK_E_ARG; }
    if (fl[1]) { ctx->err = "oatk_hip_ingest: not four-line FASTQ ('@' header, sequence, '+', quality of equal length): OATK_FMT_KSEQ reads it line by line"; return OATK_E_SPLIT; }
    if (fl[2]) { ctx->err = "oatk_hip_ingest: a '+' line inside FASTA text (FASTQ records among FASTA ones): OATK_FMT_KSEQ reads it line by line"; return OATK_E_SPLIT; }
    if (n_rec >= 0xFFFFFFFFULL) { ctx->err = "oatk_hip_ingest: more than 2^32 reads in one chunk"; return OATK_E_ARG; }
    g->n_reads = n_rec, g->done = true;
    if (n_reads) *n_reads = n_rec;
    if (consumed) *consumed = used;
    return OATK_OK;
}

// sr_read's data cap (syncmer.c:537-541): only the first n_keep reads of the resident packed stream take part in what follows
extern "C" int oatk_hip_ingest_truncate(oatk_hip_ctx *ctx, uint64_t n_keep)
{
    if (!ctx) return OATK_E_NODEV;
    IngState *g = ctx->ing;
    if (!g || !g->done) { ctx->err = "oatk_hip_ingest_truncate needs oatk_hip_ingest"; return OATK_E_STATE; }
    if (n_keep >= g->n_reads) return OATK_OK;
    CK(hipSetDevice(ctx->device));
    uint64_t sb = 0;
    CK(hipMemcpyAsync(&sb, g->off.as<uint64_t>() + n_keep, 8, hipMemcpyDeviceToHost, ctx->stream));      // off[] has n_reads + 1 entries: where read n_keep starts
    CK(hipStreamSynchronize(ctx->stream));
    g->n_reads = n_keep, g->seq_bytes = sb;
    return OATK_OK;
}

extern "C" int oatk_hip_ingest_text_buffer(oatk_hip_ctx *ctx, uint64_t n_bytes, uint8_t **d_text)
{
    if (!ctx) return OATK_E_NODEV;
    CK(hipSetDevice(ctx->device));
    if (!ctx->ing) ctx->ing = new IngState();
    IngState *g = ctx->ing;
    GENSURE(text, n_bytes + 64);
    *d_text = g->text.as<uint8_t>();
    return OATK_OK;
}

extern "C" int oatk_hip_ingest_host(oatk_hip_ctx *ctx, const uint8_t *h_text, uint64_t n_bytes, int format, int final, uint64_t *n_reads, uint64_t *consumed)
{
    if (!ctx) return OATK_E_NODEV;
    CK(hipSetDevice(ctx->device));
    if (!ctx->ing) ctx->ing = new IngState();
    IngState *g = ctx->ing;
    GENSURE(text, n_bytes + 64);
    if (n_bytes) CK(hipMemcpyAsync(g->text.p, h_text, n_bytes, hipMemcpyHostToDevice, ctx->stream));
    return oatk_hip_ingest(ctx, g->text.as<uint8_t>(), n_bytes, format, final, n_reads, consumed);
}

extern "C" int oatk_hip_scan_ingested(oatk_hip_ctx *ctx, uint64_t sid0, int k, int s)
{
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->ing || !ctx->ing->done) { ctx->err = "oatk_hip_scan_ingested needs oatk_hip_ingest"; return OATK_E_STATE; }
    IngState *g = ctx->ing;
    return oatk_hip_scan(ctx, g->seq.as<uint8_t>(), g->off.as<uint64_t>(), g->len.as<uint32_t>(), g->n_reads, g->seq_bytes, sid0, k, s);
}
