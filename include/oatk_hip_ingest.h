/*
 * include/oatk_hip_ingest.h -- C ABI of the device-side FASTA / FASTQ record scan (the reader loop of sr_read, syncmer.c:522-543,
 * over sstream_read -> kseq_read, sstream.c:83-103, kseq.h:192-235).
 *
 * The reference parses on one thread (kseq + strdup per read) and that bounds it: 0.4 Gbases/s whether it runs 8 or 128 analysis
 * threads.  Here the TEXT of the file goes to the device as it is (PCIe is ~100x faster than kseq) and the records are found there:
 * newline positions, header lines, per-record sequence lengths by prefix sums, and one copy pass that leaves the packed read stream
 * oatk_hip_scan takes (sequence bytes only, every read on a 64-byte boundary) in HBM -- the host never touches a base.
 *
 * Accepted text (kseq's reading of it, restricted to what sequencing files look like):
 *   FASTA   a header line starts with '>' (kseq also takes '@'); the sequence is every following line up to the next header, line
 *           breaks removed ("\n" or "\r\n"), empty lines skipped; text before the first header is ignored
 *   FASTQ   four lines per record: '@' header, sequence, '+' line, quality of the same length (the form every sequencer writes)
 *   KSEQ    anything kseq reads with headers at line starts: wrapped FASTQ, FASTA and FASTQ records in one stream (OATK_FMT_KSEQ below)
 * Read names are not kept on the device (sr_t.sname is only ever printed): OATK_BUF_INGEST_HDR gives the header-line offsets for a
 * caller that wants them.  gzip'ed input: a DEFLATE stream is serial on any hardware, but a BGZF file (bgzip) is a hundred thousand independent
 * streams of at most 64 KiB -- oatk_hip_inflate_bgzf below inflates those on the device, one wave per member, so that the compressed bytes cross the
 * bus and the text first exists where oatk_hip_ingest wants it.  A plain gzip member (one stream) must still be inflated by the caller.
 */
#ifndef OATK_HIP_INGEST_H
#define OATK_HIP_INGEST_H

#include "oatk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OATK_FMT_AUTO 0           /* by the first non-blank character: '>' FASTA, '@' FASTQ */
#define OATK_FMT_FASTA 1
#define OATK_FMT_FASTQ 2
#define OATK_FMT_KSEQ 3           /* kseq_read's own reading, line by line (kseq.h:192-235): every record FASTA or FASTQ by whether a '+' line follows its
                                   * sequence, sequence AND quality over any number of lines (a quality line may start with '@').  The two formats above
                                   * are what sequencing files look like and run entirely on the device; they answer OATK_E_SPLIT for text that needs
                                   * this one (FASTQ that is not four lines per record; a '+' line in FASTA text).  Here the device extracts three numbers per
                                   * line and the classification -- inherently serial: what a line is depends on the lines before it -- is a walk over them on
                                   * the host; lengths, offsets and the copy stay on the device.  Headers must begin a line. */

/* Parse n_bytes of text resident in device memory.  final = 0: the text is a chunk of a longer file -- only records that are certainly
 * complete are taken and *consumed tells how many bytes they span (feed the rest again in front of the next chunk); final = 1: the
 * text ends the file.  The packed stream stays resident (OATK_BUF_INGEST_*) until the next ingest. */
int oatk_hip_ingest(oatk_hip_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, int format, int final, uint64_t *n_reads, uint64_t *consumed);
/* the same from host memory (one hipMemcpy first) */
int oatk_hip_ingest_host(oatk_hip_ctx *ctx, const uint8_t *h_text, uint64_t n_bytes, int format, int final, uint64_t *n_reads, uint64_t *consumed);
/* sr_read's data cap (-D; syncmer.c:537-541: the read that takes the total to the cap is the last one): keep only the first n_keep reads of the
 * resident packed stream */
int oatk_hip_ingest_truncate(oatk_hip_ctx *ctx, uint64_t n_keep);
/* device memory owned by the context for n_bytes of text (valid until the next call or the next oatk_hip_ingest_host): a caller that uploads the
 * text itself -- in pieces, through page-locked memory, while it is still reading the file -- fills it with oatk_hip_h2d_async and then calls
 * oatk_hip_ingest on it */
int oatk_hip_ingest_text_buffer(oatk_hip_ctx *ctx, uint64_t n_bytes, uint8_t **d_text);
/* oatk_hip_scan on the resident packed stream: reads are numbered sid0, sid0 + 1, ... in file order (syncmer.c:525) */
int oatk_hip_scan_ingested(oatk_hip_ctx *ctx, uint64_t sid0, int k, int s);

/* ---- BGZF members inflated on the device (oatk_amd/csrc/inflate.hpp) ----
 * in_off / in_len: the raw deflate stream of the member inside d_comp (gzip header and 8-byte trailer excluded); out_off / out_len: its place in d_text
 * (out_len is the trailer's ISIZE); crc: the trailer's CRC-32.  oatk_bgzf_index (include/oatk_inflate.h) makes such a table from the bytes of a file. */
typedef struct { uint64_t in_off; uint32_t in_len, out_len; uint64_t out_off; uint32_t crc, pad; } oatk_bgzf_member_t;

#define OATK_INF_OK 0             /* status of a member: its text is in place, as long as its trailer says and with the trailer's CRC-32 */
#define OATK_INF_STREAM 1         /* not a DEFLATE stream this decoder takes: ends early, bytes behind the final block, a bad code set, a distance that reaches
                                   * before the member's first byte, block type 3, LEN != ~NLEN ... (it may refuse what zlib accepts: an incomplete code set) */
#define OATK_INF_LENGTH 2         /* the stream holds more or less text than out_len */
#define OATK_INF_CRC 3            /* the text's CRC-32 is not the member's */

/* Inflate n members on the context's stream.  The table is checked on the host first -- every member inside comp_bytes, in_len and out_len <= 65536, outputs
 * ascending, disjoint and inside text_cap: OATK_E_ARG otherwise, nothing launched.  OATK_OK means the call ran, whatever *n_bad (members with a status other than 0;
 * h_status, n bytes, may be NULL) says: what a bad member means is the caller's decision.  Nothing outside the members' own output ranges is written; the range of a
 * member with status 1 or 2 is left as it was.  The call returns when the text, the statuses and the count are complete. */
int oatk_hip_inflate_bgzf(oatk_hip_ctx *ctx, const uint8_t *d_comp, uint64_t comp_bytes, const oatk_bgzf_member_t *h_members, uint64_t n,
                          uint8_t *d_text, uint64_t text_cap, uint64_t *n_bad, uint8_t *h_status);
/* the same with the compressed bytes in host memory (one upload first) */
int oatk_hip_inflate_bgzf_host(oatk_hip_ctx *ctx, const uint8_t *h_comp, uint64_t comp_bytes, const oatk_bgzf_member_t *h_members, uint64_t n,
                               uint8_t *d_text, uint64_t text_cap, uint64_t *n_bad, uint8_t *h_status);
/* the last byte of the text the context's latest oatk_hip_inflate_bgzf produced (0: none): kseq gives a file that ends without a newline one */
int oatk_hip_inflate_last_byte(oatk_hip_ctx *ctx);

/* The names of the records the context's latest oatk_hip_ingest found (after oatk_hip_ingest_truncate: of those kept), cut out of the text ON THE DEVICE -- for text
 * that has no copy on the host, such as a window inflated there.  d_text / n_bytes: the text that ingest was given.  A name is what follows the header character up
 * to the first space, tab, CR or LF, or the end of the text.  *h_off: n + 1 offsets into *h_packed, the names back to back without terminators; both lie in host
 * memory owned by the context, valid until its next call. */
int oatk_hip_ingest_names(oatk_hip_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, const uint8_t **h_packed, const uint64_t **h_off, uint64_t *n_names);

/* ---- unaligned BAM (PacBio's *.hifi_reads.bam) read on the device (oatk_amd/csrc/bam.hpp) ----
 * d_bam: n_bytes of the INFLATED stream (BAM is a BGZF container: oatk_hip_inflate_bgzf above), at any byte alignment.  header = 1: the bytes begin with the BAM
 * header ("BAM\1", text, reference list), which is walked on the host over a copy of the chunk's head; a wrong magic or a negative length is OATK_E_ARG, a header
 * that is not whole inside the chunk gives OATK_OK with *n_reads = 0 and *consumed = 0 when final = 0 (come back with more) and OATK_E_ARG when final = 1.
 * The records are found on the device: every byte offset that passes the record check is a candidate, and the chain of records from the first byte behind the
 * header is the set of candidates reachable from it -- found by pointer doubling, not by a walk (oatk_amd/csrc/bam.hpp).  The chain stops at the end of
 * the chunk (all taken), inside a record (final = 0: *consumed is that record's offset, feed the rest again in front of the next chunk; final = 1: OATK_E_ARG,
 * "BAM stream ends inside a record"), or at bytes that are no record (OATK_E_ARG with the offset).  *consumed counts from the chunk's first byte, header included.
 * A record with flag & 0x910 (reverse-complemented, secondary, supplementary) is one samtools fasta would reverse or drop: the whole input is refused with
 * OATK_E_SPLIT and the record named.  n_cigar_op need not be 0; quality and tags are never read; l_seq = 0 is a read of length 0.
 * A read is its l_seq letters of "=ACMGRSVTWYHKDBN", what samtools fasta prints.  On success the packed stream is resident exactly as oatk_hip_ingest leaves it
 * (OATK_BUF_INGEST_*; INGEST_HDR: the byte offset of each record's block_size), and oatk_hip_scan_ingested, oatk_hip_ingest_truncate and oatk_hip_ingest_names
 * (a name: the bytes at INGEST_HDR + 36 up to the first NUL) work on it.  On any error nothing is resident. */
int oatk_hip_ingest_bam(oatk_hip_ctx *ctx, const uint8_t *d_bam, uint64_t n_bytes, int header, int final, uint64_t *n_reads, uint64_t *consumed);
/* the same from host memory (one hipMemcpy first, into the context's text buffer: that is the d_text oatk_hip_ingest_names wants afterwards) */
int oatk_hip_ingest_bam_host(oatk_hip_ctx *ctx, const uint8_t *h_bam, uint64_t n_bytes, int header, int final, uint64_t *n_reads, uint64_t *consumed);
/* candidates, records, header bytes of the latest oatk_hip_ingest_bam */
int oatk_hip_ingest_bam_stats(oatk_hip_ctx *ctx, uint64_t out[3]);
/* milliseconds of the phases of the latest oatk_hip_ingest_bam, if it ran with oatk_hip_set_timing on (zeros otherwise): candidate passes, successors + doubling
 * rounds, compaction + stop, record kernel + offsets scan, unpack kernel (tests/bam_time.py) */
int oatk_hip_ingest_bam_times(oatk_hip_ctx *ctx, float ms[5]);

/* INGEST_SEQ u8[seq_bytes]  INGEST_OFF u64[n_reads]  INGEST_LEN u32[n_reads]  INGEST_HDR u64[n_reads] byte offset of each header line */
enum { OATK_BUF_INGEST_SEQ = 160, OATK_BUF_INGEST_OFF, OATK_BUF_INGEST_LEN, OATK_BUF_INGEST_HDR };

#ifdef __cplusplus
}
#endif
#endif
