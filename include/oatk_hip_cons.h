/*
 * include/oatk_hip_cons.h -- C ABI of the base-space syncmer consensus on the device (scg_syncmer_consensus, syncasm.c:888-1003).
 *
 * Call after oatk_hip_count (reads as scanned) or after oatk_hip_ec (corrected chains: corrected entries are skipped, :958-959).
 * With reads sharded over GPUs the totals of a syncmer are sums over all shards: oatk_hip_consensus_sharded (include/oatk_hip_multi.h) adds them up.
 */
#ifndef OATK_HIP_CONS_H
#define OATK_HIP_CONS_H

#include "oatk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* For every syncmer that is not deleted and has coverage >= min_cov (and >= 1): the rounded mean run length at each of the k hoco
 * positions of its FORWARD k-mer over its uncorrected occurrences -- the `b` of syncasm.c:994 -- their number, and the first of them
 * (whose bases the reference prints, :912-936).  The reverse orientation is the mirror image.  Results stay resident:
 *   CONS_SEL   u32[n_sel]       the syncmer ids, ascending          CONS_SLOT  u32[n_scm]   slot of a syncmer in CONS_SEL, ~0 = not selected
 *   CONS_RL    u32[n_sel * k]   lround(total run length / CONS_MSEQ) per forward position
 *   CONS_MSEQ  u32[n_sel]       occurrences that took part (0: every occurrence was corrected away, the reference prints N's)
 *   CONS_FIRST u64[n_sel]       sid << 32 | idx << 1 | rev of the first of them, ~0 if none */
int oatk_hip_consensus(oatk_hip_ctx *ctx, uint32_t min_cov);

/* The same for a caller-chosen list of syncmer ids (DEVICE pointer, ascending).  With reads sharded over GPUs (oatk_hip_ec_set_global ...
 * oatk_hip_ec_correct done) the ids are global and the results cover THIS shard's occurrences only: add CONS_TOT (u64[n * k], the totals
 * before the division) and CONS_MSEQ over the shards, then round(total / count) is the reference's value; the bases come from the shard
 * of lowest rank whose CONS_FIRST is not ~0 (oatk_amd/multi.py: ShardedEc.consensus). */
int oatk_hip_consensus_ids(oatk_hip_ctx *ctx, const uint32_t *d_ids, uint64_t n);

/* What calc_syncmer_overlap (syncasm.c:477-582) tabulates, for EVERY pair of syncmers adjacent on a read, in one pass over the resident
 * chains (after oatk_hip_ec: the corrected ones, pairs with a corrected member left out as :499 / :511 do).  Per pair, under its canonical
 * key ((v << 32 | w) with v <= w, or the complementary pair's; v, w = syncmer id << 1 | strand): the distinct distances between the two
 * syncmers in the order the reference's walk meets them first, their counts, and whether the walk's last add_ovl_count call was a repeat
 * (a khashl table grows at the call AFTER the insert that filled it, so this decides the final bucket order, khashl.h:199).  Replaying
 * kh_put for the distinct distances in this order -- plus one more put of any of them when the flag is set -- leaves the reference's own
 * table in exactly the state its walk would, so the mode and its tie-break (:558-571) come out identical.
 *   OVL_KEY  u64[n_pairs]  ascending      OVL_OFF u64[n_pairs + 1]      OVL_DIST i32[n_entries]   OVL_CNT u32[n_entries]   OVL_TAIL u8[n_pairs]
 * Returns OATK_E_SPLIT when a pair has more than 64 distinct distances. */
int oatk_hip_overlap_hist(oatk_hip_ctx *ctx, uint64_t *n_pairs, uint64_t *n_entries);
/* With reads sharded over GPUs (after oatk_hip_ec_correct, global ids) the table of a pair is made of all shards' adjacencies: every shard lists its
 * pairs (canonical key -- ~0 for fillers -- and distance, in (read, slot) order; DEVICE pointers), the caller all-gathers both lists in shard
 * order, which is the order of one context holding all reads, and any shard builds the same tables from the whole. */
int oatk_hip_overlap_pairs(oatk_hip_ctx *ctx, const void **d_keys, const void **d_dist, uint64_t *n);
int oatk_hip_overlap_hist_from_pairs(oatk_hip_ctx *ctx, const uint64_t *d_keys, const uint32_t *d_dist, uint64_t n, uint64_t *n_pairs, uint64_t *n_entries);

/* The strings of scg_consensus (syncasm.c:716-823) from the tables oatk_hip_consensus(ctx, min_cov) left resident: the text of every sequence of a plan, where
 * a sequence is a list of pieces (syncmer id << 1 | rev, beg) -- what scg_unitig_consensus (:1004-1046) hands to scg_syncmer_consensus (:888-1001) one after the
 * other -- and a piece reads as that function writes it: max(-beg, 0) letters N, then positions max(beg, 0) .. k - 1 of the oriented k-mer of the syncmer's first
 * uncorrected occurrence, each base 1 + CONS_RL times in base space and once with hoco_seq; N's throughout when CONS_FIRST is ~0.  Only the plan goes to the
 * device and only the text comes back; CONS_RL stays where it is.  Results stay resident:
 *   CONS_STR        u8[total]        ASCII, the sequences back to back
 *   CONS_STR_OFF    u64[n_seq + 1]   where sequence i starts in CONS_STR
 *   CONS_STR_LEN    u64[n_seq]       what scg_unitig_consensus returns, also for a sequence with want_bytes 0; ~0 when refused
 *   CONS_STR_STATUS u8[n_seq]        1: a piece's syncmer has no prepared consensus (CONS_SLOT is ~0); the sequence is refused
 * Length-only and refused sequences take no bytes of CONS_STR; *n_refused counts the refused ones and the call still returns OATK_OK.
 * OATK_E_STATE: no oatk_hip_consensus on the resident batch, or reads sharded over GPUs (oatk_hip_ec_set_global; their form is oatk_hip_consensus_strings_sharded, include/oatk_hip_multi.h).  OATK_E_ARG, nothing launched: the offsets do
 * not ascend from 0 to n_piece, an id is not below the number of syncmers, or a beg is not below k (the reference asserts that). */
typedef struct { uint64_t n_seq, n_piece;
                 const uint64_t *seq_off;     /* [n_seq + 1] pieces of sequence i                      */
                 const uint64_t *piece_v;     /* [n_piece] syncmer id << 1 | rev                       */
                 const int32_t  *piece_beg;   /* [n_piece] < k, may be negative                        */
                 const uint8_t  *want_bytes;  /* [n_seq] 0: length only (arc overlaps), NULL = all 1   */
} oatk_cons_plan_t;                           /* HOST pointers, graph-sized */
int oatk_hip_consensus_strings(oatk_hip_ctx *ctx, const oatk_cons_plan_t *plan, int hoco_seq,
                               uint64_t *total_bytes, uint64_t *n_refused);
/* milliseconds the length kernel and the fill kernel of the last oatk_hip_consensus_strings took (0 unless oatk_hip_set_timing was on), and the pieces of its plan
 * (n_piece may be NULL) */
int oatk_hip_consensus_strings_times(oatk_hip_ctx *ctx, float *ms2, uint64_t *n_piece);

enum { OATK_BUF_CONS_SEL = 140, OATK_BUF_CONS_SLOT, OATK_BUF_CONS_RL, OATK_BUF_CONS_MSEQ, OATK_BUF_CONS_FIRST, OATK_BUF_CONS_TOT,
       OATK_BUF_CONS_STR, OATK_BUF_CONS_STR_OFF, OATK_BUF_CONS_STR_LEN, OATK_BUF_CONS_STR_STATUS };
enum { OATK_BUF_OVL_KEY = 150, OATK_BUF_OVL_OFF, OATK_BUF_OVL_DIST, OATK_BUF_OVL_CNT, OATK_BUF_OVL_TAIL };

#ifdef __cplusplus
}
#endif
#endif
