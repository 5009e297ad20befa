/*
 * include/oatk_hip_racov.h -- C ABI of the coverage estimates from read alignments on the device: scg_ra_utg_coverage (syncasm.c:1882-2065,
 * with make_ma_block / find_lcs :1652-1878 and the EM over the multiple-alignment blocks) and the duplet sums of scg_ra_arc_coverage
 * (:2067-2138, before its refinement).  Results are the reference's doubles before its (uint32_t) casts; the host adaptor
 * (include/oatk_syncasm.h: oatk_scg_ra_utg_coverage / oatk_scg_ra_arc_coverage) writes them into the graph.
 *
 * The alignments are the resident ones of the last oatk_hip_read_alignment (aln == NULL) or uploaded; the reads' chains are the resident
 * batch's (reads == NULL; after oatk_hip_ec: the corrected chains) or uploaded.  The graph is passed in, flattened, HOST pointers.
 *
 * Both estimates exist for one handle holding all reads and, as collectives over an oatk_comm (include/oatk_hip_multi.h), for reads sharded
 * by record over several handles: the *_sharded entry points below return, on every rank, the doubles the one-handle call returns.
 */
#ifndef OATK_HIP_RACOV_H
#define OATK_HIP_RACOV_H

#include "oatk_hip.h"
#include "oatk_hip_multi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint64_t n_scm, n_utg, n_arc;
    const uint64_t *su_off;    /* [n_scm + 1] scg->idx_u as offsets (as in oatk_ra_graph_t)                                         */
    const uint64_t *su_uid;    /* [su_off[n_scm]] unitig << 1 | strand                                                             */
    const uint32_t *su_pos;    /*                 position on the unitig                                                           */
    const uint32_t *scm_cov;   /* [n_scm] syncmer_t.cov                                                                            */
    const uint64_t *utg_off;   /* [n_utg + 1] offsets of the unitigs' syncmer lists; utg_off[i + 1] - utg_off[i] = vtx[i].n         */
    const uint64_t *utg_a;     /* [utg_off[n_utg]] vtx[].a back to back                                                            */
    const uint64_t *idx_p;     /* [2 n_utg] asmg_t.idx_p / idx_n (arc coverage only; may be NULL for the unitig coverage)          */
    const uint64_t *idx_n;
    const uint64_t *arc_v;     /* [n_arc] asmg_arc_t.v, .w, .link_id, .comp, .del in array order (arc coverage only)                */
    const uint64_t *arc_w;
    const uint64_t *arc_link;
    const uint8_t *arc_comp;
    const uint8_t *arc_del;
    const uint8_t *vtx_del;    /* [n_utg] asmg_vtx_t.del (the triplet scores only; NULL = no unitig is deleted; the coverage calls never read it) */
} oatk_racov_graph_t;

/* uploaded alignments: scg_ra_v flattened in its order (sid = index of the read's chain) */
typedef struct {
    uint64_t n_aln, n_frg;
    const uint32_t *sid;       /* [n_aln]                                                                                           */
    const uint64_t *off;       /* [n_aln + 1] fragments of alignment i                                                             */
    const double *s;           /* [n_aln]                                                                                           */
    const uint64_t *uid;       /* [n_frg] ra_frg_t.uid, u_beg, u_end, s_beg, s_end                                                 */
    const uint32_t *u_beg, *u_end, *s_beg, *s_end;
} oatk_racov_aln_t;

/* uploaded chains: the reads' k_mer arrays back to back (syncmer id << 1 | flag) */
typedef struct {
    uint64_t n_reads;
    const uint64_t *off;       /* [n_reads + 1]                                                                                     */
    const uint64_t *k_mer;
} oatk_racov_reads_t;

/* utg_cov[n_utg]: avg_covs after the third round and MAX(1., .) (:2040-2044); *n_iter: the `i` of the EM's "ended at iteration" line.
 * verbose > 2 prints the reference's EM lines to stderr.  With no alignment nothing is written (the caller prints the reference's warning).
 * OATK_E_SPLIT: make_ma_block's LCS matrices of this input would take more than the working limit (oatk_hip_debug_racov_cap); nothing is
 * written and the caller runs the original.  OATK_E_ARG: an alignment that does not fit the graph (the reference would read out of bounds). */
int oatk_hip_ra_utg_coverage(oatk_hip_ctx *ctx, const oatk_racov_graph_t *g, const oatk_racov_reads_t *reads, const oatk_racov_aln_t *aln,
                             int verbose, double *utg_cov, uint64_t *n_iter);

/* arc_cov[n_arc]: for every arc that is not deleted, the spanning-duplet sum of its key link_id << 1 | comp, 0 when it has none
 * (:2131-2137 before the (uint32_t)); deleted arcs get 0.  OATK_E_ARG when two consecutive fragments have no arc (asmg_arc == NULL). */
int oatk_hip_ra_arc_coverage(oatk_hip_ctx *ctx, const oatk_racov_graph_t *g, const oatk_racov_aln_t *aln, double *arc_cov);

/* The same two estimates with the reads SHARDED BY RECORD: every rank makes the same call with the same graph (global syncmer ids); rank r
 * holds a contiguous range of the reads, rank order is read order.  aln == NULL: the handle's resident alignments of its last
 * oatk_hip_read_alignment; reads == NULL: its resident chains from the source that alignment used -- after oatk_hip_ec_sharded the
 * corrected chains in global ids (what the one-handle call refuses to serve).  Non-NULL reads / aln are THIS RANK'S slice, uploaded: sid
 * indexes the slice's own chains, records in the order of the whole set.  A rank without alignments still takes part.
 *
 * Results are identical on every rank and equal, double for double, what the one-handle call returns for all reads; no sum is
 * re-associated:
 *   first round   the per-position counts are integers: one all-reduce of u32[utg_off[n_utg]], then the same IQR code on every rank
 *   make_ma_block per read, local; the working limit (OATK_E_SPLIT, oatk_hip_debug_racov_cap) applies per rank, and the ranks agree on
 *                 the verdict before anything is written: one rank over the limit, OATK_E_SPLIT on all
 *   EM            a unitig's sum takes its addends in (read, block, member) order and the shards are consecutive stretches of it: rank r
 *                 starts every sum from rank r - 1's result and hands its own on; the last rank's n_utg sums go to everybody, the update
 *                 and diff run on every rank alike, all leave at the same iteration.  n_utg doubles per rank and iteration, whatever
 *                 the number of reads.  verbose > 2: rank 0 prints the reference's lines
 *   third round   the graph and the averages only: every rank computes it
 *   arc duplets   per link, a rank's events are a stretch of the reference's put order: the table (seen flags and values of both keys of
 *                 every link, 18 bytes per link) is handed from rank to rank and the last rank's goes to everybody.  A missing arc on any
 *                 rank is OATK_E_ARG on all
 * If no rank has an alignment the unitig call writes nothing.  A rank that fails between two collectives poisons the group like the
 * other sharded calls do.  The one-handle entry points run the same kernels with zero carries and no collective. */
int oatk_hip_ra_utg_coverage_sharded(oatk_hip_ctx *ctx, oatk_comm *comm, const oatk_racov_graph_t *g, const oatk_racov_reads_t *reads,
                                     const oatk_racov_aln_t *aln, int verbose, double *utg_cov, uint64_t *n_iter);
int oatk_hip_ra_arc_coverage_sharded(oatk_hip_ctx *ctx, oatk_comm *comm, const oatk_racov_graph_t *g, const oatk_racov_aln_t *aln, double *arc_cov);

/* ---- the spanning-triplet table of scg_multiplex (syncasm.c:1110-1166) and its lookups (:1181-1255) ----
 * The PAIRS are what the reference looks up at :1240, in its order: for every unitig i that is not deleted and has live arcs on both
 * sides, s over the live arcs out of i << 1 | 1 in array order (pair_in = asmg_comp_arc_id), inside it t over the live arcs out of i << 1
 * (pair_out = asmg_arc_id).  pair_off[i .. i + 1] delimits unitig i's pairs (empty for the others), *n_pair = pair_off[n_utg].
 * score[p] is the table's double under the key (pair_in[p], pair_out[p]), have[p] == 0 (score[p] = 0) where the reference finds no key
 * and reads .001.  The table is built from the alignments resident in the handle (aln == NULL) or uploaded, by the reference's rules:
 * records of three or more fragments, the unique-syncmer test for records with a fractional score, assignment on a key's first event
 * and addition afterwards, the mirror key beside it, identity by key value.  Every double is bit for bit the reference's.
 *   OATK_E_ARG    two consecutive fragments of a record of three or more fragments have no arc (the reference dereferences NULL), or an
 *                 alignment does not fit the graph, or a link id is 2^32 or more.  Nothing is written.
 *   OATK_E_NOMEM  n_pair_cap is below the number of pairs: *n_pair holds the number needed, nothing else is written.
 * Sharded (reads by record, every rank the same graph, rank order is read order): the table -- for every group of keys that the pairs
 * name, a group being the keys over one unordered pair of link ids, 8 doubles and 8 flags = 72 bytes; at most one group per pair -- is
 * handed from rank to rank as a carry and the last rank's goes to everybody: per rank one small all-gather (the verdict: a missing arc on
 * any rank is OATK_E_ARG on all) and 72 bytes per group, whatever the number of reads.  A rank that fails on its own poisons the group
 * like the other sharded calls.  The one-handle call runs the same kernels with a zero carry and no collective. */
int oatk_hip_ra_triplet_scores(oatk_hip_ctx *ctx, const oatk_racov_graph_t *g, const oatk_racov_aln_t *aln, uint64_t *pair_off, uint64_t n_pair_cap,
                               uint64_t *n_pair, uint64_t *pair_in, uint64_t *pair_out, double *score, uint8_t *have);
int oatk_hip_ra_triplet_scores_sharded(oatk_hip_ctx *ctx, oatk_comm *comm, const oatk_racov_graph_t *g, const oatk_racov_aln_t *aln, uint64_t *pair_off,
                                       uint64_t n_pair_cap, uint64_t *n_pair, uint64_t *pair_in, uint64_t *pair_out, double *score, uint8_t *have);

/* ---- the repeat units of the mini-circle path finder (extract_minicircles_with_anchor, path_finder.c:539-693), one handle ----
 * For every alignment record -- the resident ones (aln == NULL) or uploaded ones, of which only off and uid are read -- the unit the reference's
 * minicircle_analysis_thread finds round the unitig anchor_utg: beg << 33 | end << 1 | rev, or UINT64_MAX when the record has fewer than two
 * fragments on the anchor, two of different orientation, or does not repeat the unit over its whole length (:545-607).  Then the valid records'
 * paths as the reference collects them (:657-671: (uint32_t) uid[beg .. end]; a reverse unit with elements 1 .. nv - 1 reversed and every
 * element ^ 1, so that every path starts with anchor_utg << 1), reduced to the distinct ones in path_cmpfunc order (:620-638, :677-693).
 * Resident afterwards (ids for oatk_hip_buffer), until the next call that succeeds:
 *   MC_UNIT      u64[n_aln]           the unit of every record
 *   MC_PATH_OFF  u64[n_path + 1]      path p is MC_PATH_V[MC_PATH_OFF[p] .. MC_PATH_OFF[p + 1])
 *   MC_PATH_V    u32[n_path_vtx]
 *   MC_PATH_CNT  u64[n_path]          the number of records that gave path p (their sum is *n_valid)
 * n_aln == 0: OATK_OK, all zero.  OATK_E_STATE: aln == NULL and no resident alignment.  OATK_E_ARG: anchor_utg >= 2^31; uploaded offsets that do
 * not ascend from 0 to n_frg; a uid of 2^32 or more inside a unit (the reference truncates it silently); a record of 2^31 fragments or more.
 * Whatever is refused leaves the resident results of the previous call as they were, and the three counts unwritten. */
int oatk_hip_ra_minicircle_units(oatk_hip_ctx *ctx, const oatk_racov_aln_t *aln, uint64_t anchor_utg, uint64_t *n_valid, uint64_t *n_path,
                                 uint64_t *n_path_vtx);
enum { OATK_BUF_MC_UNIT = 250, OATK_BUF_MC_PATH_OFF, OATK_BUF_MC_PATH_V, OATK_BUF_MC_PATH_CNT };
/* device time of the last call's three phases (units; valid records and their paths; distinct paths), ms, between events on the handle's stream,
 * and the number of compare rounds the distinct paths took (1 unless two different paths shared a hash) */
int oatk_hip_ra_minicircle_times(oatk_hip_ctx *ctx, float *ms3, uint64_t *rounds);
/* Test hook: the distinct paths are grouped by the low `bits` of their 64-bit hash only, so that different paths meet in a group; 0 = default (all
 * 64).  Results never depend on it: every member of a group is compared with its head element by element. */
int oatk_hip_debug_mc_hash_bits(oatk_hip_ctx *ctx, unsigned bits);

/* Test hook: the most LCS-matrix cells (4 bytes each) the unitig coverage may hold at once, over all reads; 0 = default (2^31, 8 GiB). */
int oatk_hip_debug_racov_cap(oatk_hip_ctx *ctx, uint64_t cells);

#ifdef __cplusplus
}
#endif
#endif
