/*
 * oatk_amd/csrc/host/host_internal.h -- the second halves of the host adaptors (include/oatk_syncasm.h), shared between the one-handle entry
 * points and the N-handle ones of multi_host.c (include/oatk_multi.h): each adaptor is "run the device step, then turn what is resident into the
 * reference's structs"; with reads sharded over several handles the device step is a collective and the second half is the same.
 */
#ifndef OATK_HOST_INTERNAL_H
#define OATK_HOST_INTERNAL_H

#include <stdio.h>

#include "oatk_hip_cons.h"
#include "oatk_hip_racov.h"
#include "oatk_inflate.h"
#include "oatk_hip_stat.h"
#include "oatk_syncasm.h"

/* syncmer_db_t from the flat table (collect_syncmer_from_reads, syncmer.c:1419-1444) and every read's k_mer rewritten from `kid` (all reads' ids in
 * read order, :1378).  With arenas `occ` becomes the table's storage (adopted); everything else stays the caller's. */
oatk_syncmer_db_t *oatk_host_build_syncmer_db(oatk_sr_db_t *sr_db, uint64_t n_scm, uint64_t n_occ, const uint64_t *h, const uint64_t *s, const uint32_t *cov,
                                              const uint64_t *occ_off, uint64_t **occ, const uint64_t *kid);
/* what read_error_correction leaves in the reads (syncerr.c:600-612) and update_syncmer_db in the table (:769-814), from flat arrays: new_n per read,
 * chains concatenated in read order, the refreshed table.  With arenas the chain arrays and `occ` are adopted (the pointers are cleared). */
void oatk_host_ec_write_back(oatk_sr_db_t *sr_db, oatk_syncmer_db_t *scm_db, const uint32_t *new_n, uint64_t **new_k, uint32_t **new_m, uint64_t **new_s,
                             const uint32_t *cov, const uint8_t *del, const uint64_t *occ_off, uint64_t **occ);
/* ">name\nSEQ\n" of the corrected sequences (read_error_correction's FILE *fo, syncerr.c:614-624) of the reads ctx holds, after a correction made with
 * oatk_hip_ec_keep_seq: the handle's reads 0 .. count are sr_db->a[first .. first + count) (one handle: 0, sr_db->n).  Only the names are read from sr_db. */
int oatk_host_ec_write_sequences(oatk_hip_ctx *ctx, const oatk_sr_db_t *sr_db, uint64_t first, uint64_t count, FILE *fo);
/* asmg_t from the graph resident in ctx (OATK_BUF_AG_*), scm_db->a[i].del updated like syncasm.c:228 */
oatk_asmg_t *oatk_host_asmg_from_resident(oatk_hip_ctx *ctx, oatk_syncmer_db_t *scm_db, uint64_t nv, uint64_t na, int *rc);
oatk_consensus_t *oatk_host_consensus_from_resident(oatk_hip_ctx *ctx, int k, int *rc);
oatk_overlap_t *oatk_host_overlap_from_resident(oatk_hip_ctx *ctx, uint64_t n_pairs, uint64_t n_entries, int *rc);
/* sr_db_stat's arithmetic, report and sr_db->stats from the raw tabulation */
int oatk_host_stat_report(oatk_sr_db_t *sr_db, const oatk_stat_raw_t *raw, FILE *fo);
/* scg_read_alignment with the reads spread over n handles: handle r holds reads [first[r], first[r + 1]) */
int oatk_host_read_alignment_n(oatk_hip_ctx **ctx, const uint64_t *first, int n, oatk_sr_db_t *sr_db, oatk_scg_ra_v *ra_v, oatk_scg_t *g, int for_unzip,
                               uint64_t *n_skipped, uint32_t **skipped);
/* sr_read (syncmer.c:487) for files with the reads spread over n handles by position in the input: first[0 .. n] receives the read ranges */
int oatk_host_sr_read_files_n(oatk_hip_ctx **ctx, int n, oatk_sr_db_t *sr_db, char **files, int n_files, uint64_t *first, uint64_t m_data);
/* host/racov_host.c for host/multi_host.c: scg_t flattened into what include/oatk_hip_racov.h reads (free with oatk_host_racov_graph_free(keep)), and the
 * reference's write-back of the doubles into vtx[].cov / the live arcs' cov */
const oatk_racov_graph_t *oatk_host_racov_graph(const oatk_scg_t *g, int with_arcs, void **keep);
void oatk_host_racov_graph_free(void *keep);
void oatk_host_racov_write_utg(oatk_scg_t *g, const double *cov);
void oatk_host_racov_write_arc(oatk_scg_t *g, const double *cov);
/* scg_ra_v flattened for an upload (NULL: a value does not fit the device's fields, or a sid is no read); free with oatk_host_racov_aln_free(keep) either way */
const oatk_racov_aln_t *oatk_host_racov_aln(const oatk_scg_ra_v *v, uint64_t n_reads, void **keep);
void oatk_host_racov_aln_free(void *keep);
/* host/multiplex_host.c for host/multi_host.c: how many (in, out) arc pairs scg_multiplex looks up in g, and its decisions (syncasm.c:1181-1302) from their
 * scores in the order of include/oatk_hip_racov.h; tab (may be NULL) receives the entries that exist.  -1: the pairs are not those of g */
uint64_t oatk_host_multiplex_pairs(const oatk_scg_t *g);
int oatk_host_multiplex_decide(const oatk_scg_t *g, const uint64_t *pair_off, const uint64_t *pair_in, const uint64_t *pair_out, const double *score,
                               const uint8_t *have, uint32_t max_n_scm, double min_n_r, double min_d_f, uint8_t *multi_vtx, int *updated, oatk_triplet_table *tab);

/* host/scgcons_host.c split at its one device call, for host/multi_host.c: the plan of scg_consensus over g (NULL with OATK_E_SPLIT / OATK_E_ARG where
 * oatk_scg_consensus declines before the device), the plan as oatk_hip_consensus_strings(_sharded) takes it, and -- after that call, with what it returned -- the
 * strings resident in ctx fetched and the graph and the GFA lines written as the reference writes them; unless it returns OATK_OK, g and fo are untouched */
typedef struct oatk_scgcons_plan oatk_scgcons_plan_t;
oatk_scgcons_plan_t *oatk_host_scgcons_plan(const oatk_overlap_t *o, const oatk_sr_db_t *sr_db, const oatk_scg_t *g, int *rc);
const oatk_cons_plan_t *oatk_host_scgcons_device_plan(const oatk_scgcons_plan_t *sp);
int oatk_host_scgcons_write(oatk_hip_ctx *ctx, const oatk_scgcons_plan_t *sp, uint64_t total, uint64_t refused, oatk_scg_t *g, int save_seq, FILE *fo);
void oatk_host_scgcons_plan_free(oatk_scgcons_plan_t *sp);

typedef struct { uint8_t *p, *end; } oatk_name_bump_t;
char *oatk_host_name_dup(const uint8_t *src, size_t len, oatk_name_bump_t *b, const void *owner);
int oatk_host_threads_granted(void);
void oatk_host_set_threads_internal(int n);

/* a gzip'ed file (one member, several, BGZF) as a stream of inflated bytes (gzsrc.c) */
typedef struct oatk_gzsrc oatk_gzsrc_t;
oatk_gzsrc_t *oatk_gzsrc_open(const char *path, int n_threads, int *rc);
int64_t oatk_gzsrc_read(oatk_gzsrc_t *g, uint8_t *dst, uint64_t cap);
uint64_t oatk_gzsrc_tell_in(const oatk_gzsrc_t *g);
uint64_t oatk_gzsrc_size_in(const oatk_gzsrc_t *g);
uint64_t oatk_gzsrc_members_on_many_threads(const oatk_gzsrc_t *g);      /* (statistics, tests) */
int oatk_gzsrc_kind(const oatk_gzsrc_t *g);          /* 1 plain member(s), 2 BGZF, 3 not a regular file (zlib's gzread) */
void oatk_gzsrc_close(oatk_gzsrc_t *g);
/* the BGZF members at the read position listed for the device inflater, and the position moved past them once their text is in place (gzsrc.c) */
uint64_t oatk_gzsrc_bgzf_peek(oatk_gzsrc_t *g, uint64_t text_cap, uint64_t comp_cap, uint64_t member_cap, oatk_bgzf_member_t *members, uint64_t *text_bytes,
                              uint64_t *comp_bytes, const uint8_t **span);
void oatk_gzsrc_bgzf_skip(oatk_gzsrc_t *g, uint64_t comp_bytes);
/* oatk_gzsrc_read that stops at the end of the member at hand, so that the members behind it can be listed again */
int64_t oatk_gzsrc_read_member(oatk_gzsrc_t *g, uint8_t *dst, uint64_t cap);
/* one member's deflate data inflated on many threads (host/gzpar.c) */
typedef struct oatk_gzpar oatk_gzpar_t;
oatk_gzpar_t *oatk_gzpar_open(const uint8_t *deflate, uint64_t n_in, int n_threads);
int64_t oatk_gzpar_read(oatk_gzpar_t *p, uint8_t *dst, uint64_t cap);
int oatk_gzpar_done(const oatk_gzpar_t *p);
uint64_t oatk_gzpar_in_used(const oatk_gzpar_t *p);
uint32_t oatk_gzpar_crc(const oatk_gzpar_t *p);
uint64_t oatk_gzpar_total(const oatk_gzpar_t *p);
void oatk_gzpar_close(oatk_gzpar_t *p);

#endif
