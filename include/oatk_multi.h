/*
 * include/oatk_multi.h -- the reference's hot-path entry points with the reads spread over SEVERAL MI355X of one node, from one host process.
 *
 * north_star: "Reads shard by record across the 8 GPUs of one node with an RCCL all-reduce over xGMI to merge per-GPU syncmer count tables before
 * graph construction"; SURVEY.md 8e: "Either yields identical syncmer_db_t ... graph construction stays on host rank 0".  This is the host half of
 * that hand-off: an oatk_multi owns one device handle per GPU (include/oatk_hip.h) and one communicator per handle (include/oatk_hip_multi.h); its
 * entry points mirror those of include/oatk_syncasm.h one for one and leave the SAME structs -- one sr_db_t, one syncmer_db_t with every syncmer's
 * occurrences in (sid, idx) order (syncmer.c:1353-1360, syncerr.c:796-805), one asmg_t, one consensus / distance table set, one scg_ra_v -- so the
 * reference's serial tail (unitigging, cleaning, unzipping, GFA) runs on them unchanged; the tail's two coverage estimates from read alignments, whose
 * work grows with the reads, have their N-handle form here too.  Results are bit-identical to one handle holding all reads
 * (tests/test_gpu_cli.py::test_cli_over_several_handles: both GFA files byte-identical with 2 and 4 handles).
 *
 * Who talks to whom: handle r holds the reads of the r-th part of the input (contiguous read ids).  Scan and count are local.  The collectives run on
 * one host thread per handle: over RCCL when every handle sits on its own device (librccl is loaded then, not before), over the in-process group
 * (device-to-device copies) when devices repeat -- which is how a single-GPU box runs 2 - 4 handles in the tests.
 */
#ifndef OATK_MULTI_H
#define OATK_MULTI_H

#include "oatk_hip_multi.h"
#include "oatk_syncasm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct oatk_multi oatk_multi;

/* devices[0 .. n): the ordinal each handle is made on (1 <= n <= 64); NULL when a device is unusable or the communicators cannot be made */
oatk_multi *oatk_multi_create(const int *devices, int n);
void oatk_multi_destroy(oatk_multi *m);
int oatk_multi_size(const oatk_multi *m);
oatk_hip_ctx *oatk_multi_ctx(oatk_multi *m, int rank);
/* reads [first, first + n) of sr_db live in handle `rank` (valid after oatk_multi_sr_read_files) */
void oatk_multi_range(const oatk_multi *m, int rank, uint64_t *first, uint64_t *n);
const char *oatk_multi_backend(const oatk_multi *m);         /* "rccl" or "local" */
const char *oatk_multi_last_error(oatk_multi *m);

/* sr_read (syncmer.c:487): the files' text streams through the devices in windows, consecutive parts of the input to consecutive handles */
int oatk_multi_sr_read_files(oatk_multi *m, oatk_sr_db_t *sr_db, char **files, int n_files);
int oatk_multi_sr_read_files_capped(oatk_multi *m, oatk_sr_db_t *sr_db, char **files, int n_files, uint64_t m_data);      /* with sr_read's data cap (-D), 0 = none */
/* sr_db_stat (syncmer.c:867), after the read and after the correction */
int oatk_multi_sr_db_stat(oatk_multi *m, oatk_sr_db_t *sr_db, FILE *fo, int verbose);
/* collect_syncmer_from_reads (syncmer.c:1397): local counts, the table merge, the table gathered into the reference's struct */
oatk_syncmer_db_t *oatk_multi_collect_syncmer_from_reads(oatk_multi *m, oatk_sr_db_t *sr_db, int *rc);
/* read_error_correction (syncerr.c:819) with the EC graph built on the devices (the asmg == NULL form of oatk_read_error_correction) */
int oatk_multi_read_error_correction(oatk_multi *m, oatk_sr_db_t *sr_db, oatk_syncmer_db_t *scm_db, double max_edist, uint32_t err_mer_c, uint32_t max_err_c,
                                     uint32_t err_arc_c, double max_arc_f, uint64_t *stats12);
/* the same with the reference's FILE *fo (oatk_read_error_correction_fo on one handle): ">name\nSEQ\n" of every read's corrected sequence in hoco space, in
 * sr_db order -- handle after handle, each handle's reads from its own resident correction (oatk_hip_ec_corrected_reads is rank-local) -- byte for byte the
 * reference's file.  oatk_hip_ec_keep_seq is set on every handle for this one call and cleared on every way out.  Order: correction, table gather, every
 * handle's text written, and only then sr_db / scm_db rewritten: any failure (the file included) leaves them as they were.  fo == NULL: no strings are
 * built anywhere, this is oatk_multi_read_error_correction. */
int oatk_multi_read_error_correction_fo(oatk_multi *m, oatk_sr_db_t *sr_db, oatk_syncmer_db_t *scm_db, double max_edist, uint32_t err_mer_c, uint32_t max_err_c,
                                        uint32_t err_arc_c, double max_arc_f, FILE *fo, uint64_t *stats12);
/* make_syncmer_graph(sr_db, scm_db, min_k_cov, min_a_cov_f) of the corrected reads (run_syncasm.c:138) */
oatk_asmg_t *oatk_multi_make_syncmer_asmg(oatk_multi *m, oatk_syncmer_db_t *scm_db, uint32_t min_k_cov, double min_a_cov_f, int *rc);
/* the consensus sums and distance tables behind scg_consensus (include/oatk_syncasm.h: oatk_consensus_fetch / oatk_overlap_fetch); the tables cover
 * the pairs whose two syncmers are alive and seen >= min_cov times -- every pair of neighbours in the graph made with that min_k_cov */
oatk_consensus_t *oatk_multi_consensus_fetch(oatk_multi *m, uint32_t min_cov, int k, int *rc);
oatk_overlap_t *oatk_multi_overlap_fetch(oatk_multi *m, uint32_t min_cov, int *rc);
/* the consensus sums over all handles (oatk_hip_consensus_sharded), left resident: nothing is copied to the host */
int oatk_multi_consensus(oatk_multi *m, uint32_t min_cov);
/* scg_consensus (syncasm.c:716-823) as oatk_scg_consensus (include/oatk_syncasm.h) makes it on one handle, word for word, from the tables oatk_multi_consensus
 * left resident: positions from `o`, one plan for the whole graph, the text made on every handle (oatk_hip_consensus_strings_sharded; the first call after a
 * consensus exchanges the syncmers' own k-mers once, later calls nothing) and fetched from handle 0 -- the run-length table never leaves the devices.  Writes
 * vtx.len, vtx.cov, vtx.seq (save_seq), arc.ls and, with fo, the GFA lines.  OATK_E_SPLIT: a syncmer of the graph has no prepared consensus, or a piece would
 * begin at or behind position k; unless the code is OATK_OK the graph and fo are untouched. */
int oatk_multi_scg_consensus(oatk_multi *m, const oatk_overlap_t *o, const oatk_sr_db_t *sr_db, oatk_scg_t *g, int hoco_seq, int save_seq, FILE *fo);
/* scg_read_alignment (alignment.c:596): every handle aligns its own reads against the same graph, no exchange */
int oatk_multi_scg_read_alignment(oatk_multi *m, oatk_sr_db_t *sr_db, oatk_scg_ra_v *ra_v, oatk_scg_t *g, int for_unzip, uint64_t *n_skipped);
/* scg_ra_utg_coverage (syncasm.c:1882) and scg_ra_arc_coverage up to its refinement (:2067-2138), as oatk_scg_ra_utg_coverage / oatk_scg_ra_arc_coverage
 * leave them: vtx[].cov / the live arcs' cov of g->utg_asmg.  Every handle works on the alignments and corrected chains of its own reads where they
 * lie, resident (include/oatk_hip_racov.h: the *_sharded calls); what travels is the size of the graph, not of the reads.  ra_v must be what
 * oatk_multi_scg_read_alignment wrote last, for this g and unchanged (OATK_E_STATE otherwise, as for foreign reads).  Nothing is written unless the
 * code is OATK_OK (OATK_E_SPLIT: some handle is over the working limit -- run the original); the unitig call with no alignment prints the reference's
 * warning once and changes nothing.  The arc caller finishes with the reference's scg_refine_arc_coverage or asmg_arc_fix_cov itself. */
int oatk_multi_scg_ra_utg_coverage(oatk_multi *m, const oatk_sr_db_t *sr_db, const oatk_scg_ra_v *ra_v, oatk_scg_t *g, int verbose);
int oatk_multi_scg_ra_arc_coverage(oatk_multi *m, const oatk_sr_db_t *sr_db, const oatk_scg_ra_v *ra_v, oatk_scg_t *g, int verbose);
/* oatk_scg_multiplex_plan (include/oatk_syncasm.h) over the handles' resident alignments: the triplet table is handed from handle to handle
 * (oatk_hip_ra_triplet_scores_sharded), what travels is the size of the graph.  ra_v must be what oatk_multi_scg_read_alignment wrote last, for
 * this g and unchanged (OATK_E_STATE otherwise); nothing is written unless the code is OATK_OK */
int oatk_multi_scg_multiplex_plan(oatk_multi *m, const oatk_scg_ra_v *ra_v, const oatk_scg_t *g, uint32_t max_n_scm, double min_n_r, double min_d_f,
                                  uint8_t *multi_vtx, int *updated, oatk_triplet_table *tab);

#ifdef __cplusplus
}
#endif
#endif
