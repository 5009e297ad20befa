"""ctypes loader for the in-tree gfx950 library (oatk_amd/lib/liboatk_hip.so, C ABI in include/oatk_hip.h).

The product path has no CPU fallback: if the library is missing or no MI355X is visible, callers get an
exception, never a silently slower path.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OATK_HIP_LIB") or os.path.join(HERE, "lib", "liboatk_hip.so")   # override: development experiments only
HOST_LIB_PATH = os.path.join(HERE, "lib", "liboatk_host.so")

# names mirror include/oatk_hip.h
OK, E_NODEV, E_ARG, E_STATE, E_SMER, E_SPLIT, E_NOMEM = range(7)
READ_ALIGN = 64
BUF = {name: i for i, name in enumerate([
    "HOCO_L", "N_SCM", "N_NN", "N_LRL", "HO_RL", "HOCO_S", "NN_KEY", "LRL_KEY", "LRL_VAL",
    "SCM_OFF", "POS_MPOS", "POS_SMER", "POS_HASH", "POS_KID",
    "SCM_H", "SCM_S", "SCM_COV", "SCM_OCC_OFF", "SCM_OCC"])}
# include/oatk_hip_ec.h
BUF.update({name: 100 + i for i, name in enumerate([
    "EC_N_SCM", "EC_SCM_OFF", "EC_KMER", "EC_MPOS", "EC_SMER", "EC_SCM_COV", "EC_SCM_DEL", "EC_SCM_OCC_OFF", "EC_SCM_OCC", "EC_ERR_DEL",
    "EC_SCM_FWD", "EC_VTX_SRC", "EC_BLOCK_WORK", "EC_BLOCK_OUT", "EC_CSEQ_LEN", "EC_CSEQ_OFF", "EC_CSEQ", "EC_BLOCK_QEND"])})
# include/oatk_hip_ingest.h
BUF.update({name: 160 + i for i, name in enumerate(["INGEST_SEQ", "INGEST_OFF", "INGEST_LEN", "INGEST_HDR"])})
FMT_AUTO, FMT_FASTA, FMT_FASTQ = 0, 1, 2
# include/oatk_hip_cons.h
BUF.update({name: 140 + i for i, name in enumerate(["CONS_SEL", "CONS_SLOT", "CONS_RL", "CONS_MSEQ", "CONS_FIRST", "CONS_TOT",
                                                    "CONS_STR", "CONS_STR_OFF", "CONS_STR_LEN", "CONS_STR_STATUS"])})
# include/oatk_hip_align.h
BUF.update({name: 200 + i for i, name in enumerate(["RA_ALN_SID", "RA_ALN_OFF", "RA_ALN_S", "RA_FRG_UID", "RA_FRG_UBEG", "RA_FRG_UEND", "RA_FRG_SBEG", "RA_FRG_SEND", "RA_SKIPPED"])})
BUF.update({name: 150 + i for i, name in enumerate(["OVL_KEY", "OVL_OFF", "OVL_DIST", "OVL_CNT", "OVL_TAIL"])})
BUF.update({name: 120 + i for i, name in enumerate([
    "EG_IDX_P", "EG_IDX_N", "EG_ARC_V", "EG_ARC_W", "EG_ARC_LS", "EG_ARC_COV", "EG_ARC_COMP", "EG_OTHER"])})
# include/oatk_hip_graph.h
BUF.update({name: 180 + i for i, name in enumerate([
    "AG_SCM_DEL", "AG_VTX_SCM", "AG_VTX_COV", "AG_IDX_P", "AG_IDX_N", "AG_ARC_V", "AG_ARC_W", "AG_ARC_COV", "AG_ARC_COMP", "AG_ARC_LINK"])})
# include/oatk_hip_multi.h
BUF.update({name: 220 + i for i, name in enumerate(["MG_H", "MG_S", "MG_COV", "MG_L2G", "MG_EC_COV", "MG_EC_DEL", "MG_LCOV"])})
BUF.update({name: 230 + i for i, name in enumerate(["MG_G_H", "MG_G_S", "MG_G_COV", "MG_G_DEL", "MG_G_OCC_OFF", "MG_G_OCC", "MG_POS_GKID"])})
BUF["CONS_KMER"] = 240
# include/oatk_hip_racov.h
BUF.update({name: 250 + i for i, name in enumerate(["MC_UNIT", "MC_PATH_OFF", "MC_PATH_V", "MC_PATH_CNT"])})
TIMERS = ["hpc", "syncmer", "syncmer_n", "scan_post", "count_place", "count_sort", "count_group", "kmer_hash", "ec_graph", "ec_mark", "ec_solve", "ec_refresh"]

EXPORTS = [
    "oatk_hip_abi_version", "oatk_hip_device_count", "oatk_hip_create", "oatk_hip_destroy", "oatk_hip_last_error",
    "oatk_hip_stream", "oatk_hip_sync", "oatk_hip_max_k", "oatk_hip_scan", "oatk_hip_scan_host", "oatk_hip_count",
    "oatk_comm_unique_id", "oatk_comm_create", "oatk_comm_group_create", "oatk_comm_group_rank", "oatk_comm_group_destroy", "oatk_comm_destroy",
    "oatk_comm_rank", "oatk_comm_size", "oatk_comm_backend", "oatk_comm_traffic", "oatk_hip_merge_counts", "oatk_hip_multi_range", "oatk_hip_ec_sharded",
    "oatk_hip_gather_table", "oatk_hip_asm_graph_sharded", "oatk_hip_consensus_sharded", "oatk_hip_overlap_hist_sharded", "oatk_hip_stat_sharded",
    "oatk_hip_scan_begin", "oatk_hip_scan_reserve", "oatk_hip_scan_append", "oatk_hip_device", "oatk_hip_d2d", "oatk_hip_mem_pool",
    "oatk_hip_info", "oatk_hip_buffer", "oatk_hip_d2h", "oatk_hip_d2h_async", "oatk_hip_h2d_async", "oatk_hip_staging", "oatk_hip_ingest_text_buffer", "oatk_hip_set_timing", "oatk_hip_get_timing",
    "oatk_hip_debug_hash_mask", "oatk_hip_debug_force_general", "oatk_hip_debug_list_cap",
    "oatk_hip_ec_graph", "oatk_hip_ec_graph_light", "oatk_hip_ec", "oatk_hip_ec_stats", "oatk_hip_debug_ec_tiers", "oatk_hip_debug_wf_ed", "oatk_hip_debug_wf_ed_turns", "oatk_hip_debug_cov_runs", "oatk_hip_debug_wf_ed_wg", "oatk_hip_ec_mark", "oatk_hip_ec_correct",
    "oatk_hip_ec_set_global", "oatk_hip_ec_pairs", "oatk_hip_ec_graph_from_pairs", "oatk_hip_ec_graph_from_segments", "oatk_hip_ec_export_kmers", "oatk_hip_ec_import_kmers",
    "oatk_hip_ec_reserve_import", "oatk_hip_consensus", "oatk_hip_consensus_ids", "oatk_hip_ingest", "oatk_hip_ingest_host", "oatk_hip_scan_ingested", "oatk_hip_stat", "oatk_hip_stat_keys", "oatk_hip_stat_from_keys",
    "oatk_hip_asm_graph", "oatk_hip_asm_pairs", "oatk_hip_asm_graph_from_pairs", "oatk_hip_overlap_hist", "oatk_hip_overlap_pairs", "oatk_hip_overlap_hist_from_pairs", "oatk_hip_read_alignment", "oatk_hip_debug_align_two_pass",
    "oatk_hip_ra_utg_coverage", "oatk_hip_ra_arc_coverage", "oatk_hip_debug_racov_cap", "oatk_hip_ra_utg_coverage_sharded", "oatk_hip_ra_arc_coverage_sharded",
    "oatk_hip_ra_triplet_scores", "oatk_hip_ra_triplet_scores_sharded",
    "oatk_hip_ra_minicircle_units", "oatk_hip_ra_minicircle_times", "oatk_hip_debug_mc_hash_bits",
    "oatk_hip_ec_keep_seq", "oatk_hip_ec_corrected_reads", "oatk_hip_consensus_strings", "oatk_hip_consensus_strings_times",
    "oatk_hip_consensus_strings_sharded", "oatk_hip_consensus_kmer_time",
    "oatk_hip_inflate_bgzf", "oatk_hip_inflate_bgzf_host", "oatk_hip_inflate_last_byte", "oatk_hip_ingest_names",
    "oatk_hip_ingest_bam", "oatk_hip_ingest_bam_host", "oatk_hip_ingest_bam_stats", "oatk_hip_ingest_bam_times",
]

# the N-handle mirror in liboatk_host.so (include/oatk_multi.h) of entry points listed above; EXPORTS itself is checked against liboatk_hip.so
HOST_EXPORTS = ["oatk_multi_scg_ra_utg_coverage", "oatk_multi_scg_ra_arc_coverage", "oatk_scg_multiplex_plan", "oatk_multi_scg_multiplex_plan",
                "oatk_triplet_table_free", "oatk_multi_read_error_correction_fo", "oatk_multi_consensus", "oatk_multi_scg_consensus", "oatk_bgzf_index", "oatk_host_set_device_inflate", "oatk_host_inflate_counts",
                "oatk_extract_minicircles", "oatk_mc_path_stats", "oatk_mc_paths_free"]


def load_host():
    """liboatk_host.so with the argtypes of include/oatk_multi.h (the N-handle entry points the tests and timing scripts drive)"""
    H = C.CDLL(HOST_LIB_PATH)
    vp = C.c_void_p
    H.oatk_sr_db_new.restype = vp
    H.oatk_sr_db_new.argtypes = [C.c_int, C.c_int]
    H.oatk_multi_create.restype = vp
    H.oatk_multi_create.argtypes = [C.POINTER(C.c_int), C.c_int]
    H.oatk_multi_destroy.argtypes = [vp]
    H.oatk_multi_ctx.restype = vp
    H.oatk_multi_ctx.argtypes = [vp, C.c_int]
    H.oatk_multi_last_error.restype = C.c_char_p
    H.oatk_multi_last_error.argtypes = [vp]
    H.oatk_multi_range.argtypes = [vp, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    H.oatk_multi_sr_read_files.argtypes = [vp, vp, C.POINTER(C.c_char_p), C.c_int]
    H.oatk_multi_collect_syncmer_from_reads.restype = vp
    H.oatk_multi_collect_syncmer_from_reads.argtypes = [vp, vp, C.POINTER(C.c_int)]
    H.oatk_multi_read_error_correction.argtypes = [vp, vp, vp, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, vp]
    H.oatk_multi_read_error_correction_fo.argtypes = [vp, vp, vp, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, vp, vp]      # (..., FILE *fo, stats12)
    H.oatk_multi_make_syncmer_asmg.restype = vp
    H.oatk_multi_make_syncmer_asmg.argtypes = [vp, vp, C.c_uint32, C.c_double, C.POINTER(C.c_int)]
    H.oatk_multi_overlap_fetch.restype = vp
    H.oatk_multi_overlap_fetch.argtypes = [vp, C.c_uint32, C.POINTER(C.c_int)]
    H.oatk_overlap_destroy.argtypes = [vp]
    H.oatk_multi_consensus.argtypes = [vp, C.c_uint32]
    H.oatk_multi_scg_consensus.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp]      # (m, overlap tables, sr_db, scg, hoco_seq, save_seq, FILE *fo)
    H.oatk_multi_scg_read_alignment.argtypes = [vp, vp, vp, vp, C.c_int, C.POINTER(C.c_uint64)]
    H.oatk_multi_scg_ra_utg_coverage.argtypes = [vp, vp, vp, vp, C.c_int]
    H.oatk_multi_scg_ra_arc_coverage.argtypes = [vp, vp, vp, vp, C.c_int]
    H.oatk_scg_multiplex_plan.argtypes = [vp, vp, vp, C.c_uint, C.c_uint32, C.c_double, C.c_double, vp, C.POINTER(C.c_int), C.POINTER(TripletTable)]
    H.oatk_multi_scg_multiplex_plan.argtypes = [vp, vp, vp, C.c_uint32, C.c_double, C.c_double, vp, C.POINTER(C.c_int), C.POINTER(TripletTable)]
    H.oatk_triplet_table_free.restype = None
    H.oatk_triplet_table_free.argtypes = [C.POINTER(TripletTable)]
    H.oatk_extract_minicircles.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint, C.POINTER(McPaths)]
    H.oatk_mc_path_stats.argtypes = [vp, C.POINTER(McPaths)]
    H.oatk_mc_paths_free.restype = None
    H.oatk_mc_paths_free.argtypes = [C.POINTER(McPaths)]
    H.oatk_host_debug_window.argtypes = [C.c_uint64]
    H.oatk_bgzf_index.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]      # include/oatk_inflate.h
    return H


# oatk_bgzf_member_t (include/oatk_hip_ingest.h) as a numpy record: the member table of oatk_hip_inflate_bgzf / oatk_bgzf_index
BGZF_MEMBER = [("in_off", "<u8"), ("in_len", "<u4"), ("out_len", "<u4"), ("out_off", "<u8"), ("crc", "<u4"), ("pad", "<u4")]
INF_OK, INF_STREAM, INF_LENGTH, INF_CRC = range(4)


class TripletTable(C.Structure):
    """oatk_triplet_table (include/oatk_syncasm.h): the entries of scg_multiplex's tri_s that its lookups find"""
    _fields_ = [("n", C.c_uint64), ("m", C.c_uint64), ("l_in", C.POINTER(C.c_uint64)), ("l_out", C.POINTER(C.c_uint64)), ("val", C.POINTER(C.c_double))]


class McPath(C.Structure):
    """oatk_mc_path (include/oatk_syncasm.h): one distinct repeat unit round the anchor, the reference's path_t fields that extract_minicircles_with_anchor sets"""
    _fields_ = [("nv", C.c_uint32), ("v", C.POINTER(C.c_uint32)), ("len", C.c_uint32), ("wlen", C.c_double), ("cnt", C.c_uint64)]


class McPaths(C.Structure):
    """oatk_mc_paths"""
    _fields_ = [("n", C.c_uint64), ("m", C.c_uint64), ("a", C.POINTER(McPath))]


class EcGraph(C.Structure):
    """oatk_ec_graph_t (include/oatk_hip_ec.h): the reference's asmg_t flattened, host pointers"""
    _fields_ = [("n_vtx", C.c_uint64), ("n_arc", C.c_uint64), ("idx_p", C.c_void_p), ("idx_n", C.c_void_p), ("arc_v", C.c_void_p),
                ("arc_w", C.c_void_p), ("arc_ls", C.c_void_p), ("arc_cov", C.c_void_p), ("arc_del", C.c_void_p)]


class RaGraph(C.Structure):
    """oatk_ra_graph_t (include/oatk_hip_align.h): what scg_read_alignment reads from scg_t, flattened, host pointers"""
    _fields_ = [("n_scm", C.c_uint64), ("n_utg", C.c_uint64), ("n_arc", C.c_uint64), ("su_off", C.c_void_p), ("su_uid", C.c_void_p), ("su_pos", C.c_void_p),
                ("utg_n", C.c_void_p), ("idx_p", C.c_void_p), ("idx_n", C.c_void_p), ("arc_w", C.c_void_p), ("arc_ln", C.c_void_p), ("arc_del", C.c_void_p)]


class RacovGraph(C.Structure):
    """oatk_racov_graph_t (include/oatk_hip_racov.h): what scg_ra_utg_coverage / scg_ra_arc_coverage read from scg_t, flattened, host pointers"""
    _fields_ = [("n_scm", C.c_uint64), ("n_utg", C.c_uint64), ("n_arc", C.c_uint64), ("su_off", C.c_void_p), ("su_uid", C.c_void_p), ("su_pos", C.c_void_p),
                ("scm_cov", C.c_void_p), ("utg_off", C.c_void_p), ("utg_a", C.c_void_p), ("idx_p", C.c_void_p), ("idx_n", C.c_void_p), ("arc_v", C.c_void_p),
                ("arc_w", C.c_void_p), ("arc_link", C.c_void_p), ("arc_comp", C.c_void_p), ("arc_del", C.c_void_p), ("vtx_del", C.c_void_p)]


class RacovAln(C.Structure):
    """oatk_racov_aln_t: scg_ra_v flattened"""
    _fields_ = [("n_aln", C.c_uint64), ("n_frg", C.c_uint64), ("sid", C.c_void_p), ("off", C.c_void_p), ("s", C.c_void_p), ("uid", C.c_void_p),
                ("u_beg", C.c_void_p), ("u_end", C.c_void_p), ("s_beg", C.c_void_p), ("s_end", C.c_void_p)]


class RacovReads(C.Structure):
    """oatk_racov_reads_t: the reads' chains back to back"""
    _fields_ = [("n_reads", C.c_uint64), ("off", C.c_void_p), ("k_mer", C.c_void_p)]


class ConsPlan(C.Structure):
    """oatk_cons_plan_t (include/oatk_hip_cons.h): the sequences whose text oatk_hip_consensus_strings makes, host pointers"""
    _fields_ = [("n_seq", C.c_uint64), ("n_piece", C.c_uint64), ("seq_off", C.c_void_p), ("piece_v", C.c_void_p), ("piece_beg", C.c_void_p),
                ("want_bytes", C.c_void_p)]


class StatRaw(C.Structure):
    """oatk_stat_raw_t (include/oatk_hip_stat.h)"""
    _fields_ = [("n_reads", C.c_uint64), ("n_syncmers", C.c_uint64), ("sum_dist", C.c_int64), ("n_dist", C.c_uint64),
                ("smer_unique", C.c_uint64), ("kmer_unique", C.c_uint64), ("smer_cnt", C.c_int64 * 1001), ("kmer_cnt", C.c_int64 * 1001),
                ("smer_no_singleton", C.c_int64), ("kmer_no_singleton", C.c_int64)]


class Info(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("seq_bytes", C.c_uint64), ("sid0", C.c_uint64),
                ("k", C.c_int32), ("s", C.c_int32),
                ("n_occ", C.c_uint64), ("n_nn", C.c_uint64), ("n_lrl", C.c_uint64), ("n_scm", C.c_uint64),
                ("scan_retries", C.c_uint32), ("collisions", C.c_uint32)]


class OatkHipError(RuntimeError):
    pass


_lib = None


def load():
    """Load liboatk_hip.so; raises if it has not been built (python -c 'import __graft_entry__ as g; g.build()')."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OatkHipError("%s is missing: build it with __graft_entry__.build()" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.oatk_hip_abi_version.restype = C.c_int
    L.oatk_hip_device_count.restype = C.c_int
    L.oatk_hip_create.restype = vp
    L.oatk_hip_create.argtypes = [C.c_int]
    L.oatk_hip_destroy.argtypes = [vp]
    L.oatk_hip_last_error.restype = C.c_char_p
    L.oatk_hip_last_error.argtypes = [vp]
    L.oatk_hip_stream.restype = vp
    L.oatk_hip_stream.argtypes = [vp]
    L.oatk_hip_sync.argtypes = [vp]
    L.oatk_hip_max_k.restype = C.c_int
    L.oatk_hip_scan.argtypes = [vp, vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int]
    L.oatk_hip_scan_host.argtypes = [vp, vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int]
    L.oatk_hip_count.argtypes = [vp]
    L.oatk_comm_unique_id.argtypes = [vp]
    L.oatk_comm_create.restype = vp
    L.oatk_comm_create.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.oatk_comm_group_create.restype = vp
    L.oatk_comm_group_create.argtypes = [C.c_int]
    L.oatk_comm_group_rank.restype = vp
    L.oatk_comm_group_rank.argtypes = [vp, C.c_int]
    L.oatk_comm_group_destroy.argtypes = [vp]
    L.oatk_comm_destroy.argtypes = [vp]
    L.oatk_comm_rank.argtypes = [vp]
    L.oatk_comm_size.argtypes = [vp]
    L.oatk_comm_backend.restype = C.c_char_p
    L.oatk_comm_backend.argtypes = [vp]
    L.oatk_comm_traffic.restype = None
    L.oatk_comm_traffic.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
    L.oatk_hip_merge_counts.argtypes = [vp, vp, C.POINTER(C.c_uint64)]
    L.oatk_hip_multi_range.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.oatk_hip_ec_sharded.argtypes = [vp, vp, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, vp, C.POINTER(C.c_uint64)]
    L.oatk_hip_gather_table.argtypes = [vp, vp, C.c_int]
    L.oatk_hip_asm_graph_sharded.argtypes = [vp, vp, C.c_uint32, C.c_double, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.oatk_hip_consensus_sharded.argtypes = [vp, vp, C.c_uint32]
    L.oatk_hip_overlap_hist_sharded.argtypes = [vp, vp, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.oatk_hip_stat_sharded.argtypes = [vp, vp, C.POINTER(StatRaw)]
    L.oatk_hip_scan_begin.argtypes = [vp, C.c_uint64, C.c_int, C.c_int]
    L.oatk_hip_scan_reserve.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64]
    L.oatk_hip_scan_append.argtypes = [vp, vp]
    L.oatk_hip_device.argtypes = [vp]
    L.oatk_hip_mem_pool.argtypes = [vp, C.c_uint64]
    L.oatk_hip_d2d.argtypes = [vp, vp, vp, C.c_uint64]
    L.oatk_hip_info.argtypes = [vp, C.POINTER(Info)]
    L.oatk_hip_buffer.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.oatk_hip_d2h.argtypes = [vp, vp, vp, C.c_uint64]
    L.oatk_hip_staging.restype = vp
    L.oatk_hip_staging.argtypes = [vp, C.c_uint64]
    L.oatk_hip_set_timing.argtypes = [vp, C.c_int]
    L.oatk_hip_get_timing.argtypes = [vp, C.POINTER(C.c_float), C.c_int]
    L.oatk_hip_debug_hash_mask.argtypes = [vp, C.c_uint64]
    L.oatk_hip_debug_force_general.argtypes = [vp, C.c_int]
    L.oatk_hip_debug_list_cap.argtypes = [vp, C.c_int]
    L.oatk_hip_ec_graph.argtypes = [vp]
    L.oatk_hip_ec_graph_light.argtypes = [vp, C.c_uint32]
    L.oatk_hip_ec.argtypes = [vp, C.POINTER(EcGraph), C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double]
    L.oatk_hip_ec_stats.argtypes = [vp, vp]
    L.oatk_hip_debug_ec_tiers.argtypes = [vp, C.c_int, C.c_int]
    L.oatk_hip_debug_wf_ed.argtypes = [vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "oatk_hip_debug_wf_ed_turns"):   # (a library built before r20 lacks it)
        L.oatk_hip_debug_wf_ed_turns.argtypes = [vp, C.c_int, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "oatk_hip_debug_cov_runs"):
        L.oatk_hip_debug_cov_runs.argtypes = [vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp, vp]
    if hasattr(L, "oatk_hip_debug_wf_ed_wg"):      # (an experiments library built before round 5 lacks it)
        L.oatk_hip_debug_wf_ed_wg.argtypes = [vp, C.c_int, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "oatk_hip_debug_ed_ab"):      # tools/experiments/liboatk_hip_experiments.so only
        L.oatk_hip_debug_ed_ab.argtypes = [vp, C.c_int, C.c_uint64, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_float)]
    L.oatk_hip_ec_mark.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double]
    L.oatk_hip_ec_correct.argtypes = [vp, C.c_double]
    L.oatk_hip_ec_keep_seq.argtypes = [vp, C.c_int]
    L.oatk_hip_ec_corrected_reads.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.oatk_hip_ec_set_global.argtypes = [vp, C.c_uint64, vp, vp, vp]
    L.oatk_hip_ec_pairs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.oatk_hip_ec_graph_from_pairs.argtypes = [vp, vp, vp, C.c_uint64]
    L.oatk_hip_ec_graph_from_segments.argtypes = [vp, vp, vp, C.c_uint64]
    L.oatk_hip_ec_export_kmers.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, vp]
    L.oatk_hip_ec_import_kmers.argtypes = [vp, vp, vp, vp, C.c_uint64, C.c_uint32]
    L.oatk_hip_ec_reserve_import.argtypes = [vp, C.c_uint64]
    L.oatk_hip_consensus.argtypes = [vp, C.c_uint32]
    L.oatk_hip_consensus_ids.argtypes = [vp, vp, C.c_uint64]
    L.oatk_hip_consensus_strings.argtypes = [vp, C.POINTER(ConsPlan), C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.oatk_hip_consensus_strings_times.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
    L.oatk_hip_consensus_strings_sharded.argtypes = [vp, vp, C.POINTER(ConsPlan), C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.oatk_hip_consensus_kmer_time.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
    L.oatk_hip_ingest.argtypes = [vp, vp, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.oatk_hip_ingest_host.argtypes = [vp, vp, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.oatk_hip_scan_ingested.argtypes = [vp, C.c_uint64, C.c_int, C.c_int]
    L.oatk_hip_ingest_text_buffer.argtypes = [vp, C.c_uint64, C.POINTER(vp)]
    L.oatk_hip_inflate_bgzf.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64), vp]
    L.oatk_hip_inflate_bgzf_host.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64), vp]
    L.oatk_hip_inflate_last_byte.argtypes = [vp]
    L.oatk_hip_ingest_names.argtypes = [vp, vp, C.c_uint64, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.oatk_hip_ingest_bam.argtypes = [vp, vp, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.oatk_hip_ingest_bam_host.argtypes = [vp, vp, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.oatk_hip_ingest_bam_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.oatk_hip_ingest_bam_times.argtypes = [vp, C.POINTER(C.c_float)]
    L.oatk_hip_stat.argtypes = [vp, C.POINTER(StatRaw)]
    L.oatk_hip_stat_keys.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint64), vp]
    L.oatk_hip_stat_from_keys.argtypes = [vp, vp, vp, C.c_uint64, vp, C.POINTER(StatRaw)]
    L.oatk_hip_debug_align_two_pass.argtypes = [vp, C.c_int]
    L.oatk_hip_read_alignment.argtypes = [vp, C.POINTER(RaGraph), vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp]
    L.oatk_hip_ra_utg_coverage.argtypes = [vp, C.POINTER(RacovGraph), C.POINTER(RacovReads), C.POINTER(RacovAln), C.c_int, vp, C.POINTER(C.c_uint64)]
    L.oatk_hip_ra_arc_coverage.argtypes = [vp, C.POINTER(RacovGraph), C.POINTER(RacovAln), vp]
    L.oatk_hip_debug_racov_cap.argtypes = [vp, C.c_uint64]
    L.oatk_hip_ra_utg_coverage_sharded.argtypes = [vp, vp, C.POINTER(RacovGraph), C.POINTER(RacovReads), C.POINTER(RacovAln), C.c_int, vp, C.POINTER(C.c_uint64)]
    L.oatk_hip_ra_arc_coverage_sharded.argtypes = [vp, vp, C.POINTER(RacovGraph), C.POINTER(RacovAln), vp]
    u64p = C.POINTER(C.c_uint64)
    L.oatk_hip_ra_triplet_scores.argtypes = [vp, C.POINTER(RacovGraph), C.POINTER(RacovAln), vp, C.c_uint64, u64p, vp, vp, vp, vp]
    L.oatk_hip_ra_triplet_scores_sharded.argtypes = [vp, vp, C.POINTER(RacovGraph), C.POINTER(RacovAln), vp, C.c_uint64, u64p, vp, vp, vp, vp]
    L.oatk_hip_ra_minicircle_units.argtypes = [vp, C.POINTER(RacovAln), C.c_uint64, u64p, u64p, u64p]
    L.oatk_hip_ra_minicircle_times.argtypes = [vp, C.POINTER(C.c_float), u64p]
    L.oatk_hip_debug_mc_hash_bits.argtypes = [vp, C.c_uint]
    L.oatk_hip_overlap_pairs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.oatk_hip_overlap_hist_from_pairs.argtypes = [vp, vp, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.oatk_hip_overlap_hist.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.oatk_hip_asm_graph.argtypes = [vp, C.c_uint32, C.c_double, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.oatk_hip_asm_pairs.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.oatk_hip_asm_graph_from_pairs.argtypes = [vp, vp, C.c_uint64, C.c_uint64, vp, vp, C.c_uint32, C.c_double, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    _lib = L
    return L
