"""GPU parity of the coverage estimates from read alignments (oatk_scg_ra_utg_coverage / oatk_scg_ra_arc_coverage of liboatk_host.so over
include/oatk_hip_racov.h) against the COMPILED REFERENCE's scg_ra_utg_coverage, scg_ra_arc_coverage, scg_refine_arc_coverage and
asmg_arc_fix_cov (syncasm.c:1882-2147, graph.c:237) on the same structures.  Every comparison is exact: all vtx[].cov and arc[].cov.

Procedure of every comparison: snapshot the covs, run the device adaptor, restore, run the reference, compare, go on with the reference's
result.  The device runs twice: with the alignments and chains resident in the handle, and with everything uploaded."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import ref_lib as R
from racov_util import Scg
import test_gpu_align as GA
from test_gpu_dropin import device_dbs

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")

RESIDENT_READS, RESIDENT_ALN = 1, 2
E_SPLIT = 5


def libs():
    L, H = GA.setup_libs()
    vp = C.c_void_p
    L.scg_ra_utg_coverage.argtypes = [vp, vp, vp, C.c_int]
    L.scg_ra_arc_coverage.argtypes = [vp, vp, vp, C.c_int, C.c_int]
    L.scg_refine_arc_coverage.argtypes = [vp, C.c_int]
    L.asmg_arc_fix_cov.argtypes = [vp]
    H.oatk_scg_ra_utg_coverage.argtypes = [vp, vp, vp, vp, C.c_uint, C.c_int]
    H.oatk_scg_ra_arc_coverage.argtypes = [vp, vp, vp, vp, C.c_uint, C.c_int]
    return L, H


def asmg(g):
    return C.cast(g, C.POINTER(Scg)).contents.utg_asmg.contents


def covs(g):
    a = asmg(g)
    return (np.array([a.vtx[i].cov for i in range(a.n_vtx)], np.uint32), np.array([a.arc[i].cov for i in range(a.n_arc)], np.uint32))


def restore(g, snap):
    a = asmg(g)
    for i in range(a.n_vtx):
        a.vtx[i].cov = int(snap[0][i])
    for i in range(a.n_arc):
        a.arc[i].cov = int(snap[1][i])


def assert_covs(got, want, what):
    assert np.array_equal(got[0], want[0]), ("vtx", what, np.flatnonzero(got[0] != want[0])[:10])
    assert np.array_equal(got[1], want[1]), ("arc", what, np.flatnonzero(got[1] != want[1])[:10])


def finish_arcs(L, g, refine):
    """what scg_ra_arc_coverage does after the duplet sums (:2143-2146): stays the reference's"""
    if refine:
        L.scg_refine_arc_coverage(g, 0)
    else:
        L.asmg_arc_fix_cov(C.cast(g, C.POINTER(Scg)).contents.utg_asmg)


def compare_utg(L, H, hip, db, v, g, flags_list=(RESIDENT_READS | RESIDENT_ALN, 0), verbose=0):
    snap = covs(g)
    got = []
    for flags in flags_list:
        rc = H.oatk_scg_ra_utg_coverage(hip.h, db, v, g, flags, verbose)
        assert rc == 0, hip.L.oatk_hip_last_error(hip.h)
        got.append(covs(g))
        restore(g, snap)
    L.scg_ra_utg_coverage(g, db, v, verbose)
    want = covs(g)
    for x, flags in zip(got, flags_list):
        assert_covs(x, want, ("utg", flags))


def compare_arc(L, H, hip, db, v, g, flags_list=(RESIDENT_ALN, 0)):
    for refine in (0, 1):
        snap = covs(g)
        got = []
        for flags in flags_list:
            rc = H.oatk_scg_ra_arc_coverage(hip.h, db, v, g, flags, 0)
            assert rc == 0, hip.L.oatk_hip_last_error(hip.h)
            finish_arcs(L, g, refine)
            got.append(covs(g))
            restore(g, snap)
        L.scg_ra_arc_coverage(g, db, v, refine, 0)
        want = covs(g)
        for x, flags in zip(got, flags_list):
            assert_covs(x, want, ("arc", refine, flags))
        if refine == 0:
            restore(g, snap)


def tally(L, v, seen):
    f = GA.flatten(L, v)
    if len(f["sid"]) == 0:
        return
    frac = np.modf(f["s"])[0] > np.finfo(np.float64).eps
    _, cnt = np.unique(f["sid"], return_counts=True)
    seen["multi_aln"] += int(frac.sum()) if cnt.max() >= 2 else 0
    seen["multi_frg"] += int((f["n"] >= 2).sum())
    seen["calls"] += 1


@needs_ref
@pytest.mark.parametrize("case", range(len(GA.CASES)))
def test_coverage_matches_reference_through_the_pipeline(hip, case):
    """test_gpu_align.CASES driven like test_read_alignment_matches_reference: after every alignment both functions are compared, the arc
    coverage with refine 0 and 1, the device with resident alignments and chains and with everything uploaded"""
    K, S, c, mk = GA.CASES[case]
    L, H = libs()
    db, scm = device_dbs(hip, mk(), K, S)
    st = np.zeros(12, np.uint64)
    assert H.oatk_read_error_correction(hip.h, db, scm, None, 0.02, c, 10 * c, c, 0.35, st.ctypes.data) == 0
    g = L.refx_make_graph(db, scm, c, 0.35)
    assert g
    v = L.refx_ra_new()
    seen = {"multi_aln": 0, "multi_frg": 0, "calls": 0}

    def align(for_unzip):
        nsk = C.c_uint64(0)
        rc = H.oatk_scg_read_alignment(hip.h, db, v, g, for_unzip, C.byref(nsk), None)
        assert rc == 0, hip.L.oatk_hip_last_error(hip.h)
        tally(L, v, seen)
        compare_utg(L, H, hip, db, v, g)
        compare_arc(L, H, hip, db, v, g)

    align(0)
    L.refx_process_unitigs(g)
    align(0)
    max_n_scm = int(math.ceil(30000.0 / K))
    for _ in range(3):
        align(1)
        L.refx_update_utg_cov(g)
        if L.refx_multiplex(g, v, max_n_scm, 10.0, 0.3) == 0:
            break
    align(1)
    align(0)
    print("case", case, seen)
    assert seen["calls"] >= 4
    if case == 3:
        assert seen["multi_aln"] > 0            # reads with two or more alignments: EM blocks of two or more members
    if case in (2, 3, 4, 5):
        assert seen["multi_frg"] > 0            # records with two or more fragments: arc duplets
    L.refx_ra_destroy(v)
    L.refx_scg_destroy(g)
    L.refx_scmdb_destroy(scm)
    L.refx_srdb_destroy(db)


# ---- the synthetic set ----
A_, B_, C_ = 0, 1, 2
UTG = [[0, 1, 2, 3, 4, 20, 21, 22, 23, 24],
       [0, 1, 2, 3, 4, 25, 26, 27, 28, 29, 10, 11, 12, 13, 14],
       [10, 11, 12, 13, 14, 30, 31, 32, 33, 34]]
N_SCM = 100
# arcs sorted by v (oriented: utg << 1 | rev): (v, w, link_id, comp, del)
ARCS = [(0, 2, 0, 0, 0),        # A+ -> B+
        (0, 4, 3, 0, 1),        # A+ -> C+, deleted (asmg_arc still finds it)
        (2, 4, 1, 0, 0),        # B+ -> C+
        (3, 1, 0, 1, 0),        # B- -> A-
        (4, 5, 2, 0, 0),        # C+ -> C-, self-complementary
        (5, 3, 1, 1, 0),        # C- -> B-
        (5, 1, 3, 1, 0)]        # C- -> A-, the live complement of the deleted arc


def synthetic_reads():
    """(chain, [(s, [(uid, u_beg, u_end, s_beg, s_end), ...]), ...]) per read"""
    rd = []
    one = lambda u, ub, ue, sb=0, se=4: (u, ub, ue, sb, se)
    rd += [([20, 21, 22, 23, 24], [(5.0, [one(A_ << 1, 5, 9)])])] * 10                       # unique on A
    rd += [([25, 26, 27, 28, 29], [(5.0, [one(B_ << 1, 5, 9)])])] * 40                       # unique on B
    rd += [([30, 31, 32, 33, 34], [(5.0, [one(C_ << 1, 5, 9)])])] * 25                       # unique on C
    rd += [([0, 1, 2, 3, 4], [(5.5, [one(A_ << 1, 0, 4)]), (5.5, [one(B_ << 1, 0, 4)])])] * 30          # two alignments, (A, B)
    rd += [([10, 11, 12, 13, 14], [(5.5, [one(B_ << 1, 10, 14)]), (5.5, [one(C_ << 1, 0, 4)])])] * 20   # two alignments, (B, C)
    # a chain that differs from the unitig slice: the LCS matrix and its backtrace run (a tie included)
    rd += [([20, 22, 21, 23, 24], [(5.0, [one(A_ << 1, 5, 9)])])] * 2
    rd += [([0, 2, 1, 3, 4], [(5.5, [one(A_ << 1, 0, 4)]), (5.5, [one(B_ << 1, 0, 4)])])] * 3
    rd += [([20, 99, 98, 23, 24, 25], [(6.0, [one(A_ << 1, 5, 9, 0, 4), one(B_ << 1, 5, 5, 5, 5)])])]
    # reverse-strand fragments
    rd += [([34, 33, 32, 31, 30], [(5.0, [one(C_ << 1 | 1, 5, 9)])])] * 3
    rd += [([34, 32, 33, 31, 30], [(5.0, [one(C_ << 1 | 1, 5, 9)])])]
    # records that yield no LCS block: alone, and beside one that does (the read gets no block)
    rd += [([90, 91, 92, 93, 94], [(5.0, [one(C_ << 1, 5, 9)])])]
    rd += [([0, 1, 2, 3, 4], [(5.5, [one(A_ << 1, 0, 4)]), (5.5, [one(C_ << 1, 5, 9)])])]
    # two alignments of two fragments each: the score < .99 branch, with unique syncmers (A+ 5..9, B+ 5..9) and without (A+ 0..4, B+ 0..4)
    rd += [([20, 21, 22, 23, 24, 25, 26, 27, 28, 29], [(10.5, [one(A_ << 1, 5, 9, 0, 4), one(B_ << 1, 5, 9, 5, 9)]),
                                                       (10.5, [one(A_ << 1, 0, 4, 0, 4), one(B_ << 1, 0, 4, 5, 9)])])] * 3
    # unique two-fragment records: B+ -> C+
    rd += [([10, 11, 12, 13, 14, 30, 31, 32, 33, 34], [(10.0, [one(B_ << 1, 10, 14, 0, 4), one(C_ << 1, 5, 9, 5, 9)])])] * 5
    # the self-complementary arc C+ -> C-
    rd += [([30, 31, 32, 33, 34, 34, 33, 32, 31, 30], [(10.0, [one(C_ << 1, 5, 9, 0, 4), one(C_ << 1 | 1, 5, 9, 5, 9)])])] * 3
    # the deleted arc A+ -> C+
    rd += [([20, 21, 22, 23, 24, 30, 31, 32, 33, 34], [(10.0, [one(A_ << 1, 5, 9, 0, 4), one(C_ << 1, 5, 9, 5, 9)])])] * 2
    return rd


# the duplet sums by kh_dbl's rules (before the (uint32_t)), arc index -> value.  A+ -> B+: 1 (the unique two-fragment record of the LCS
# reads) + 3 x .5 (both fragments unique; the second records of those reads have no unique syncmer); the self-complementary arc: its first
# score is SET (1), each later one added twice (2 + 2); the deleted arc gets nothing, its live complement the two scores
WANT_ARC = {0: 2.5, 1: 0.0, 2: 5.0, 3: 2.5, 4: 5.0, 5: 5.0, 6: 2.0}


class Synthetic:
    def __init__(self, L, reads=None):
        reads = synthetic_reads() if reads is None else reads
        self.L = L
        vp = C.c_void_p
        L.refx_fake_srdb.restype = vp
        L.refx_fake_srdb.argtypes = [C.c_uint64, vp, vp, vp]
        L.refx_fake_scmdb.restype = vp
        L.refx_fake_scmdb.argtypes = [C.c_uint64, vp, vp]
        L.refx_fake_dbs_free.argtypes = [vp, vp]
        L.refx_scg_from_flat.restype = vp
        L.refx_scg_from_flat.argtypes = [vp, C.c_uint64, C.c_uint64] + [vp] * 10
        L.refx_scg_flat_destroy.argtypes = [vp]
        L.refx_ra_build.restype = vp
        L.refx_ra_build.argtypes = [C.c_uint64] + [vp] * 8
        n_scm = np.array([len(c) for c, _ in reads], np.uint32)
        kmer = np.array([x << 1 for c, _ in reads for x in c], np.uint64)
        mpos = np.zeros(len(kmer), np.uint32)
        self.db = L.refx_fake_srdb(len(reads), n_scm.ctypes.data, kmer.ctypes.data, mpos.ctypes.data)
        self.chains = (np.concatenate([[0], np.cumsum(n_scm.astype(np.uint64))]).astype(np.uint64), kmer)
        cov = (20 + (np.arange(N_SCM) * 7) % 13).astype(np.uint32)
        self.scm = L.refx_fake_scmdb(N_SCM, cov.ctypes.data, np.zeros(N_SCM, np.uint8).ctypes.data)
        su = [[] for _ in range(N_SCM)]
        for u, lst in enumerate(UTG):
            for p, s in enumerate(lst):
                su[s].append((u << 1, p))
        su_off = np.concatenate([[0], np.cumsum([len(x) for x in su])]).astype(np.uint64)
        su_uid = np.array([e[0] for x in su for e in x], np.uint64)
        su_pos = np.array([e[1] for x in su for e in x], np.uint32)
        utg_n = np.array([len(x) for x in UTG], np.uint32)
        av = np.array([a[0] for a in ARCS], np.uint64)
        aw = np.array([a[1] for a in ARCS], np.uint64)
        idx_p = np.zeros(2 * len(UTG), np.uint64)
        idx_n = np.zeros(2 * len(UTG), np.uint64)
        for i, a in enumerate(ARCS):
            if idx_n[a[0]] == 0:
                idx_p[a[0]] = i
            idx_n[a[0]] += 1
        self.g = L.refx_scg_from_flat(self.scm, len(UTG), len(ARCS), su_off.ctypes.data, su_uid.ctypes.data, su_pos.ctypes.data, utg_n.ctypes.data,
                                      idx_p.ctypes.data, idx_n.ctypes.data, av.ctypes.data, aw.ctypes.data, np.zeros(len(ARCS), np.uint64).ctypes.data,
                                      np.array([a[4] for a in ARCS], np.uint8).ctypes.data)
        # refx_scg_from_flat leaves vtx[].a, link_id and comp zero: filled through the layout mirrors
        self.lists = [np.array([s << 1 for s in lst], np.uint64) for lst in UTG]
        ag = asmg(self.g)
        for u, x in enumerate(self.lists):
            ag.vtx[u].a = x.ctypes.data
        for i, a in enumerate(ARCS):
            ag.arc[i].link_id, ag.arc[i].comp = a[2], a[3]
        # ra_v
        sid, n, s, uid, ub, ue, sb, se = [], [], [], [], [], [], [], []
        for r, (_, recs) in enumerate(reads):
            for sc, frags in recs:
                sid.append(r), n.append(len(frags)), s.append(sc)
                for f in frags:
                    uid.append(f[0]), ub.append(f[1]), ue.append(f[2]), sb.append(f[3]), se.append(f[4])
        self.aln = {"sid": np.array(sid, np.uint64), "n": np.array(n, np.uint32), "s": np.array(s, np.float64), "uid": np.array(uid, np.uint64),
                    "u_beg": np.array(ub, np.uint64), "u_end": np.array(ue, np.uint64), "s_beg": np.array(sb, np.uint32), "s_end": np.array(se, np.uint32)}
        self.v = L.refx_ra_build(len(sid), *[self.aln[k].ctypes.data for k in ("sid", "n", "s", "uid", "u_beg", "u_end", "s_beg", "s_end")])
        self.graph = {"n_scm": N_SCM, "su_off": su_off, "su_uid": su_uid, "su_pos": su_pos, "scm_cov": cov,
                      "utg_off": np.concatenate([[0], np.cumsum(utg_n.astype(np.uint64))]).astype(np.uint64), "utg_a": np.concatenate(self.lists),
                      "idx_p": idx_p, "idx_n": idx_n, "arc_v": av, "arc_w": aw, "arc_link": np.array([a[2] for a in ARCS], np.uint64),
                      "arc_comp": np.array([a[3] for a in ARCS], np.uint8), "arc_del": np.array([a[4] for a in ARCS], np.uint8)}

    def flat_aln(self):
        a = self.aln
        return {"sid": a["sid"], "off": np.concatenate([[0], np.cumsum(a["n"].astype(np.uint64))]).astype(np.uint64), "s": a["s"], "uid": a["uid"],
                "u_beg": a["u_beg"], "u_end": a["u_end"], "s_beg": a["s_beg"], "s_end": a["s_end"]}

    def close(self):
        self.L.refx_ra_destroy(self.v)
        self.L.refx_scg_flat_destroy(self.g)
        self.L.refx_fake_dbs_free(self.db, self.scm)


def em_lines(err):
    return [x for x in err.splitlines() if x.startswith("[M::scg_ra_utg_coverage]") or x.startswith("[W::scg_ra_utg_coverage]")]


@needs_ref
def test_synthetic_em_and_edge_cases_match_reference(hip, capfd):
    """three unitigs over shared syncmers, unique reads (10, 40, 25), reads with two alignments on (A, B) and (B, C), and the edge cases of
    make_ma_block and the duplet table: the EM must run several iterations, print the reference's lines, and leave the reference's covs"""
    L, H = libs()
    syn = Synthetic(L)
    try:
        g, v, db = syn.g, syn.v, syn.db
        snap = covs(g)
        capfd.readouterr()
        assert H.oatk_scg_ra_utg_coverage(hip.h, db, v, g, 0, 3) == 0, hip.L.oatk_hip_last_error(hip.h)
        got = covs(g)
        dev_lines = em_lines(capfd.readouterr().err)
        restore(g, snap)
        L.scg_ra_utg_coverage(g, db, v, 3)
        want = covs(g)
        ref_lines = em_lines(capfd.readouterr().err)
        print("\n".join(ref_lines[-3:]), want[0])
        m = re.search(r"ended at iteration (\d+)", ref_lines[-1])
        assert m and int(m.group(1)) >= 3, ref_lines[-3:]
        assert dev_lines == ref_lines
        assert_covs(got, want, "synthetic utg")
        # the raw doubles, through the Python binding: the EM's count and the unitig values before the (uint32_t)
        avg, it = hip.ra_utg_coverage(syn.graph, syn.flat_aln(), syn.chains)
        assert it == int(m.group(1)) and np.array_equal(avg.astype(np.uint32), want[0])
        # the arc coverage on top of the reference's unitig coverage, refine 0 (asmg_arc_fix_cov) against the reference
        compare_arc_fix(L, H, hip, syn)
        raw = hip.ra_arc_coverage(syn.graph, syn.flat_aln())
        print("raw arc sums", raw)
        for i, x in WANT_ARC.items():
            assert raw[i] == x, (i, raw[i], x)
    finally:
        syn.close()


def compare_arc_fix(L, H, hip, syn):
    g, v, db = syn.g, syn.v, syn.db
    snap = covs(g)
    assert H.oatk_scg_ra_arc_coverage(hip.h, db, v, g, 0, 0) == 0, hip.L.oatk_hip_last_error(hip.h)
    finish_arcs(L, g, 0)
    got = covs(g)
    restore(g, snap)
    L.scg_ra_arc_coverage(g, db, v, 0, 0)
    want = covs(g)
    assert_covs(got, want, "synthetic arc")
    assert want[1].max() > 0


@needs_ref
def test_no_alignment_warns_and_changes_nothing(hip, capfd):
    L, H = libs()
    syn = Synthetic(L)
    empty = L.refx_ra_new()
    try:
        a = asmg(syn.g)
        for i in range(a.n_vtx):
            a.vtx[i].cov = 7 + i
        snap = covs(syn.g)
        capfd.readouterr()
        assert H.oatk_scg_ra_utg_coverage(hip.h, syn.db, empty, syn.g, 0, 3) == 0
        dev = capfd.readouterr().err
        assert_covs(covs(syn.g), snap, "empty, device")
        L.scg_ra_utg_coverage(syn.g, syn.db, empty, 3)
        ref = capfd.readouterr().err
        assert_covs(covs(syn.g), snap, "empty, reference")
        assert em_lines(dev) == em_lines(ref) and len(em_lines(ref)) == 1 and "no read alignment" in ref
    finally:
        L.refx_ra_destroy(empty)
        syn.close()


@needs_ref
def test_refusal_over_the_lcs_limit_writes_nothing(hip):
    """a debug cap of one LCS-matrix cell: the synthetic set needs more, so the call refuses (OATK_E_SPLIT) and leaves every cov as it was"""
    L, H = libs()
    syn = Synthetic(L)
    try:
        a = asmg(syn.g)
        for i in range(a.n_vtx):
            a.vtx[i].cov = 3 + i
        for i in range(a.n_arc):
            a.arc[i].cov = 11 + i
        snap = covs(syn.g)
        hip._check(hip.L.oatk_hip_debug_racov_cap(hip.h, 1), "oatk_hip_debug_racov_cap")
        try:
            assert H.oatk_scg_ra_utg_coverage(hip.h, syn.db, syn.v, syn.g, 0, 0) == E_SPLIT
        finally:
            hip._check(hip.L.oatk_hip_debug_racov_cap(hip.h, 0), "oatk_hip_debug_racov_cap")
        assert_covs(covs(syn.g), snap, "refused")
        assert H.oatk_scg_ra_utg_coverage(hip.h, syn.db, syn.v, syn.g, 0, 0) == 0
    finally:
        syn.close()


@needs_ref
def test_tail_with_device_coverage_prints_the_reference_gfa(hip, tmp_path):
    """run_syncasm.c:160-303 in the reference's order through its exported functions (cleanup, weak cross-links, demultiplex, consensus),
    the coverage calls of :245, :260-261 and :296-297 served by the device adaptor: both GFA files equal a pure-reference run's, byte for byte"""
    import filecmp
    K, S, c, mk = GA.CASES[3]
    reads = mk()
    L, H = libs()
    vp = C.c_void_p
    L.refx_syncasm_tail.restype = C.c_int
    L.refx_syncasm_tail.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_char_p]
    L.scg_consensus.argtypes = [vp, vp, C.c_int, C.c_int, vp]
    L.scg_demultiplex.argtypes = [vp]
    for f in ("asmg_drop_tip", "asmg_pop_bubble", "asmg_remove_weak_crosslink"):
        getattr(L, f).restype = C.c_uint64
    L.asmg_drop_tip.argtypes = [vp, C.c_int32, C.c_uint64, C.c_int, C.c_int, C.c_int]
    L.asmg_pop_bubble.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int]
    L.asmg_remove_weak_crosslink.argtypes = [vp, C.c_double, C.c_double, C.c_int, C.c_int]
    libc = C.CDLL(None)
    libc.fopen.restype = vp
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [vp]
    bubble, tip, weak, unzip = 100000, 10000, 0.3, 3
    st = np.zeros(12, np.uint64)
    # the pure reference, on the device's corrected databases
    db, scm = device_dbs(hip, reads, K, S)
    assert H.oatk_read_error_correction(hip.h, db, scm, None, 0.02, c, 10 * c, c, 0.35, st.ctypes.data) == 0
    ref = str(tmp_path / "ref")
    assert L.refx_syncasm_tail(db, scm, K, bubble, tip, c, 0.35, weak, 0, unzip, 1, ref.encode()) == 0
    L.refx_scmdb_destroy(scm)
    L.refx_srdb_destroy(db)
    # the same tail driven here (fresh databases: the resident batch is theirs)
    db, scm = device_dbs(hip, reads, K, S)
    assert H.oatk_read_error_correction(hip.h, db, scm, None, 0.02, c, 10 * c, c, 0.35, st.ctypes.data) == 0
    dev = str(tmp_path / "dev")
    g = L.refx_make_graph(db, scm, c, 0.35)                                     # :138
    ag = lambda: C.cast(g, C.POINTER(Scg)).contents.utg_asmg
    v = L.refx_ra_new()
    calls = {"utg": 0, "arc": 0}

    def align(for_unzip):
        nsk = C.c_uint64(0)
        assert H.oatk_scg_read_alignment(hip.h, db, v, g, for_unzip, C.byref(nsk), None) == 0, hip.L.oatk_hip_last_error(hip.h)

    def utg():
        assert H.oatk_scg_ra_utg_coverage(hip.h, db, v, g, RESIDENT_READS | RESIDENT_ALN, 0) == 0, hip.L.oatk_hip_last_error(hip.h)
        calls["utg"] += 1

    def arc(refine):
        assert H.oatk_scg_ra_arc_coverage(hip.h, db, v, g, RESIDENT_ALN, 0) == 0, hip.L.oatk_hip_last_error(hip.h)
        finish_arcs(L, g, refine)
        calls["arc"] += 1

    def consensus(path):
        fo = libc.fopen(path.encode(), b"w") if path else None
        L.scg_consensus(db, g, 0, 0, fo)
        if fo:
            libc.fclose(fo)

    L.refx_process_unitigs(g)                                                   # :161
    consensus(dev + ".utg.gfa")
    while L.asmg_drop_tip(ag(), 2**31 - 1, tip, 1, 0, 0):                        # :183-192
        pass
    L.refx_process_unitigs(g)
    rnd, updated = 0, 1
    while updated != 0 and rnd < unzip:                                         # :219-239
        rnd += 1
        align(1)
        L.refx_update_utg_cov(g)
        updated = L.refx_multiplex(g, v, int(math.ceil(30000.0 / K)), 10.0, 0.3)
    align(1)                                                                    # :244-246
    arc(0)
    L.asmg_remove_weak_crosslink(ag(), weak, 10, 0, 0)
    L.scg_demultiplex(g)                                                        # :257-261
    align(0)
    utg()
    arc(1)
    consensus(None)
    cleaned = 1
    while cleaned:                                                              # :275-282
        cleaned = L.asmg_pop_bubble(ag(), bubble, 0, 0, 1, 0, 0)
        cleaned += L.asmg_remove_weak_crosslink(ag(), weak, 10, 0, 0)
        cleaned += L.asmg_drop_tip(ag(), 2**31 - 1, tip, 1, 0, 0)
    L.refx_process_unitigs(g)
    align(0)                                                                    # :295-303
    utg()
    arc(1)
    consensus(dev + ".utg.final.gfa")
    assert calls == {"utg": 2, "arc": 3}
    for sfx in (".utg.gfa", ".utg.final.gfa"):
        assert filecmp.cmp(ref + sfx, dev + sfx, shallow=False), sfx
    assert os.path.getsize(dev + ".utg.final.gfa") > 100
    L.refx_ra_destroy(v)
    L.refx_scg_destroy(g)
    L.refx_scmdb_destroy(scm)
    L.refx_srdb_destroy(db)
