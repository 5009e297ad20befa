"""GPU parity of the coverage estimates from read alignments with the reads SHARDED BY RECORD over several handles
(include/oatk_hip_racov.h: oatk_hip_ra_utg_coverage_sharded / oatk_hip_ra_arc_coverage_sharded; include/oatk_multi.h:
oatk_multi_scg_ra_utg_coverage / oatk_multi_scg_ra_arc_coverage) against the one-handle calls and the COMPILED REFERENCE's
scg_ra_utg_coverage / scg_ra_arc_coverage (syncasm.c:1882-2147).  Every comparison is exact: doubles bit for bit, covs, iteration counts,
the EM's printed lines.  Several handles live on the one GPU and talk over the in-process communicator group, one thread per handle."""
import ctypes as C
import math
import os
import threading

import numpy as np
import pytest

import ref_lib as R
import test_gpu_align as GA
import test_gpu_racov as RC
from racov_sharded_util import boundary_facts, cut_slices, whole
from oatk_amd import HipSyncasm, _lib

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")

JOIN_S = 120
BUF_RA_ALN_SID = 200            # include/oatk_hip_align.h


class Ranks:
    """n handles on device 0, reused over many collective calls; run(fn) calls fn(rank, handle, comm) on one thread per rank over a fresh
    communicator group and fails if a thread does not come back"""

    def __init__(self, n):
        self.L = _lib.load()
        self.h = [HipSyncasm(0) for _ in range(n)]

    def run(self, n, fn, grp=None):
        L = self.L
        own = grp is None
        if own:
            grp = L.oatk_comm_group_create(n)
        comms = [L.oatk_comm_group_rank(grp, r) for r in range(n)]
        out, errs = [None] * n, []

        def work(r):
            try:
                out[r] = fn(r, self.h[r], comms[r])
            except Exception as ex:                      # noqa: BLE001
                errs.append((r, ex))

        th = [threading.Thread(target=work, args=(r,)) for r in range(n)]
        [t.start() for t in th]
        [t.join(timeout=JOIN_S) for t in th]
        assert not any(t.is_alive() for t in th), "a rank waits for a peer that is gone"
        for c in comms:
            L.oatk_comm_destroy(c)
        if own:
            L.oatk_comm_group_destroy(grp)
        assert not errs, errs
        return out

    def close(self):
        for h in self.h:
            h.close()


@pytest.fixture(scope="module")
def ranks():
    r = Ranks(3)
    yield r
    r.close()


def sharded_pair(ranks, graph, slices, verbose=0):
    """both sharded calls on len(slices) ranks: ([(avg, n_iter)] per rank, [arc] per rank)"""
    n = len(slices)
    utg = ranks.run(n, lambda r, h, comm: h.ra_utg_coverage_sharded(comm, graph, slices[r][0], slices[r][1], verbose))
    arc = ranks.run(n, lambda r, h, comm: h.ra_arc_coverage_sharded(comm, graph, slices[r][0]))
    return utg, arc


def same_doubles(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def arcs_as_the_reference_leaves_them(L, syn, arc):
    """the sums written like scg_ra_arc_coverage writes them (:2131-2138), then its asmg_arc_fix_cov (refine 0): arc[].cov"""
    snap = RC.covs(syn.g)
    a = RC.asmg(syn.g)
    for i in range(a.n_arc):
        if not a.arc[i].del_:
            a.arc[i].cov = int(np.uint32(arc[i]))
    RC.finish_arcs(L, syn.g, 0)
    got = RC.covs(syn.g)[1]
    RC.restore(syn.g, snap)
    return got


@needs_ref
def test_synthetic_set_cut_by_read_equals_one_handle_and_reference(hip, ranks, capfd):
    """the synthetic set of test_gpu_racov on 2 ranks at every cut point and on 3 ranks (one cut with an empty rank in the middle, one with an
    empty first rank): utg_cov, n_iter, arc_cov and rank 0's EM lines equal the one-handle call's and the compiled reference's"""
    L, H = RC.libs()
    reads = RC.synthetic_reads()
    syn = RC.Synthetic(L)
    try:
        # the reference and the one-handle call
        snap = RC.covs(syn.g)
        capfd.readouterr()
        L.scg_ra_utg_coverage(syn.g, syn.db, syn.v, 3)
        ref_lines = RC.em_lines(capfd.readouterr().err)
        ref_utg = RC.covs(syn.g)[0]
        on_utg = RC.covs(syn.g)                  # the arc coverage on top of the reference's unitig coverage (asmg_arc_fix_cov reads it)
        L.scg_ra_arc_coverage(syn.g, syn.db, syn.v, 0, 0)
        ref_arc = RC.covs(syn.g)[1]
        RC.restore(syn.g, on_utg)
        assert ref_arc.max() > 0
        one_avg, one_it = hip.ra_utg_coverage(syn.graph, syn.flat_aln(), syn.chains, verbose=3)
        one_lines = RC.em_lines(capfd.readouterr().err)
        one_arc = hip.ra_arc_coverage(syn.graph, syn.flat_aln())
        assert one_lines == ref_lines and np.array_equal(one_avg.astype(np.uint32), ref_utg) and one_it >= 3
        for i, x in RC.WANT_ARC.items():
            assert one_arc[i] == x
        live = np.array([a[4] == 0 for a in RC.ARCS])
        seen = {"frac": 0, "link": 0, "self": 0}
        cuts = [[0, b, len(reads)] for b in range(len(reads) + 1)]
        cuts += [[0, 50, 100, len(reads)], [0, 90, 90, len(reads)], [0, 0, 146, len(reads)], [0, 141, 146, len(reads)]]
        for bounds in cuts:
            slices = cut_slices(reads, bounds)
            capfd.readouterr()
            utg, arc = sharded_pair(ranks, syn.graph, slices, verbose=3)
            lines = RC.em_lines(capfd.readouterr().err)
            assert lines == ref_lines, (bounds, lines[-2:], ref_lines[-2:])          # rank 0's, once
            for r in range(len(slices)):
                assert same_doubles(utg[r][0], one_avg), (bounds, r, utg[r][0], one_avg)
                assert utg[r][1] == one_it, (bounds, r)
                assert same_doubles(arc[r], one_arc), (bounds, r, arc[r], one_arc)
                assert np.array_equal(utg[r][0].astype(np.uint32), ref_utg)
            assert np.array_equal(arcs_as_the_reference_leaves_them(L, syn, arc[0]), ref_arc), bounds
            if len(bounds) == 3:
                f = boundary_facts(reads, bounds[1])
                seen["frac"] += bool(f[0])
                seen["link"] += bool(f[1])
                seen["self"] += bool(f[2])
        print("cuts where the boundary matters:", seen, "reference arc covs", ref_arc[live])
        assert seen["frac"] > 0 and seen["link"] > 0 and seen["self"] > 0
    finally:
        syn.close()


@needs_ref
def test_one_rank_equals_the_unsharded_call(hip, ranks):
    L, _ = RC.libs()
    syn = RC.Synthetic(L)
    try:
        one_avg, one_it = hip.ra_utg_coverage(syn.graph, syn.flat_aln(), syn.chains)
        one_arc = hip.ra_arc_coverage(syn.graph, syn.flat_aln())
        utg, arc = sharded_pair(ranks, syn.graph, [whole(RC.synthetic_reads())])
        assert same_doubles(utg[0][0], one_avg) and utg[0][1] == one_it and same_doubles(arc[0], one_arc)
    finally:
        syn.close()


def raw_calls(ranks, graph, slices, caps=None, grp=None):
    """the C entry points themselves (return codes instead of exceptions), outputs pre-filled with a sentinel: [(rc_utg, utg, it, rc_arc, arc)]"""
    n = len(slices)

    def fn(r, h, comm):
        g, keep_g = h._racov_graph(graph)
        a, keep_a = h._racov_aln(slices[r][0])
        k0, k1 = np.ascontiguousarray(slices[r][1][0], np.uint64), np.ascontiguousarray(slices[r][1][1], np.uint64)
        rd = _lib.RacovReads(len(k0) - 1, k0.ctypes.data, k1.ctypes.data)
        utg, arc, it = np.full(g.n_utg, -7.0), np.full(g.n_arc, -7.0), C.c_uint64(99)
        if caps:
            h._check(h.L.oatk_hip_debug_racov_cap(h.h, caps[r]), "oatk_hip_debug_racov_cap")
        try:
            rc_u = h.L.oatk_hip_ra_utg_coverage_sharded(h.h, comm, C.byref(g), C.byref(rd), C.byref(a), 0, utg.ctypes.data, C.byref(it))
        finally:
            if caps:
                h._check(h.L.oatk_hip_debug_racov_cap(h.h, 0), "oatk_hip_debug_racov_cap")
        rc_a = h.L.oatk_hip_ra_arc_coverage_sharded(h.h, comm, C.byref(g), C.byref(a), arc.ctypes.data)
        return rc_u, utg, it.value, rc_a, arc

    return ranks.run(n, fn, grp)


@needs_ref
def test_refusal_and_error_agree_across_ranks(hip, ranks):
    """the LCS working limit exceeded on one rank only: OATK_E_SPLIT on every rank; an alignment with a missing arc on one rank only:
    OATK_E_ARG on every rank; no output array is touched, nobody is left waiting, and the communicator group stays usable"""
    L, _ = RC.libs()
    reads = RC.synthetic_reads()
    syn = RC.Synthetic(L)
    try:
        one_avg, _ = hip.ra_utg_coverage(syn.graph, syn.flat_aln(), syn.chains)
        one_arc = hip.ra_arc_coverage(syn.graph, syn.flat_aln())
        # B+ -> A+ is no arc of the graph
        bad = reads + [([25, 26, 27, 28, 29, 20, 21, 22, 23, 24], [(10.0, [(RC.B_ << 1, 5, 9, 0, 4), (RC.A_ << 1, 5, 9, 5, 9)])])]
        for n, bounds in ((2, [0, 100, len(reads)]), (3, [0, 60, 120, len(reads)])):
            grp = ranks.L.oatk_comm_group_create(n)
            try:
                good = cut_slices(reads, bounds)
                res = raw_calls(ranks, syn.graph, good, caps=[0] * (n - 1) + [1], grp=grp)
                for rc_u, utg, it, rc_a, arc in res:
                    assert rc_u == _lib.E_SPLIT and np.all(utg == -7.0) and it in (0, 99)
                    assert rc_a == 0 and same_doubles(arc, one_arc)
                res = raw_calls(ranks, syn.graph, cut_slices(bad, bounds[:-1] + [len(bad)]), grp=grp)
                for rc_u, utg, it, rc_a, arc in res:
                    assert rc_u == 0
                    assert rc_a == _lib.E_ARG and np.all(arc == -7.0)
                # both verdicts were everybody's: the same group serves the next call
                res = raw_calls(ranks, syn.graph, good, grp=grp)
                for rc_u, utg, it, rc_a, arc in res:
                    assert rc_u == 0 and rc_a == 0 and same_doubles(utg, one_avg) and same_doubles(arc, one_arc)
            finally:
                ranks.L.oatk_comm_group_destroy(grp)
    finally:
        syn.close()


@needs_ref
def test_a_failing_rank_releases_its_peers(ranks):
    """a rank that asks for resident alignments it does not have fails on its own (call order): the group is poisoned and its peer returns
    an error instead of waiting"""
    L, _ = RC.libs()
    reads = RC.synthetic_reads()
    syn = RC.Synthetic(L)
    try:
        slices = cut_slices(reads, [0, 75, len(reads)])

        def fn(r, h, comm):
            g, keep_g = h._racov_graph(syn.graph)
            a, keep_a = h._racov_aln(slices[r][0])
            arc = np.full(g.n_arc, -7.0)
            fresh = HipSyncasm(0) if r == 1 else h              # nothing resident in it
            try:
                return fresh.L.oatk_hip_ra_arc_coverage_sharded(fresh.h, comm, C.byref(g), None if r == 1 else C.byref(a), arc.ctypes.data), arc
            finally:
                if r == 1:
                    fresh.close()

        res = ranks.run(2, fn)
        assert res[1][0] == _lib.E_STATE and res[0][0] != 0
        assert np.all(res[0][1] == -7.0) and np.all(res[1][1] == -7.0)
    finally:
        syn.close()


def traffic_of(ranks, graph, slices):
    """oatk_comm_traffic of every rank for the unitig call and for the arc call, reset before each: ([out8] per rank, n_iter, [out8] per rank)"""
    n = len(slices)

    def utg(r, h, comm):
        h.L.oatk_comm_traffic(comm, None, 1)
        _, it = h.ra_utg_coverage_sharded(comm, graph, slices[r][0], slices[r][1])
        t = (C.c_uint64 * 8)()
        h.L.oatk_comm_traffic(comm, t, 1)
        return list(t), it

    def arc(r, h, comm):
        h.L.oatk_comm_traffic(comm, None, 1)
        h.ra_arc_coverage_sharded(comm, graph, slices[r][0])
        t = (C.c_uint64 * 8)()
        h.L.oatk_comm_traffic(comm, t, 1)
        return list(t)

    u = ranks.run(n, utg)
    return [x[0] for x in u], u[0][1], ranks.run(n, arc)


def traffic_formula(n_ranks, m_scm, n_utg, n_link, n_iter):
    """DESIGN.md 8.8, per rank: [small all-gathers, bytes, array all-gathers, bytes, all-reduces, bytes, exchanges, bytes]"""
    passes = min(n_iter + 1, 1000)
    return ([3, 24, n_ranks * passes, 8 * n_utg * passes, 1, 4 * m_scm, 0, 0],
            [1, 8, n_ranks, 18 * n_link, 0, 0, 0, 0])


@needs_ref
@pytest.mark.parametrize("n", [2, 3])
def test_traffic_does_not_grow_with_the_reads(ranks, n):
    """every read of the synthetic set twice (same graph, twice the alignments and chains): what a rank puts into the collectives is the
    formula of DESIGN.md 8.8 in m_scm, n_utg x EM passes, n_link and the number of ranks -- it has no term in the reads"""
    L, _ = RC.libs()
    syn = RC.Synthetic(L)
    try:
        reads = RC.synthetic_reads()
        twice = [r for r in reads for _ in (0, 1)]
        m_scm, n_utg = sum(len(u) for u in RC.UTG), len(RC.UTG)
        n_link = max(a[2] for a in RC.ARCS) + 1
        got = []
        for rd in (reads, twice):
            bounds = [len(rd) * r // n for r in range(n + 1)]
            t_utg, it, t_arc = traffic_of(ranks, syn.graph, cut_slices(rd, bounds))
            want_utg, want_arc = traffic_formula(n, m_scm, n_utg, n_link, it)
            for r in range(n):
                assert t_utg[r] == want_utg, (len(rd), r, t_utg[r], want_utg)
                assert t_arc[r] == want_arc, (len(rd), r, t_arc[r], want_arc)
            passes = min(it + 1, 1000)
            got.append((t_utg[0][1], t_utg[0][3] // passes, t_utg[0][5], t_arc[0][1] + t_arc[0][3]))
            print(len(rd), "reads:", "EM passes", passes, "bytes per rank: utg", t_utg[0][1] + t_utg[0][3] + t_utg[0][5], "arc", t_arc[0][1] + t_arc[0][3])
        assert got[0] == got[1]                  # bytes outside the EM, bytes per EM pass, the arc call's bytes: unchanged
    finally:
        syn.close()


# ---- through the pipeline, resident ----
def multi_libs():
    L, _ = RC.libs()
    return L, _lib.load_host()


PIPE_CASES = [2, 3, 4]          # test_gpu_align.CASES: 3 has reads with several alignments, 2 and 4 records of several fragments


@needs_ref
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("case", PIPE_CASES)
def test_coverage_over_several_handles_matches_reference_through_the_pipeline(case, n, tmp_path):
    """reads from a file into n handles, count, merge, sharded correction, the reference's graph and tail, the alignment on every handle:
    after every alignment both N-handle calls against the compiled reference on the same state, every vtx[].cov and arc[].cov, refine 0 and 1"""
    K, S, c, mk = GA.CASES[case]
    L, H = multi_libs()
    Lh = _lib.load()
    reads = mk()
    fa = str(tmp_path / "reads.fa")
    R.write_fasta(reads, fa)
    m = H.oatk_multi_create((C.c_int * n)(*([0] * n)), n)
    assert m
    err = lambda: H.oatk_multi_last_error(m)
    db = H.oatk_sr_db_new(K, S)
    H.oatk_host_debug_window(os.path.getsize(fa) // (3 * n) + 1000)          # about three windows per handle
    try:
        assert H.oatk_multi_sr_read_files(m, db, R._files_arg([fa]), 1) == 0, err()
    finally:
        H.oatk_host_debug_window(0)
    for r in range(n):
        first, cnt = C.c_uint64(), C.c_uint64()
        H.oatk_multi_range(m, r, C.byref(first), C.byref(cnt))
        assert cnt.value > 0, (r, "a handle without reads")
    rcc = C.c_int(0)
    scm = H.oatk_multi_collect_syncmer_from_reads(m, db, C.byref(rcc))
    assert rcc.value == 0 and scm, err()
    st = np.zeros(12, np.uint64)
    assert H.oatk_multi_read_error_correction(m, db, scm, 0.02, c, 10 * c, c, 0.35, st.ctypes.data) == 0, err()
    g = L.refx_make_graph(db, scm, c, 0.35)
    assert g
    v = L.refx_ra_new()
    seen = {"multi_aln": 0, "multi_frg": 0, "calls": 0}

    def held():
        k = []
        for r in range(n):
            d, b = C.c_void_p(), C.c_uint64()
            assert Lh.oatk_hip_buffer(H.oatk_multi_ctx(m, r), BUF_RA_ALN_SID, C.byref(d), C.byref(b)) == 0
            k.append(b.value // 4)
        return k

    def align(for_unzip):
        nsk = C.c_uint64(0)
        assert H.oatk_multi_scg_read_alignment(m, db, v, g, for_unzip, C.byref(nsk)) == 0, err()
        RC.tally(L, v, seen)
        k = held()
        print("for_unzip", for_unzip, "alignments per handle", k)
        assert sum(k) == C.cast(v, C.POINTER(C.c_size_t))[0]
        # an alignment round that leaves no alignment at all (the for_unzip filter can) is still compared -- the warning, the arcs' zeros --
        # but shows nothing about sharding: every other call must have found alignments on two handles or more
        if sum(k):
            assert sum(x > 0 for x in k) >= 2, "fewer than two handles hold alignments"
            seen["sharded_calls"] = seen.get("sharded_calls", 0) + 1
        # the unitig coverage
        snap = RC.covs(g)
        assert H.oatk_multi_scg_ra_utg_coverage(m, db, v, g, 0) == 0, err()
        got = RC.covs(g)
        RC.restore(g, snap)
        L.scg_ra_utg_coverage(g, db, v, 0)
        RC.assert_covs(got, RC.covs(g), ("utg", n))
        # the arc coverage, refine 0 and 1
        for refine in (0, 1):
            snap = RC.covs(g)
            assert H.oatk_multi_scg_ra_arc_coverage(m, db, v, g, 0) == 0, err()
            RC.finish_arcs(L, g, refine)
            got = RC.covs(g)
            RC.restore(g, snap)
            L.scg_ra_arc_coverage(g, db, v, refine, 0)
            RC.assert_covs(got, RC.covs(g), ("arc", refine, n))
            if refine == 0:
                RC.restore(g, snap)

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
    print("case", case, "handles", n, seen)
    assert seen["calls"] >= 4 and seen["sharded_calls"] == seen["calls"]
    if case == 3:
        assert seen["multi_aln"] > 0            # reads with two or more alignments: EM blocks of two or more members
    assert seen["multi_frg"] > 0                # records with two or more fragments: arc duplets
    # alignments that are not the last ones written for this graph are refused, and nothing is written
    snap = RC.covs(g)
    clone = GA.clone(L, H, v)
    assert H.oatk_multi_scg_ra_utg_coverage(m, db, clone, g, 0) == _lib.E_STATE
    assert H.oatk_multi_scg_ra_arc_coverage(m, db, clone, g, 0) == _lib.E_STATE
    RC.assert_covs(RC.covs(g), snap, "foreign alignments")
    L.refx_ra_destroy(clone)
    L.refx_ra_destroy(v)
    L.refx_scg_destroy(g)
    L.refx_scmdb_destroy(scm)
    L.refx_srdb_destroy(db)
    H.oatk_multi_destroy(m)
