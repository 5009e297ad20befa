"""GPU parity of the spanning-triplet scores with the reads SHARDED BY RECORD over several handles (include/oatk_hip_racov.h:
oatk_hip_ra_triplet_scores_sharded; include/oatk_multi.h: oatk_multi_scg_multiplex_plan) against the one-handle call, the Python model and,
through the pipeline, the COMPILED REFERENCE's scg_multiplex.  Every comparison of doubles is bit for bit.  Several handles live on the one
GPU and talk over the in-process communicator group, one thread per handle."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import multiplex_util as MX
import ref_lib as R
import test_gpu_align as GA
import test_gpu_multiplex as TM
import test_gpu_racov as RC
from test_gpu_racov_sharded import BUF_RA_ALN_SID, Ranks, multi_libs
from oatk_amd import HipSyncasm, _lib

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")


@pytest.fixture(scope="module")
def ranks():
    r = Ranks(3)
    yield r
    r.close()


def cut(reads, bounds):
    return [TM.flatten_reads(reads[bounds[r]:bounds[r + 1]]) for r in range(len(bounds) - 1)]


def sharded(ranks, graph, slices):
    return ranks.run(len(slices), lambda r, h, comm: h.ra_triplet_scores_sharded(comm, graph, slices[r]))


def first_read_of_records(reads):
    out = []
    for i, recs in enumerate(reads):
        out += [i] * len(recs)
    return out


def test_synthetic_set_cut_by_read_equals_one_handle(hip, ranks):
    """the synthetic set of test_gpu_multiplex on 2 ranks at every cut point and on 3 ranks at four cuts, empty ranks included"""
    reads = TM.synthetic_reads()
    graph = TM.synthetic_graph()
    whole = TM.flatten_reads(reads)
    trace = []
    m = MX.decide(graph, MX.triplet_table(graph, whole, trace), TM.MAX_N_SCM, TM.MIN_N_R, TM.MIN_D_F)
    one = hip.ra_triplet_scores(graph, whole)
    MX.assert_same_scores(one, m, "one handle")
    # which reads put which key (a key and its mirror are one entry here), from the model's trace
    read_of = first_read_of_records(reads)
    by_key = {}
    for rec, A, M, _ in trace:
        by_key.setdefault(min(A, M), []).append(read_of[rec])
    mix = by_key[min((2, 4), (5, 3))]
    seen = {"assign": 0, "mix": 0}
    cuts = [[0, b, len(reads)] for b in range(len(reads) + 1)]
    cuts += [[0, 20, 40, len(reads)], [0, 17, 17, len(reads)], [0, 0, 19, len(reads)], [0, 16, 18, len(reads)]]
    for bounds in cuts:
        res = sharded(ranks, graph, cut(reads, bounds))
        for r, got in enumerate(res):
            MX.assert_same_scores(got, one, (bounds, r))
        if len(bounds) == 3:
            b = bounds[1]
            seen["assign"] += any(rd[0] < b <= min(rd[1:]) for rd in by_key.values() if len(rd) > 1)
            seen["mix"] += mix[0] < b <= mix[-1]
    print("cuts where the boundary matters:", seen)
    assert seen["assign"] > 0 and seen["mix"] >= 5               # between every two of the six events of the two-strand key


def test_one_rank_equals_the_unsharded_call(hip, ranks):
    graph, whole = TM.synthetic_graph(), TM.flatten_reads(TM.synthetic_reads())
    MX.assert_same_scores(sharded(ranks, graph, [whole])[0], hip.ra_triplet_scores(graph, whole), "one rank")


def raw_calls(ranks, graph, slices, grp=None, resident_rank=None):
    """the C entry point itself, outputs pre-filled with a sentinel: [(rc, n_pair, score, have)] per rank"""
    def fn(r, h, comm):
        g, keep_g = h._racov_graph(graph)
        a, keep_a = h._racov_aln(slices[r])
        off, n = np.full(g.n_utg + 1, 77, np.uint64), C.c_uint64(99)
        p_in, p_out, sc, hv = np.full(16, 77, np.uint64), np.full(16, 77, np.uint64), np.full(16, -7.0), np.full(16, 7, np.uint8)
        fresh = HipSyncasm(0) if r == resident_rank else h       # nothing resident in it
        try:
            rc = fresh.L.oatk_hip_ra_triplet_scores_sharded(fresh.h, comm, C.byref(g), None if r == resident_rank else C.byref(a), off.ctypes.data, 16, C.byref(n),
                                                            p_in.ctypes.data, p_out.ctypes.data, sc.ctypes.data, hv.ctypes.data)
        finally:
            if r == resident_rank:
                fresh.close()
        return rc, n.value, sc, hv

    return ranks.run(len(slices), fn, grp)


def test_a_missing_arc_on_one_rank_is_refused_on_all(hip, ranks):
    """a record of three fragments whose first two have no arc, on the last rank only: OATK_E_ARG everywhere, nothing written, nobody left
    waiting, and the same communicator group serves the next call"""
    reads = TM.synthetic_reads()
    graph = TM.synthetic_graph()
    one = hip.ra_triplet_scores(graph, TM.flatten_reads(reads))
    bad = reads + [[(2.5, [TM.N(TM.fw(TM.D_)), TM.N(TM.fw(TM.A_)), TM.N(TM.fw(TM.B_))]), (2.5, [TM.N(TM.fw(TM.C_))])]]
    for n, bounds in ((2, [0, 30, len(reads)]), (3, [0, 20, 40, len(reads)])):
        grp = ranks.L.oatk_comm_group_create(n)
        try:
            for rc, n_pair, sc, hv in raw_calls(ranks, graph, cut(bad, bounds[:-1] + [len(bad)]), grp=grp):
                assert rc == _lib.E_ARG and n_pair == 99 and (sc == -7.0).all() and (hv == 7).all()
            for rc, n_pair, sc, hv in raw_calls(ranks, graph, cut(reads, bounds), grp=grp):
                assert rc == 0 and n_pair == len(TM.WANT) and MX.same_doubles(sc[:n_pair], one["score"]) and (hv[:n_pair] == 1).all()
        finally:
            ranks.L.oatk_comm_group_destroy(grp)


def test_a_failing_rank_releases_its_peers(ranks):
    """a rank that asks for resident alignments it does not have fails on its own: the group is poisoned and its peer returns an error
    instead of waiting"""
    reads = TM.synthetic_reads()
    res = raw_calls(ranks, TM.synthetic_graph(), cut(reads, [0, 30, len(reads)]), resident_rank=1)
    assert res[1][0] == _lib.E_STATE and res[0][0] != 0
    for rc, n_pair, sc, hv in res:
        assert n_pair == 99 and (sc == -7.0).all() and (hv == 7).all()


@pytest.mark.parametrize("n", [2, 3])
def test_traffic_does_not_grow_with_the_reads(ranks, n):
    """every read of the synthetic set twice: what a rank puts into the collectives is what include/oatk_hip_racov.h documents -- one small
    all-gather (the verdict) and 72 bytes per group of keys -- and has no term in the reads"""
    graph = TM.synthetic_graph()
    reads = TM.synthetic_reads()
    n_grp = len({tuple(sorted((a >> 1, b >> 1))) for (a, b), _ in TM.WANT})
    assert n_grp == len(TM.WANT)

    def fn(slices):
        def one(r, h, comm):
            h.L.oatk_comm_traffic(comm, None, 1)
            h.ra_triplet_scores_sharded(comm, graph, slices[r])
            t = (C.c_uint64 * 8)()
            h.L.oatk_comm_traffic(comm, t, 1)
            return list(t)
        return one

    got = []
    for rd in (reads, [r for r in reads for _ in (0, 1)]):
        bounds = [len(rd) * r // n for r in range(n + 1)]
        t = ranks.run(n, fn(cut(rd, bounds)))
        for r in range(n):
            assert t[r] == [1, 8, n, 72 * n_grp, 0, 0, 0, 0], (len(rd), r, t[r])
        got.append(t)
    assert got[0] == got[1]


@needs_ref
@pytest.mark.parametrize("n", [2, 3])
def test_plan_over_several_handles_matches_reference_through_the_pipeline(n, tmp_path):
    """case 3 of test_gpu_align.CASES: reads from a file into n handles, count, merge, sharded correction, the reference's graph, the alignment
    on every handle; in every unzip round oatk_multi_scg_multiplex_plan BEFORE the reference's scg_multiplex, against its return value and
    against the model's marks"""
    K, S, c, mk = GA.CASES[3]
    L, H = multi_libs()
    Lh = _lib.load()
    reads = mk()
    fa = str(tmp_path / "reads.fa")
    R.write_fasta(reads, fa)
    m = H.oatk_multi_create((C.c_int * n)(*([0] * n)), n)
    assert m
    err = lambda: H.oatk_multi_last_error(m)
    db = H.oatk_sr_db_new(K, S)
    H.oatk_host_debug_window(os.path.getsize(fa) // (3 * n) + 1000)
    try:
        assert H.oatk_multi_sr_read_files(m, db, R._files_arg([fa]), 1) == 0, err()
    finally:
        H.oatk_host_debug_window(0)
    rcc = C.c_int(0)
    scm = H.oatk_multi_collect_syncmer_from_reads(m, db, C.byref(rcc))
    assert rcc.value == 0 and scm, err()
    st = np.zeros(12, np.uint64)
    assert H.oatk_multi_read_error_correction(m, db, scm, 0.02, c, 10 * c, c, 0.35, st.ctypes.data) == 0, err()
    g = L.refx_make_graph(db, scm, c, 0.35)
    assert g
    v = L.refx_ra_new()

    def align(for_unzip):
        nsk = C.c_uint64(0)
        assert H.oatk_multi_scg_read_alignment(m, db, v, g, for_unzip, C.byref(nsk)) == 0, err()

    def held():
        k = []
        for r in range(n):
            d, b = C.c_void_p(), C.c_uint64()
            assert Lh.oatk_hip_buffer(H.oatk_multi_ctx(m, r), BUF_RA_ALN_SID, C.byref(d), C.byref(b)) == 0
            k.append(b.value // 4)
        return k

    def plan(ra, want_rc=0):
        nu = C.cast(g, C.POINTER(RC.Scg)).contents.utg_asmg.contents.n_vtx
        mv, upd, tab = np.full(max(nu, 1), 9, np.uint8), C.c_int(-5), _lib.TripletTable()
        rc = H.oatk_multi_scg_multiplex_plan(m, ra, g, max_n_scm, 10.0, 0.3, mv.ctypes.data, C.byref(upd), C.byref(tab))
        assert rc == want_rc, (rc, err())
        ent = [(tab.l_in[k], tab.l_out[k], tab.val[k]) for k in range(tab.n)] if rc == 0 else None
        if rc == 0:
            H.oatk_triplet_table_free(C.byref(tab))
        return mv[:nu], upd.value, ent

    align(0)
    L.refx_process_unitigs(g)
    align(0)
    max_n_scm = int(math.ceil(30000.0 / K))
    seen = {"updated": 0, "sharded": 0}
    for _ in range(3):
        align(1)
        L.refx_update_utg_cov(g)
        k = held()
        seen["sharded"] += sum(x > 0 for x in k) >= 2
        model = MX.model(MX.flatten_graph(g), MX.flat_aln(GA.flatten(L, v)), max_n_scm, 10.0, 0.3)
        TM.check_plan(plan(v), model, ("handles", n))
        # alignments that are not the last ones written for this graph are refused, and nothing is written
        clone = GA.clone(L, H, v)
        mv, upd, _ = plan(clone, want_rc=_lib.E_STATE)
        assert (mv == 9).all() and upd == -5
        L.refx_ra_destroy(clone)
        updated = L.refx_multiplex(g, v, max_n_scm, 10.0, 0.3)
        assert model["updated"] == updated
        seen["updated"] += updated > 0
        if updated == 0:
            break
    print("handles", n, seen)
    assert seen["updated"] > 0 and seen["sharded"] > 0
    L.refx_ra_destroy(v)
    L.refx_scg_destroy(g)
    L.refx_scmdb_destroy(scm)
    L.refx_srdb_destroy(db)
    H.oatk_multi_destroy(m)
