"""GPU: the strings of scg_consensus for reads sharded over several handles (oatk_hip_consensus_strings_sharded, csrc/cons_str.hpp: cstr_kmer_kernel, and
liboatk_host.so: oatk_multi_consensus / oatk_multi_scg_consensus) against ONE handle holding all the reads, byte for byte -- the one-handle text is pinned to the
compiled reference by tests/test_gpu_cons_strings.py.  Single pieces of every selected syncmer, whole unitigs with length-only and refused sequences, the host
adaptor on the reference's graph against scg_consensus itself, and what the call costs: one all-reduce of the k-mer table per consensus, nothing afterwards.
The ranks are threads of this process, each with its own handle on the test box's one GPU, over the in-process communicator group."""
import ctypes as C
import threading

import numpy as np
import pytest

import cons_util as CU
import ref_lib as R
import test_gpu_ec as T
from oatk_amd import HipSyncasm, _lib, pack_reads

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")
NONE64 = 0xFFFFFFFFFFFFFFFF
A = 0.35


class Ranks:
    """one handle and one communicator of the in-process group per shard; each(fn) runs fn(rank, handle, comm) on a thread per rank"""

    def __init__(self, reads, bounds, K, S):
        self.L = _lib.load()
        self.reads, self.bounds, self.K, self.S = reads, bounds, K, S
        self.world = len(bounds) - 1
        self.grp = self.L.oatk_comm_group_create(self.world)
        assert self.grp
        self.h = [HipSyncasm(0) for _ in range(self.world)]
        self.comm = [self.L.oatk_comm_group_rank(self.grp, r) for r in range(self.world)]
        assert all(self.comm)

    def each(self, fn):
        out, errs = [None] * self.world, []

        def work(rank):
            try:
                out[rank] = fn(rank, self.h[rank], self.comm[rank])
            except Exception as ex:                      # noqa: BLE001
                errs.append((rank, ex))

        th = [threading.Thread(target=work, args=(r,)) for r in range(self.world)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in th), "a rank hangs in a collective"
        assert not errs, errs
        return out

    def corrected(self, c):
        def fn(rank, h, comm):
            lo, hi = self.bounds[rank], self.bounds[rank + 1]
            h.scan_host(*pack_reads(self.reads[lo:hi]), self.K, self.S, sid0=lo)
            h.count()
            h.merge_counts(comm)
            h.ec_sharded(comm, 0.02, c, A)
        self.each(fn)
        return self

    def consensus(self, c):
        self.each(lambda rank, h, comm: h.consensus_sharded(comm, c))
        return self

    def strings(self, seq_off, pv, pb, hoco, want=None):
        return self.each(lambda rank, h, comm: h.consensus_strings_sharded(comm, seq_off, pv, pb, hoco, want) + (h.cons_strings,))

    def traffic(self, reset=False):
        out = []
        for c in self.comm:
            t = (C.c_uint64 * 8)()
            self.L.oatk_comm_traffic(c, t, 1 if reset else 0)
            out.append([int(x) for x in t])
        return out

    def close(self):
        for c in self.comm:
            self.L.oatk_comm_destroy(c)
        for h in self.h:
            h.close()
        self.L.oatk_comm_group_destroy(self.grp)


def one_handle(hip, reads, K, S, c):
    hip.scan_host(*pack_reads(reads), K, S)
    hip.count()
    hip.ec_graph(light_c=c)
    hip.ec(0.02, c, A)
    hip.consensus(c)


def raw_sharded(h, comm, seq_off, piece_v, piece_beg, hoco=0):
    """the return code of the entry point itself for a plan as given (nothing checked on this side)"""
    seq_off, piece_v, piece_beg = np.asarray(seq_off, np.uint64), np.asarray(piece_v, np.uint64), np.asarray(piece_beg, np.int32)
    plan = _lib.ConsPlan(max(len(seq_off) - 1, 0), len(piece_v), seq_off.ctypes.data, piece_v.ctypes.data, piece_beg.ctypes.data, None)
    tot, ref = C.c_uint64(), C.c_uint64()
    return h.L.oatk_hip_consensus_strings_sharded(h.h, comm, C.byref(plan), hoco, C.byref(tot), C.byref(ref))


def owners(hip, bounds, ids):
    """from one handle's CONS_FIRST: per shard, the strands of the first occurrences it holds among the syncmers `ids`"""
    slot = hip.fetch("CONS_SLOT")[np.asarray(ids, np.int64)]
    assert (slot != 0xFFFFFFFF).all()
    first = hip.fetch("CONS_FIRST")[slot.astype(np.int64)]
    first = first[first != np.uint64(NONE64)]
    sid = (first >> np.uint64(32)).astype(np.int64)
    strand = (first & np.uint64(1)).astype(np.int64)
    return [strand[(sid >= bounds[r]) & (sid < bounds[r + 1])] for r in range(len(bounds) - 1)]


def assert_not_blind(hip, bounds, ids, long_runs=True):
    own = owners(hip, bounds, ids)
    for r in range(len(bounds) - 1):
        assert (len(own[r]) > 0) == (bounds[r + 1] > bounds[r]), ("owners per shard", [len(o) for o in own])
    others = np.concatenate(own[1:])
    assert (others == 0).any() and (others == 1).any(), "both strands among the syncmers rank 0 does not hold"
    if long_runs:
        assert int(hip.fetch("CONS_RL").max()) > 255                        # run lengths past the 255 escape are in the table
    return [len(o) for o in own]


def same_everywhere(got, want):
    """the four arrays on every rank against one handle's"""
    wb, woff, wlen, wst, wcs = want
    for r, (b, off, length, status, cs) in enumerate(got):
        assert b.tobytes() == wb.tobytes(), ("CONS_STR", r)
        assert np.array_equal(off, woff) and np.array_equal(length, wlen) and np.array_equal(status, wst), r
        assert cs == wcs, r


PIECE_CASES = [
    ("long", 101, 11, 4, (0, 3, 8, 200)),
    ("long", 101, 11, 4, (0, 3, 3, 8, 200)),                              # one shard empty
    ("late", 1501, 31, 4, (0, 2, 6, 150)),                                 # rows longer than 1024 codes: a lane writes a second word
]


@pytest.mark.parametrize("kind,K,S,c,bounds", PIECE_CASES)
def test_pieces_equal_one_handle(hip, kind, K, S, c, bounds):
    """one plan, one piece per sequence: every selected syncmer x rev x beg in {0, 9, K - 1, -4}, hoco and base space"""
    reads = CU.long_run_reads(104, 101) if kind == "long" else CU.late_run_reads(1508, 1501)
    assert len(reads) == bounds[-1]
    one_handle(hip, reads, K, S, c)
    ids = hip.fetch("CONS_SEL")
    assert len(ids) > (20 if kind == "long" else 5)
    print("owners per shard:", assert_not_blind(hip, bounds, ids), "of", len(ids))
    begs = (0, 9, K - 1, -4)
    v = np.repeat(np.repeat(ids.astype(np.uint64), 2) * 2 + np.tile(np.arange(2, dtype=np.uint64), len(ids)), len(begs))
    beg = np.tile(np.array(begs, np.int32), 2 * len(ids))
    seq_off = np.arange(len(v) + 1, dtype=np.uint64)
    want = {hoco: hip.consensus_strings(seq_off, v, beg, hoco) + (hip.cons_strings,) for hoco in (1, 0)}
    assert int(want[0][2].max()) > K + 255 and not want[0][3].any()
    rk = Ranks(reads, bounds, K, S)
    try:
        rk.corrected(c).consensus(c)
        for hoco in (1, 0):
            same_everywhere(rk.strings(seq_off, v, beg, hoco), want[hoco])
        # the table itself: the same on every rank, as wide as the header says, a row of zeros exactly where there is no first occurrence
        tabs = rk.each(lambda rank, h, comm: h.fetch("CONS_KMER"))
        stride = 8 * ((K + 31) // 32)
        assert len(tabs[0]) == len(ids) * stride and all(t.tobytes() == tabs[0].tobytes() for t in tabs)
        rows = tabs[0].reshape(len(ids), stride)
        assert np.array_equal(rows.any(axis=1), hip.fetch("CONS_FIRST") != np.uint64(NONE64))
    finally:
        rk.close()


def unitig_plan(hip, reads, K, S, c):
    """the plan of tests/test_gpu_cons_strings.py::test_unitigs_equal_the_reference, from one handle: every live unitig of the reference's graph and its reverse
    complement, positions from oatk_calc_syncmer_overlap, the skip loop"""
    import test_gpu_cons_strings as TS
    from test_gpu_dropin import device_dbs
    L, H = TS.libs()
    db, scm = device_dbs(hip, reads, K, S)
    TS.correct(hip, H, db, scm, c)
    hip.consensus(c)
    rc = C.c_int(0)
    ov = H.oatk_overlap_fetch(hip.h, C.byref(rc))
    assert rc.value == 0 and ov
    g = L.refx_make_graph(db, scm, c, A)
    L.refx_process_unitigs(g)
    lists = []
    for v in TS.unitig_lists(L, g):
        lists += [v, np.ascontiguousarray(v[::-1] ^ np.uint64(1))]
    plan = [TS.pieces_of(H, ov, v, K) for v in lists]
    H.oatk_overlap_destroy(ov)
    L.refx_scg_destroy(g)
    L.refx_scmdb_destroy(scm)
    L.refx_srdb_destroy(db)
    seq_off = np.concatenate([[0], np.cumsum([len(p) for p in plan])]).astype(np.uint64)
    flat = [x for p in plan for x in p]
    pv, pb = np.array([x[0] for x in flat], np.uint64), np.array([x[1] for x in flat], np.int32)
    assert len(lists) >= 2 and max(len(v) for v in lists) >= 3 and any(len(p) < len(v) for p, v in zip(plan, lists))
    assert ((pb > 0) & (pb < K)).any() and (pv & np.uint64(1)).any()
    return seq_off, pv, pb


@needs_ref
def test_unitigs_equal_one_handle(hip):
    K, S, c, mk = T.CASES[6]
    bounds = (0, 6, 20, 300)
    reads = mk()
    assert len(reads) == bounds[-1]
    seq_off, pv, pb = unitig_plan(hip, reads, K, S, c)
    n_seq = len(seq_off) - 1
    one_handle(hip, reads, K, S, c)
    sel = hip.fetch("CONS_SEL")
    cov = hip.fetch("EC_SCM_COV")
    print("owners per shard:", assert_not_blind(hip, bounds, np.unique(pv >> np.uint64(1)), long_runs=False), "of the plan's syncmers")
    drop = np.ones(n_seq, np.uint8)
    drop[n_seq // 2] = 0                                                 # one sequence length only
    want = {hoco: hip.consensus_strings(seq_off, pv, pb, hoco) + (hip.cons_strings,) for hoco in (1, 0)}
    want_drop = hip.consensus_strings(seq_off, pv, pb, 0, want_bytes=drop) + (hip.cons_strings,)
    assert not want[0][3].any() and int(want_drop[2][n_seq // 2]) > 0 and len(want_drop[0]) == len(want[0][0]) - int(want[0][2][n_seq // 2])
    # a higher min_cov on both sides: the plan's weakest syncmer loses its consensus and its sequences are refused
    used = np.unique(pv >> np.uint64(1)).astype(np.int64)
    hi = int(cov[used].min()) + 1
    assert hi <= int(cov[sel.astype(np.int64)].max())
    hip.consensus(hi)
    want_hi = hip.consensus_strings(seq_off, pv, pb, 0) + (hip.cons_strings,)
    assert want_hi[3].any() and not want_hi[3].all() and want_hi[4][1] == int(want_hi[3].sum()) and (want_hi[2][want_hi[3] != 0] == np.uint64(NONE64)).all()
    rk = Ranks(reads, bounds, K, S)
    try:
        rk.corrected(c).consensus(c)
        for hoco in (1, 0):
            same_everywhere(rk.strings(seq_off, pv, pb, hoco), want[hoco])
        same_everywhere(rk.strings(seq_off, pv, pb, 0, drop), want_drop)
        rk.consensus(hi)
        same_everywhere(rk.strings(seq_off, pv, pb, 0), want_hi)
    finally:
        rk.close()


def test_traffic_and_state(hip):
    K, S, c, bounds = 101, 11, 4, (0, 3, 8, 200)
    reads = CU.long_run_reads(104, 101)
    one_handle(hip, reads, K, S, c)
    ids = hip.fetch("CONS_SEL").astype(np.uint64)
    n_scm = hip.info()["n_scm"]
    stride = 8 * ((K + 31) // 32)
    plan_a = (np.arange(len(ids) + 1, dtype=np.uint64), ids << np.uint64(1), np.zeros(len(ids), np.int32))
    plan_b = (np.array([0, 3, 7], np.uint64), (ids[:7] << np.uint64(1)) | np.uint64(1), np.array([-4, 9, 0, 50, K - 1, 0, 0], np.int32))
    want_a = hip.consensus_strings(*plan_a, 0) + (hip.cons_strings,)
    want_b = hip.consensus_strings(*plan_b, 0) + (hip.cons_strings,)
    good = int(ids[0]) << 1
    rk = Ranks(reads, bounds, K, S)
    try:
        rk.corrected(c)
        # the one-handle call on a sharded handle: still refused
        plan = _lib.ConsPlan(1, 1, plan_a[0].ctypes.data, plan_a[1].ctypes.data, plan_a[2].ctypes.data, None)
        tot, ref = C.c_uint64(), C.c_uint64()
        rk.consensus(c)
        for h in rk.h:
            assert h.L.oatk_hip_consensus_strings(h.h, C.byref(plan), 0, C.byref(tot), C.byref(ref)) == _lib.E_STATE
        # the first call after a consensus: exactly one all-reduce, of the table's bytes; nothing else
        rk.traffic(reset=True)
        same_everywhere(rk.strings(*plan_a, 0), want_a)
        for t in rk.traffic(reset=True):
            assert t == [0, 0, 0, 0, 1, len(ids) * stride, 0, 0], t
        # another plan on the same consensus: no collective at all, and the right text
        same_everywhere(rk.strings(*plan_b, 0), want_b)
        for t in rk.traffic(reset=True):
            assert t == [0] * 8, t
        # bad plans: OATK_E_ARG on every rank, nobody left waiting, and the handles go on working
        bad = [([0, 1], [n_scm << 1], [0]), ([0, 1], [good], [K]), ([0, 2, 1, 3], [good] * 3, [0] * 3), ([0, 1, 2], [good] * 3, [0] * 3)]
        for b in bad:
            assert rk.each(lambda rank, h, comm: raw_sharded(h, comm, *b)) == [_lib.E_ARG] * rk.world
        # ranks that disagree about the plan: the one with the bad plan is refused, the others are served
        assert rk.each(lambda rank, h, comm: raw_sharded(h, comm, *(bad[1] if rank == 1 else ([0, 1], [good], [0])))) == [_lib.OK, _lib.E_ARG, _lib.OK]
        same_everywhere(rk.strings(*plan_a, 0), want_a)
        for t in rk.traffic(reset=True):
            assert t == [0] * 8, t
        # a new consensus drops the table: one more all-reduce; and a bad plan on the first call after it still makes the table
        rk.consensus(c)
        rk.traffic(reset=True)
        assert rk.each(lambda rank, h, comm: raw_sharded(h, comm, *bad[0])) == [_lib.E_ARG] * rk.world
        for t in rk.traffic(reset=True):
            assert t == [0, 0, 0, 0, 1, len(ids) * stride, 0, 0], t
        same_everywhere(rk.strings(*plan_b, 0), want_b)
        for t in rk.traffic(reset=True):
            assert t == [0] * 8, t
    finally:
        rk.close()
    # without oatk_hip_consensus_sharded: OATK_E_STATE (a call-order error: this group is not used again)
    rk = Ranks(reads, bounds, K, S)
    try:
        rk.corrected(c)
        assert rk.each(lambda rank, h, comm: raw_sharded(h, comm, [0, 1], [good], [0])) == [_lib.E_STATE] * rk.world
    finally:
        rk.close()


@needs_ref
@pytest.mark.parametrize("n", [2, 3])
def test_adaptor_over_several_handles_equals_scg_consensus(hip, tmp_path, n):
    """oatk_multi_read_error_correction, oatk_multi_consensus, oatk_multi_overlap_fetch and oatk_multi_scg_consensus on one copy of the reference's graph, the
    reference's scg_consensus on the other: every flattened array, hoco and base space, the GFA lines, and a refusal that leaves graph and file as they were"""
    import ec_util as E
    from test_gpu_cons_strings import GRAPH_FIELDS, gfa_lines, same_graph
    from test_gpu_ec_seq_sharded import ARC_F, MAX_EDIST, multi_setup
    K, S, c, mk = T.CASES[0]
    reads = mk()
    fa = str(tmp_path / "reads.fa")
    with open(fa, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b">r%d\n" % i + r + b"\n")
    L, H = R.lib(), _lib.load_host()
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    m, db, scm = multi_setup(H, n, fa, K, S)
    try:
        st = np.zeros(12, np.uint64)
        assert H.oatk_multi_read_error_correction(m, db, scm, MAX_EDIST, c, 10 * c, c, ARC_F, st.ctypes.data) == 0, H.oatk_multi_last_error(m)
        assert H.oatk_multi_consensus(m, c) == 0, H.oatk_multi_last_error(m)
        rc = C.c_int(0)
        ov = H.oatk_multi_overlap_fetch(m, c, C.byref(rc))
        assert rc.value == 0 and ov, H.oatk_multi_last_error(m)
        graphs = []
        for _ in range(2):
            g = L.refx_make_graph(db, scm, c, ARC_F)
            L.refx_process_unitigs(g)
            graphs.append(g)
        mine, ref = graphs
        same_graph(E.flatten_graph(mine), E.flatten_graph(ref))
        for hoco in (1, 0):
            assert H.oatk_multi_scg_consensus(m, ov, db, mine, hoco, 1, None) == 0, H.oatk_multi_last_error(m)
            L.refx_consensus(db, ref, hoco, 1)
            G = E.flatten_graph(ref)
            same_graph(E.flatten_graph(mine), G)
            live = G["vtx_del"] == 0
            assert live.sum() >= 2 and (G["vtx_len"][live] >= K).all() and len(G["seq"]) == int(G["vtx_len"][live].sum())
            assert (G["arc_ls"][:G["n_arc"]][G["arc_del"][:G["n_arc"]] == 0] > 0).any()
        # the GFA lines, on a graph whose coverages are set
        path = str(tmp_path / "out.gfa").encode()
        fo = libc.fopen(path, b"w")
        assert fo
        assert H.oatk_multi_scg_consensus(m, ov, db, mine, 0, 1, fo) == 0, H.oatk_multi_last_error(m)
        libc.fclose(fo)
        L.refx_consensus(db, ref, 0, 1)
        G = E.flatten_graph(ref)
        same_graph(E.flatten_graph(mine), G)
        assert open(path).read().split("\n")[:-1] == gfa_lines(G)
        # min_cov above every coverage: no syncmer has a prepared consensus -- OATK_E_SPLIT, nothing written
        before = E.flatten_graph(mine)
        r = object.__new__(R.ScmDb)
        r._h = scm
        assert H.oatk_multi_consensus(m, int(r.flatten()["cov"].max()) + 1) == 0, H.oatk_multi_last_error(m)
        fo = libc.fopen(path, b"w")
        assert H.oatk_multi_scg_consensus(m, ov, db, mine, 0, 1, fo) == _lib.E_SPLIT
        libc.fclose(fo)
        after = E.flatten_graph(mine)
        for f in GRAPH_FIELDS:
            assert before[f].tobytes() == after[f].tobytes(), f
        assert open(path).read() == ""
        H.oatk_overlap_destroy(ov)
        for g in graphs:
            L.refx_scg_destroy(g)
    finally:
        L.refx_scmdb_destroy(scm), L.refx_srdb_destroy(db)
        H.oatk_multi_destroy(m)
