"""GPU: the strings of scg_consensus made on the device (oatk_hip_consensus_strings, csrc/cons_str.hpp) and the whole function on top of them
(liboatk_host.so: oatk_scg_consensus) against the compiled reference on the very same structs -- single pieces against scg_syncmer_consensus, whole unitigs
against scg_unitig_consensus, and the graph scg_consensus leaves (vertex lengths, coverages, sequences, arc overlaps, the GFA lines) array by array."""
import ctypes as C

import numpy as np
import pytest

import adversarial as A
import cons_util as CU
import ref_lib as R
import test_gpu_ec as T
from oatk_amd import _lib, pack_reads
from racov_util import Scg
from test_gpu_dropin import device_dbs, host_lib

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")
NONE64 = 0xFFFFFFFFFFFFFFFF


def libs():
    L, H = R.lib(), host_lib()
    vp = C.c_void_p
    H.oatk_read_error_correction.argtypes = [vp, vp, vp, vp, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, vp]
    H.oatk_overlap_fetch.restype = vp
    H.oatk_overlap_fetch.argtypes = [vp, C.POINTER(C.c_int)]
    H.oatk_overlap_destroy.argtypes = [vp]
    H.oatk_ovl_table_new.restype = vp
    H.oatk_ovl_table_destroy.argtypes = [vp]
    H.oatk_calc_syncmer_overlap.argtypes = [vp, C.c_uint64, C.c_uint64, vp]
    H.oatk_scg_consensus.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp]
    L.refx_syncmer_consensus.restype = C.c_int64
    L.refx_syncmer_consensus.argtypes = [vp, vp, C.c_uint64, C.c_int, C.c_int64, C.c_int, C.c_char_p, C.c_int64]
    L.refx_utg_lists.restype = C.c_uint64
    L.refx_utg_lists.argtypes = [vp] * 4
    L.refx_unitig_consensus.restype = C.c_int64
    L.refx_unitig_consensus.argtypes = [vp, vp, vp, C.c_uint64, C.c_int, C.c_char_p, C.c_int64]
    L.refx_process_unitigs.argtypes = [vp]
    return L, H


def scm_table(scm):
    r = object.__new__(R.ScmDb)
    r._h = scm
    return r.flatten()


def correct(hip, H, db, scm, c):
    st = np.zeros(12, np.uint64)
    assert H.oatk_read_error_correction(hip.h, db, scm, None, 0.02, c, 10 * c, c, 0.35, st.ctypes.data) == 0
    return st


def raw_strings(hip, seq_off, piece_v, piece_beg, hoco=0, want=None):
    """the return code of the entry point itself for a plan as given (nothing checked on this side)"""
    seq_off, piece_v, piece_beg = np.asarray(seq_off, np.uint64), np.asarray(piece_v, np.uint64), np.asarray(piece_beg, np.int32)
    plan = _lib.ConsPlan(max(len(seq_off) - 1, 0), len(piece_v), seq_off.ctypes.data, piece_v.ctypes.data, piece_beg.ctypes.data,
                         None if want is None else want.ctypes.data)
    tot, ref = C.c_uint64(), C.c_uint64()
    return hip.L.oatk_hip_consensus_strings(hip.h, C.byref(plan), hoco, C.byref(tot), C.byref(ref))


def text_of(b, off, i):
    return b[int(off[i]):int(off[i + 1])].tobytes()


PIECE_CASES = [(101, 11, 4, False, "long"), (101, 11, 4, True, "long"), (301, 21, 4, False, "long"), (301, 21, 4, True, "long"), (T.CASES[8][0], T.CASES[8][1], 4, True, "late")]


@needs_ref
@pytest.mark.parametrize("K,S,cov,with_ec,kind", PIECE_CASES)
def test_pieces_equal_the_reference(hip, K, S, cov, with_ec, kind):
    """one plan, one piece per sequence: every selected syncmer x rev x beg in {0, 9, K - 1, -4}, hoco and base space, against scg_syncmer_consensus"""
    L, H = libs()
    reads = CU.long_run_reads(K + 3, K) if kind == "long" else CU.late_run_reads(K + 7, K)
    db, scm = device_dbs(hip, reads, K, S)
    if with_ec:
        st = correct(hip, H, db, scm, cov)
        assert int(st[2] + st[7]) > 0
    hip.consensus(cov)
    sc = scm_table(scm)
    ids = np.nonzero((sc["cov"] >= cov) & (sc["del"] == 0))[0]
    assert len(ids) > (20 if kind == "long" else 5) and np.array_equal(ids, hip.fetch("CONS_SEL"))
    assert int(hip.fetch("CONS_RL").max()) > 255                            # run lengths past the 255 escape are in the table
    begs = (0, 9, K - 1, -4)
    v = np.repeat(np.repeat(ids.astype(np.uint64), 2) * 2 + np.tile(np.arange(2, dtype=np.uint64), len(ids)), len(begs))
    beg = np.tile(np.array(begs, np.int32), 2 * len(ids))
    seq_off = np.arange(len(v) + 1, dtype=np.uint64)
    buf = C.create_string_buffer(1 << 20)
    for hoco in (1, 0):
        b, off, length, status = hip.consensus_strings(seq_off, v, beg, hoco)
        assert hip.cons_strings == (len(b), 0) and not status.any() and int(off[-1]) == len(b)
        for i in range(len(v)):
            nr = L.refx_syncmer_consensus(db, scm, int(v[i]) >> 1, int(v[i]) & 1, int(beg[i]), hoco, buf, len(buf))
            assert int(length[i]) == nr and text_of(b, off, i) == buf.raw[:nr], (int(v[i]), int(beg[i]), hoco)
        if not hoco:
            assert int(length.max()) > K + 255
    # a syncmer below min_cov inside a sequence: that sequence is refused and takes no bytes, its neighbours are served
    hi = int(np.median(sc["cov"][ids])) + 1                                 # (a threshold that leaves some of the syncmers above out)
    hip.consensus(hi)
    low = ids[sc["cov"][ids] < hi]
    assert len(low) and hip.fetch("CONS_SLOT")[low[0]] == 0xFFFFFFFF and int(sc["cov"][ids].max()) >= hi
    good = int(ids[np.argmax(sc["cov"][ids])]) << 1
    b, off, length, status = hip.consensus_strings([0, 1, 3, 4], [good, good | 1, int(low[0]) << 1, good], [0, 0, 0, -4], 0)
    assert status.tolist() == [0, 1, 0] and hip.cons_strings[1] == 1 and int(length[1]) == NONE64 and off[1] == off[2]
    for i, (x, bg) in ((0, (good, 0)), (2, (good, -4))):
        nr = L.refx_syncmer_consensus(db, scm, x >> 1, x & 1, bg, 0, buf, len(buf))
        assert int(length[i]) == nr and text_of(b, off, i) == buf.raw[:nr]
    assert len(b) == int(length[0]) + int(length[2])
    L.refx_scmdb_destroy(scm)
    L.refx_srdb_destroy(db)


def unitig_lists(L, g):
    import ec_util as E
    nv = E.flatten_graph(g)["n_vtx"]
    n = np.zeros(nv, np.uint64)
    de = np.zeros(nv, np.uint8)
    tot = L.refx_utg_lists(g, n.ctypes.data, de.ctypes.data, None)
    a = np.zeros(max(tot, 1), np.uint64)
    L.refx_utg_lists(g, None, None, a.ctypes.data)
    starts = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    return [np.ascontiguousarray(a[starts[u]:starts[u + 1]]) for u in range(nv) if not de[u]]


def pieces_of(H, ov, v, K):
    """scg_unitig_consensus (syncasm.c:1004-1046) up to its calls of scg_syncmer_consensus: positions from one table kept across the pairs, then the skip loop"""
    n = len(v)
    if n == 0:
        return []
    tab = H.oatk_ovl_table_new()
    pos = [0]
    for i in range(1, n):
        pos.append(pos[-1] + H.oatk_calc_syncmer_overlap(ov, int(v[i - 1]), int(v[i]), tab))
    H.oatk_ovl_table_destroy(tab)
    out, end, i = [], 0, 0
    while i < n:
        while i + 1 < n and pos[i + 1] <= end:
            i += 1
        out.append((int(v[i]), end - pos[i]))
        end = pos[i] + K
        i += 1
    return out


UNITIG_CASES = [
    (101, 11, 4, lambda: T.diploid_reads(101, 6000, 150, 500, 1200, 0.006)),
    (301, 21, 5, lambda: T.sample_reads(T.genome_with_repeats(7, 25000, unit=1500, copies=4), 320, 4000, 0.003, 8)),
    (1001, 31, 6, lambda: A.hifi_like(200, 40000, 9000, seed=1009, err=0.0005)),
    (101, 11, 5, lambda: T.sample_reads(T.genome_with_repeats(9, 9000, unit=600, copies=3), 300, 1500, 0.004, 10)),
    T.CASES[8], T.CASES[9],                                 # k above 1024
]


@needs_ref
@pytest.mark.parametrize("K,S,c,mk", UNITIG_CASES)
def test_unitigs_equal_the_reference(hip, K, S, c, mk):
    """every live unitig of the reference's graph and its reverse complement in one plan; the device text equals scg_unitig_consensus, hoco and base space"""
    L, H = libs()
    db, scm = device_dbs(hip, mk(), K, S)
    correct(hip, H, db, scm, c)
    hip.consensus(c)
    rc = C.c_int(0)
    ov = H.oatk_overlap_fetch(hip.h, C.byref(rc))
    assert rc.value == 0 and ov
    g = L.refx_make_graph(db, scm, c, 0.35)
    L.refx_process_unitigs(g)
    lists = []
    for v in unitig_lists(L, g):
        lists += [v, np.ascontiguousarray(v[::-1] ^ np.uint64(1))]
    plan = [pieces_of(H, ov, v, K) for v in lists]
    seq_off = np.concatenate([[0], np.cumsum([len(p) for p in plan])]).astype(np.uint64)
    flat = [x for p in plan for x in p]
    pv, pb = np.array([x[0] for x in flat], np.uint64), np.array([x[1] for x in flat], np.int32)
    assert len(lists) >= 2 and max(len(v) for v in lists) >= 3
    assert any(len(p) < len(v) for p, v in zip(plan, lists))               # the skip loop left syncmers out
    assert ((pb > 0) & (pb < K)).any() and (pv & np.uint64(1)).any()
    buf = C.create_string_buffer(1 << 22)
    for hoco in (1, 0):
        b, off, length, status = hip.consensus_strings(seq_off, pv, pb, hoco)
        assert not status.any() and hip.cons_strings == (len(b), 0)
        for i, v in enumerate(lists):
            lr = L.refx_unitig_consensus(db, g, v.ctypes.data, len(v), hoco, buf, len(buf))
            assert 0 <= lr <= len(buf) and int(length[i]) == lr and text_of(b, off, i) == buf.raw[:lr], (i, hoco, len(v))
    H.oatk_overlap_destroy(ov)
    L.refx_scg_destroy(g)
    L.refx_scmdb_destroy(scm)
    L.refx_srdb_destroy(db)


GRAPH_FIELDS = ("vtx_len", "vtx_del", "vtx_cov", "vtx_seq_off", "seq", "arc_v", "arc_w", "arc_ls", "arc_cov", "arc_del", "arc_comp", "idx_p", "idx_n")


def same_graph(a, b):
    for f in GRAPH_FIELDS:
        assert a[f].dtype == b[f].dtype and np.array_equal(a[f], b[f]), f


def gfa_lines(G):
    """the H, S and L lines of scg_consensus (syncasm.c:738, :766, :814-815) from a flattened graph whose vertex coverages are set"""
    out = ["H\tVN:Z:1.0"]
    seq = G["seq"].tobytes().decode()
    for i in range(G["n_vtx"]):
        if G["vtx_del"][i]:
            continue
        l, cov, o = int(G["vtx_len"][i]), int(G["vtx_cov"][i]), int(G["vtx_seq_off"][i])
        out.append("S\tu%d\t%s\tLN:i:%d\tKC:i:%d\tSC:f:%.3f" % (i, seq[o:o + l], l, l * cov, cov))
    for i in range(G["n_arc"]):
        if G["arc_del"][i] or G["arc_comp"][i]:
            continue
        v, w, l, cov = int(G["arc_v"][i]), int(G["arc_w"][i]), int(G["arc_ls"][i]), int(G["arc_cov"][i])
        out.append("L\tu%d\t%s\tu%d\t%s\t%dM\tEC:i:%d" % (v >> 1, "+-"[v & 1], w >> 1, "+-"[w & 1], l, cov))
        out.append("L\tu%d\t%s\tu%d\t%s\t%dM\tEC:i:%d" % (w >> 1, "-+"[w & 1], v >> 1, "-+"[v & 1], l, cov))
    return out


@needs_ref
@pytest.mark.parametrize("K,S,c,mk", UNITIG_CASES[:2])
def test_the_whole_function_equals_scg_consensus(hip, tmp_path, K, S, c, mk):
    """two identical graphs, oatk_scg_consensus on one and the reference's scg_consensus on the other: every flattened array equal, hoco and base space, again
    with an arc whose overlap is counted in syncmers (ln > 0), the GFA lines, and a refusal that leaves the graph byte for byte as it was"""
    import ec_util as E
    L, H = libs()
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    db, scm = device_dbs(hip, mk(), K, S)
    correct(hip, H, db, scm, c)
    hip.consensus(c)
    rc = C.c_int(0)
    ov = H.oatk_overlap_fetch(hip.h, C.byref(rc))
    assert rc.value == 0 and ov
    graphs = []
    for _ in range(2):
        g = L.refx_make_graph(db, scm, c, 0.35)
        L.refx_process_unitigs(g)
        graphs.append(g)
    mine, ref = graphs
    same_graph(E.flatten_graph(mine), E.flatten_graph(ref))

    def both(hoco, fo=None):
        assert H.oatk_scg_consensus(hip.h, ov, db, mine, hoco, 1, fo) == 0, hip.L.oatk_hip_last_error(hip.h)
        L.refx_consensus(db, ref, hoco, 1)
        a, b = E.flatten_graph(mine), E.flatten_graph(ref)
        same_graph(a, b)
        return b

    for hoco in (1, 0):
        G = both(hoco)
        live = G["vtx_del"] == 0
        assert live.sum() >= 2 and (G["vtx_len"][live] >= K).all() and len(G["seq"]) == int(G["vtx_len"][live].sum())
        arcs = (G["arc_del"][:G["n_arc"]] == 0)
        assert arcs.sum() >= 2 and (G["arc_ls"][:G["n_arc"]][arcs] > 0).any()
    # an arc whose overlap is ln syncmers of its source unitig (what the unzip rounds make): the same value on both graphs
    am, ar = (C.cast(g, C.POINTER(Scg)).contents.utg_asmg.contents for g in (mine, ref))
    picked = [i for i in range(int(am.n_arc)) if not am.arc[i].del_ and not am.arc[i].comp and am.vtx[am.arc[i].v >> 1].n >= 2]
    assert picked
    for i in picked[:3]:
        am.arc[i].ln = ar.arc[i].ln = 2
    for hoco in (1, 0):
        G = both(hoco)
        assert all(G["arc_ls"][i] > 0 for i in picked[:3])                  # compared above, and not the empty overlap
    assert (G["vtx_cov"][G["vtx_del"] == 0] > 0).all()
    # the GFA lines, on a graph whose coverages are set
    path = str(tmp_path / "out.gfa").encode()
    fo = libc.fopen(path, b"w")
    assert fo
    G = both(0, fo)
    libc.fclose(fo)
    assert open(path).read().split("\n")[:-1] == gfa_lines(G)
    # a syncmer of the graph without prepared consensus: OATK_E_SPLIT, nothing written
    before = E.flatten_graph(mine)
    hip.consensus(int(scm_table(scm)["cov"].max()) + 1)
    fo = libc.fopen(path, b"w")
    assert H.oatk_scg_consensus(hip.h, ov, db, mine, 0, 1, fo) == _lib.E_SPLIT
    libc.fclose(fo)
    after = E.flatten_graph(mine)
    for f in GRAPH_FIELDS:
        assert before[f].tobytes() == after[f].tobytes(), f
    assert open(path).read() == ""
    for i in picked[:3]:
        am.arc[i].ln = ar.arc[i].ln = 0
    H.oatk_overlap_destroy(ov)
    for g in graphs:
        L.refx_scg_destroy(g)
    L.refx_scmdb_destroy(scm)
    L.refx_srdb_destroy(db)


def small_batch(hip, K=101, S=11, cov=4):
    hip.scan_host(*pack_reads(CU.long_run_reads(K + 3, K)), K, S)
    hip.count()
    c = hip.fetch("SCM_COV")
    return np.nonzero(c >= cov)[0].astype(np.uint64)


def test_length_only_sequences_and_empty_plans(hip):
    K = 101
    ids = small_batch(hip)
    hip.consensus(4)
    assert len(ids) > 20
    pv = np.concatenate([ids[:12] << np.uint64(1), ids[:12] << np.uint64(1) | np.uint64(1)])
    pb = np.array([0, 40, -4, K - 1] * 6, np.int32)
    seq_off = np.array([0, 5, 5, 11, 24], np.uint64)                        # sequence 1 is empty
    b1, off1, len1, st1 = hip.consensus_strings(seq_off, pv, pb, 0)
    assert not st1.any() and len1[1] == 0 and off1[1] == off1[2] and np.array_equal(np.diff(off1), len1)
    want = np.array([1, 1, 0, 1], np.uint8)
    b2, off2, len2, st2 = hip.consensus_strings(seq_off, pv, pb, 0, want_bytes=want)
    assert np.array_equal(len2, len1) and not st2.any()                     # the length is reported either way
    assert off2[3] == off2[2] and len(b2) == len(b1) - int(len1[2]) and hip.cons_strings == (len(b2), 0)
    for i in (0, 1, 3):
        assert text_of(b2, off2, i) == text_of(b1, off1, i)
    # pieces one by one add up to their sequence
    b3, off3, len3, _ = hip.consensus_strings(np.arange(25, dtype=np.uint64), pv, pb, 0)
    assert b3.tobytes() == b1.tobytes() and int(len3[:5].sum()) == int(len1[0])
    # nothing asked for
    b, off, length, status = hip.consensus_strings(np.zeros(1, np.uint64), [], [], 0)
    assert len(b) == 0 and off.tolist() == [0] and len(length) == 0 and len(status) == 0 and hip.cons_strings == (0, 0)
    b, off, length, status = hip.consensus_strings(np.zeros(3, np.uint64), [], [], 1)
    assert len(b) == 0 and off.tolist() == [0, 0, 0] and length.tolist() == [0, 0] and status.tolist() == [0, 0]


def test_plan_errors_and_state(hip):
    K = 101
    ids = small_batch(hip)
    n_scm = hip.info()["n_scm"]
    good = int(ids[0]) << 1
    assert raw_strings(hip, [0, 1], [good], [0]) == _lib.E_STATE             # before oatk_hip_consensus on this batch
    hip.consensus(4)
    assert raw_strings(hip, [0, 1], [good], [0]) == _lib.OK
    assert raw_strings(hip, [0, 1], [n_scm << 1], [0]) == _lib.E_ARG         # an id that is no syncmer
    assert raw_strings(hip, [0, 1], [good], [K]) == _lib.E_ARG               # beg == k
    assert raw_strings(hip, [0, 2, 1, 3], [good] * 3, [0] * 3) == _lib.E_ARG  # descending offsets
    assert raw_strings(hip, [0, 1, 2], [good] * 3, [0] * 3) == _lib.E_ARG    # offsets that do not end at n_piece
    assert raw_strings(hip, [0, 1], [good], [K - 1]) == _lib.OK
    b, off, length, status = hip.consensus_strings([0, 1], [good], [K - 1], 1)
    assert len(b) == 1 and length.tolist() == [1]
