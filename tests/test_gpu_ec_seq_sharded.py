"""GPU: the corrected reads' SEQUENCES with the reads sharded by record over several handles (oatk_hip_ec_keep_seq read by oatk_hip_ec_sharded,
oatk_hip_ec_corrected_reads on a handle that works in global ids, oatk_multi_read_error_correction_fo, ShardedEc.run(keep_seq=True)).

A rank corrects its own reads and a replaced body is spelled from the solver's optimum consensus, whether the path's k-mers were the shard's own or were
imported behind its hoco strings: the strings are rank-local, and the ranks' outputs in rank order are the file the COMPILED REFERENCE's
read_error_correction writes to its FILE *fo in read order (one thread: tests/ec_seq_util.py).  Checked against that file and against one handle holding all
reads, read for read and -- rebased by the offset of the rank's first read -- byte for byte.

Ranks are threads of this process over the in-process communicator group on the one GPU of the test box, as in tests/test_gpu_multi_c.py."""
import ctypes as C
import os
import socket
import threading

import numpy as np
import pytest

import adversarial as A
import ec_seq_util as U
import ref_lib as R
import test_gpu_multi_c as MC
from oatk_amd import HipSyncasm, _lib, pack_reads
from test_gpu_ec_seq import ARC_F, EC_NAMES, MAX_EDIST, OUT_COLS, flat_chains, named_dbs, reference_setup
from test_gpu_sharded_ec import vertex_graph

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")]

SHAPES = [2, 3, 0]                      # test_gpu_multi_c.CASES: a rank of six reads that lives on imported k-mers; an empty middle rank; two even halves
SEQ_BUFS = ("EC_CSEQ_LEN", "EC_CSEQ_OFF", "EC_CSEQ", "EC_BLOCK_QEND")
NO_SRC = np.uint64(0xFFFFFFFFFFFFFFFF)  # EC_VTX_SRC of a syncmer without a k-mer on the handle
JOIN_S = 300


def fetch_results(h):
    got = {k: h.fetch(k) for k in EC_NAMES}
    got["EC_BLOCK_OUT"] = h.fetch("EC_BLOCK_OUT").reshape(-1, 12)[:, OUT_COLS].copy()
    return got


def run_threads(world, work):
    """work(rank) on a thread per rank; the results in rank order"""
    out, errs = [None] * world, []

    def entry(rank):
        try:
            out[rank] = work(rank)
        except Exception as ex:                          # noqa: BLE001
            errs.append((rank, ex))

    th = [threading.Thread(target=entry, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=JOIN_S)
    assert not any(t.is_alive() for t in th), "a rank hangs in a collective"
    assert not errs, errs
    return out


def sharded_run(reads, bounds, K, S, c, a=ARC_F, with_off=True):
    """every rank: scan + count of its slice, [a sharded correction with the switch off,] a fresh scan + count and one with the switch on, the strings"""
    world = len(bounds) - 1
    L = _lib.load()
    grp = L.oatk_comm_group_create(world)
    assert grp

    def work(rank):
        h = HipSyncasm(0)
        comm = L.oatk_comm_group_rank(grp, rank)
        lo, hi = bounds[rank], bounds[rank + 1]
        seq, off, lens = pack_reads(reads[lo:hi])
        res = {}
        for keep in ((False, True) if with_off else (True,)):
            h.scan_host(seq, off, lens, K, S, sid0=lo)
            h.count()
            st, n_imp = h.ec_sharded(comm, MAX_EDIST, c, a, keep_seq=keep)
            res["on" if keep else "off"] = dict(fetch_results(h), stats=st, local_stats=h.ec_stats())
            if not keep:
                n = C.c_uint64(0)
                assert L.oatk_hip_ec_corrected_reads(h.h, C.byref(n)) == _lib.E_STATE      # the switch was off
        res["n_imported"], res["seq_bytes"] = n_imp, int(h.info()["seq_bytes"])
        n = C.c_uint64(12345)
        res["rc"] = L.oatk_hip_ec_corrected_reads(h.h, C.byref(n))                          # (the raw call: an empty rank answers OATK_OK with no reads)
        res["n_bases"] = int(n.value)
        res["seqs"] = h.corrected_reads()
        res.update({k: h.fetch(k) for k in SEQ_BUFS})
        L.oatk_comm_destroy(comm)
        h.close()
        return res

    try:
        return run_threads(world, work)
    finally:
        L.oatk_comm_group_destroy(grp)


_cache = {}


def shape(hip, idx, tmp_path):
    """per shape, once: the reads, the reference's lines, one handle's strings and buffers"""
    if idx not in _cache:
        K, S, c, mk, frac = MC.CASES[idx][:5]
        reads = mk()
        bounds = [int(round(f * len(reads))) for f in frac]
        G_host, hoco, want, close = reference_setup(hip, reads, K, S, c, tmp_path)       # (the batch stays resident in hip)
        close()
        hip.ec_graph()
        st = hip.ec(MAX_EDIST, c, ARC_F, keep_seq=True)
        one = {"seqs": hip.corrected_reads(), "stats": st}
        one.update({k: hip.fetch(k) for k in SEQ_BUFS})
        one["work"] = hip.fetch("EC_BLOCK_WORK").reshape(-1, 12)
        hip.ec_keep_seq(False)
        _cache[idx] = (K, S, c, reads, bounds, want, one)
    return _cache[idx]


def assert_ranks_equal_one_handle(out, bounds, want, one, what):
    seqs = [s for o in out for s in o["seqs"]]
    assert len(seqs) == len(want)
    bad = [i for i in range(len(want)) if seqs[i] != want[i]]
    assert not bad, "%s: %d of %d corrected reads differ from the reference's, first read %d" % (what, len(bad), len(want), bad[0])
    assert seqs == one["seqs"]
    assert np.array_equal(np.concatenate([o["EC_CSEQ_LEN"] for o in out]), one["EC_CSEQ_LEN"])
    assert np.array_equal(np.concatenate([o["EC_BLOCK_QEND"] for o in out]), one["EC_BLOCK_QEND"])
    assert np.all(one["EC_CSEQ_OFF"] % 16 == 0)
    for rank, o in enumerate(out):
        lo, hi = bounds[rank], bounds[rank + 1]
        off = o["EC_CSEQ_OFF"]
        assert o["rc"] == _lib.OK and len(o["EC_CSEQ_LEN"]) == hi - lo and len(off) == hi - lo + 1 and int(off[0]) == 0 and np.all(off % 16 == 0)
        assert o["n_bases"] == int(o["EC_CSEQ_LEN"].sum(dtype=np.uint64))
        b0, b1 = int(one["EC_CSEQ_OFF"][lo]), int(one["EC_CSEQ_OFF"][hi])
        assert np.array_equal(off, one["EC_CSEQ_OFF"][lo:hi + 1] - np.uint64(b0)), "%s: rank %d: offsets rebased by the first read's" % (what, rank)
        assert len(o["EC_CSEQ"]) == b1 - b0 and np.array_equal(o["EC_CSEQ"], one["EC_CSEQ"][b0:b1]), "%s: rank %d: packed bytes" % (what, rank)
        if hi > lo:
            assert int((o["EC_BLOCK_QEND"] > 0).sum()) > 0, "%s: rank %d replaces no block" % (what, rank)
        else:
            assert o["seqs"] == [] and o["n_bases"] == 0 and len(o["EC_CSEQ"]) == 0 and len(o["EC_BLOCK_QEND"]) == 0


@pytest.mark.parametrize("idx", SHAPES)
def test_ranks_in_rank_order_are_the_reference_file(hip, idx, tmp_path):
    K, S, c, reads, bounds, want, one = shape(hip, idx, tmp_path)
    assert one["seqs"] == want, "one handle's corrected reads equal the reference's"
    out = sharded_run(reads, bounds, K, S, c)
    assert_ranks_equal_one_handle(out, bounds, want, one, "case %d" % idx)
    # the switch changes nothing else, on any rank
    for rank, o in enumerate(out):
        for k in o["off"]:
            assert o["on"][k].dtype == o["off"][k].dtype and np.array_equal(o["on"][k], o["off"][k]), "rank %d: %s differs between a correction with and without the switch" % (rank, k)
        assert o["on"]["stats"][:11].tolist() == one["stats"][:11].tolist()
    # a corrected read: its chain holds an entry the correction put there (EC_KMER & 1)
    corrected_reads = []
    for o in out:
        at = np.concatenate([[0], np.cumsum(o["on"]["EC_N_SCM"].astype(np.int64))])
        flag = np.concatenate([[0], np.cumsum((o["on"]["EC_KMER"] & np.uint64(1)).astype(np.int64))])
        corrected_reads.append(int((flag[at[1:]] > flag[at[:-1]]).sum()))
    print("case %d: corrected reads per rank %s" % (idx, corrected_reads))
    if idx == 2:
        # not vacuous (figures of the compiled reference on these inputs): 1143 blocks, 1087 corrected; rank 0 holds six reads, all corrected, and most of what
        # replaces their blocks was never seen on the rank
        st = one["stats"]
        assert int(st[0] + st[5] + st[10]) == 1143 and int(st[2] + st[7]) == 1087
        o = out[0]
        assert bounds[1] == 6 and corrected_reads[0] == 6
        assert o["n_imported"] > 0
        km = o["on"]["EC_KMER"]
        fixed = km[(km & np.uint64(1)) != 0] >> np.uint64(1)
        assert len(fixed) == 50
        src = o["on"]["EC_VTX_SRC"][fixed.astype(np.int64)]
        imported = (src != NO_SRC) & (src >= np.uint64(o["seq_bytes"] // 4))
        print("rank 0: %d corrected chain entries, %d of them spelled from imported k-mers" % (len(fixed), int(imported.sum())))
        assert int(imported.sum()) > 0, "no replaced body of rank 0 was spelled from an imported k-mer"
        assert int(imported.sum()) == 30
    if idx == 0:
        assert corrected_reads == [52, 52]


def test_solver_routes_leave_the_same_bytes(hip, monkeypatch, tmp_path):
    """the two solvers the graph would choose between (OATK_DEBUG_EC_HEAVY=0: round 4's tiers, =1: the classes and the second stage)"""
    K, S, c, reads, bounds, want, one = shape(hip, SHAPES[0], tmp_path)
    runs = []
    for heavy in ("0", "1"):
        monkeypatch.setenv("OATK_DEBUG_EC_HEAVY", heavy)
        out = sharded_run(reads, bounds, K, S, c, with_off=False)
        assert_ranks_equal_one_handle(out, bounds, want, one, "OATK_DEBUG_EC_HEAVY=" + heavy)
        runs.append(out)
    for a, b in zip(*runs):
        for k in SEQ_BUFS:
            assert np.array_equal(a[k], b[k]), k


def test_call_order_on_a_sharded_handle(hip, tmp_path):
    K, S, c, reads, bounds, want, one = shape(hip, SHAPES[0], tmp_path)
    world = len(bounds) - 1
    L = _lib.load()
    grp = L.oatk_comm_group_create(world)

    def work(rank):
        h = HipSyncasm(0)
        comm = L.oatk_comm_group_rank(grp, rank)
        n = C.c_uint64(0)
        corrected = lambda: L.oatk_hip_ec_corrected_reads(h.h, C.byref(n))      # noqa: E731
        raw = lambda: {k: h.fetch(k) for k in SEQ_BUFS}                          # noqa: E731

        def same(first):
            now = raw()
            return all(np.array_equal(now[k], first[k]) for k in SEQ_BUFS)

        lo, hi = bounds[rank], bounds[rank + 1]
        seq, off, lens = pack_reads(reads[lo:hi])
        h.scan_host(seq, off, lens, K, S, sid0=lo)
        h.count()
        # the switch off: refused, nothing readable
        h.ec_sharded(comm, MAX_EDIST, c, ARC_F, keep_seq=False)
        assert corrected() == _lib.E_STATE
        for name in SEQ_BUFS:
            with pytest.raises(_lib.OatkHipError):
                h.fetch(name)
        # the switch on
        h.scan_host(seq, off, lens, K, S, sid0=lo)
        h.count()
        h.ec_sharded(comm, MAX_EDIST, c, ARC_F, keep_seq=True)
        with pytest.raises(_lib.OatkHipError):
            h.fetch("EC_CSEQ")                               # not before the call
        assert corrected() == _lib.OK
        first = raw()
        assert corrected() == _lib.OK and same(first)
        # the later sharded calls on the handle leave the slots, q_end and the blocks alone
        h.gather_table(comm, 0)
        assert corrected() == _lib.OK and same(first)
        nv, na = h.asm_graph_sharded(comm, c, ARC_F)
        h.consensus_sharded(comm, c)
        assert corrected() == _lib.OK and same(first)
        n_aln = h.read_alignment(vertex_graph(h.fetch_asm_graph(), nv, na))[0]
        assert n_aln > 0
        assert corrected() == _lib.OK and same(first)
        seqs = h.corrected_reads()
        # the handle leaves the id space the correction was made in
        h.ec_set_global(0, None, None, None)
        assert corrected() == _lib.E_STATE and b"sharded" in L.oatk_hip_last_error(h.h)
        with pytest.raises(_lib.OatkHipError):
            h.fetch("EC_CSEQ")
        # a new scan
        h.scan_host(seq, off, lens, K, S, sid0=lo)
        assert corrected() == _lib.E_STATE
        with pytest.raises(_lib.OatkHipError):
            h.fetch("EC_CSEQ")
        L.oatk_comm_destroy(comm)
        h.close()
        return seqs

    try:
        out = run_threads(world, work)
    finally:
        L.oatk_comm_group_destroy(grp)
    assert [s for o in out for s in o] == want


# ---- the N-handle adaptor ----
def chains_and_table(db, scm, K, S):
    out = flat_chains(db, K, S)
    t = object.__new__(R.ScmDb)
    t._h = scm
    f = t.flatten()
    out.update({"t_cov": f["cov"], "t_del": f["del"], "t_occ": f["occ"]})
    return out


def multi_setup(H, n, fa, K, S):
    m = H.oatk_multi_create((C.c_int * n)(*([0] * n)), n)
    assert m
    db = H.oatk_sr_db_new(K, S)
    H.oatk_host_debug_window(os.path.getsize(fa) // (3 * n) + 1000)          # about three windows per handle
    try:
        assert H.oatk_multi_sr_read_files(m, db, R._files_arg([fa]), 1) == 0, H.oatk_multi_last_error(m)
    finally:
        H.oatk_host_debug_window(0)
    rcc = C.c_int(0)
    scm = H.oatk_multi_collect_syncmer_from_reads(m, db, C.byref(rcc))
    assert rcc.value == 0 and scm, H.oatk_multi_last_error(m)
    return m, db, scm


_adaptor = {}


def adaptor_reference(hip, tmp_path):
    """once: the reads, their FASTA file, the reference's file and the one-handle adaptor's"""
    if not _adaptor:
        K, S, c = 301, 21, 6
        reads = A.hifi_like(260, 50000, 5000, seed=5)
        names = [b"read/%d/ccs_with_a_longer_name" % i if i % 7 else b"r%d" % i for i in range(len(reads))]
        L = R.lib()
        db, scm = named_dbs(hip, reads, K, S, names)
        g = L.refx_make_graph(db, scm, 0, 0.0)
        L.refx_consensus(db, g, 1, 1)
        want = U.reference_ec_fo(db, g, MAX_EDIST, c, ARC_F, tmp_path / "ref.fo")
        L.refx_scg_destroy(g), L.refx_scmdb_destroy(scm), L.refx_srdb_destroy(db)
        H = _lib.load_host()
        vp = C.c_void_p
        H.oatk_read_error_correction_fo.argtypes = [vp, vp, vp, vp, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, vp, vp]
        db, scm = named_dbs(hip, reads, K, S, names)
        st = np.zeros(12, np.uint64)
        fo = U.libc().fopen(str(tmp_path / "one.fo").encode(), b"w")
        rc = H.oatk_read_error_correction_fo(hip.h, db, scm, None, MAX_EDIST, c, 10 * c, c, ARC_F, fo, st.ctypes.data)
        U.libc().fclose(fo)
        assert rc == 0, hip.L.oatk_hip_last_error(hip.h)
        L.refx_scmdb_destroy(scm), L.refx_srdb_destroy(db)
        one = open(tmp_path / "one.fo", "rb").read()
        assert one == want and len(U.parse_fo(want)) == len(reads)
        _adaptor["v"] = (K, S, c, reads, names, want)
    return _adaptor["v"]


@pytest.mark.parametrize("n", [2, 3])
def test_adaptor_over_several_handles_writes_the_reference_file(hip, n, tmp_path):
    K, S, c, reads, names, want = adaptor_reference(hip, tmp_path)
    fa = str(tmp_path / "reads.fa")
    with open(fa, "wb") as f:
        for nm, r in zip(names, reads):
            f.write(b">" + nm + b"\n" + r + b"\n")
    L, H, Lh = R.lib(), _lib.load_host(), _lib.load()
    lc = U.libc()

    def seq_built(m):
        built = []
        for r in range(n):
            d, b = C.c_void_p(), C.c_uint64()
            built.append(Lh.oatk_hip_buffer(H.oatk_multi_ctx(m, r), _lib.BUF["EC_CSEQ"], C.byref(d), C.byref(b)) == _lib.OK)
        return built

    # without a file: what oatk_multi_read_error_correction leaves, and no sequence buffer anywhere
    m, db, scm = multi_setup(H, n, fa, K, S)
    st0 = np.zeros(12, np.uint64)
    assert H.oatk_multi_read_error_correction(m, db, scm, MAX_EDIST, c, 10 * c, c, ARC_F, st0.ctypes.data) == 0, H.oatk_multi_last_error(m)
    plain = chains_and_table(db, scm, K, S)
    assert seq_built(m) == [False] * n
    L.refx_scmdb_destroy(scm), L.refx_srdb_destroy(db)
    H.oatk_multi_destroy(m)
    # NULL file through the new entry point: the same
    m, db, scm = multi_setup(H, n, fa, K, S)
    st1 = np.zeros(12, np.uint64)
    assert H.oatk_multi_read_error_correction_fo(m, db, scm, MAX_EDIST, c, 10 * c, c, ARC_F, None, st1.ctypes.data) == 0, H.oatk_multi_last_error(m)
    assert seq_built(m) == [False] * n
    null_fo = chains_and_table(db, scm, K, S)
    L.refx_scmdb_destroy(scm), L.refx_srdb_destroy(db)
    H.oatk_multi_destroy(m)
    # a file that cannot be written: an error, and the databases as they were
    m, db, scm = multi_setup(H, n, fa, K, S)
    for r in range(n):
        cnt = C.c_uint64()
        H.oatk_multi_range(m, r, None, C.byref(cnt))
        assert cnt.value > 0
    before = chains_and_table(db, scm, K, S)
    ro = lc.fopen(fa.encode(), b"r")
    st2 = np.zeros(12, np.uint64)
    rc = H.oatk_multi_read_error_correction_fo(m, db, scm, MAX_EDIST, c, 10 * c, c, ARC_F, ro, st2.ctypes.data)
    lc.fclose(ro)
    assert rc != 0 and H.oatk_multi_last_error(m)
    after = chains_and_table(db, scm, K, S)
    for k in before:
        assert np.array_equal(before[k], after[k]), "a failed call changed %s" % k
    L.refx_scmdb_destroy(scm), L.refx_srdb_destroy(db)
    H.oatk_multi_destroy(m)
    # into a file
    m, db, scm = multi_setup(H, n, fa, K, S)
    st3 = np.zeros(12, np.uint64)
    fo = lc.fopen(str(tmp_path / "multi.fo").encode(), b"w")
    rc = H.oatk_multi_read_error_correction_fo(m, db, scm, MAX_EDIST, c, 10 * c, c, ARC_F, fo, st3.ctypes.data)
    lc.fclose(fo)
    assert rc == 0, H.oatk_multi_last_error(m)
    got = open(tmp_path / "multi.fo", "rb").read()
    assert got == want, "the N-handle adaptor's file differs from the reference's"
    with_fo = chains_and_table(db, scm, K, S)
    L.refx_scmdb_destroy(scm), L.refx_srdb_destroy(db)
    H.oatk_multi_destroy(m)
    for k in plain:
        assert np.array_equal(with_fo[k], plain[k]) and np.array_equal(null_fo[k], plain[k]), k
    assert len(before["k_mer"]) != len(plain["k_mer"]) or not np.array_equal(before["k_mer"], plain["k_mer"])      # (the correction does change the chains)
    assert st0[:11].tolist() == st1[:11].tolist() == st3[:11].tolist()


# ---- the torch path ----
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _torch_worker(rank, world, port, reads, bounds, K, S, c, outdir):
    import pickle
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oatk_amd.multi import ShardedEc
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    h = HipSyncasm(0)
    lo, hi = bounds[rank], bounds[rank + 1]
    seq, off, lens = pack_reads(reads[lo:hi])
    h.scan_host(seq, off, lens, K, S, sid0=lo)
    h.count()
    sh = ShardedEc(h, dist, dev)
    sh.run(MAX_EDIST, c, ARC_F, keep_seq=True)
    with open(os.path.join(outdir, "seq%d.pkl" % rank), "wb") as f:
        pickle.dump(h.corrected_reads(), f)
    h.close()
    dist.barrier()
    dist.destroy_process_group()


def test_torch_path_two_processes(hip, tmp_path):
    """ShardedEc.run(keep_seq=True) drives oatk_hip_ec_mark / oatk_hip_ec_correct itself: two processes on the one GPU over gloo"""
    import pickle
    import torch.multiprocessing as mp
    K, S, c, reads, bounds, want, one = shape(hip, SHAPES[0], tmp_path)
    world = len(bounds) - 1
    mp.spawn(_torch_worker, args=(world, _free_port(), reads, bounds, K, S, c, str(tmp_path)), nprocs=world, join=True)
    got = []
    for r in range(world):
        with open(tmp_path / ("seq%d.pkl" % r), "rb") as f:
            got += pickle.load(f)
    assert got == one["seqs"] and got == want
