"""GPU: the corrected reads' SEQUENCES from the device (oatk_hip_ec_keep_seq + oatk_hip_ec_corrected_reads, oatk_amd/csrc/ec_seq.hpp) against what the COMPILED
REFERENCE's read_error_correction writes to its FILE *fo (syncerr.c:544-558, :590-597, :614-624), read by read, on the same databases and the same EC graph.

The reference is called directly (liboatk_ref.so exports read_error_correction) with ONE thread: its threads write under a mutex in the order they finish, and
with one thread that is read order.  Every solver route must leave the same strings -- they come from the solver's own optimum consensus -- and the switch must
change nothing else: every EC_* buffer and the statistics are compared with a run of the same variant without it.

Not covered: EC_AMBISNQ (two live paths that spell one string).  None of these inputs, nor any of test_gpu_ec.CASES at seven threshold settings, produces such a
block in the reference; the device writes the optimum for it as it does for EC_SUCCESS (ec_wave.hpp: ec_keep_seq)."""
import ctypes as C

import numpy as np
import pytest

import adversarial as A
import ec_seq_util as U
import ec_util as E
import ref_lib as R
import test_gpu_ec as G
from oatk_amd import _lib, pack_reads
from test_gpu_dropin import device_dbs, host_lib
from test_gpu_ec_routes import nohp_base, tiled

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")]

MAX_EDIST, ARC_F = 0.02, 0.35
VARIANTS = ["host", "device", "device-tiers", "device-heavy", "device-heavy-spill", "device-fused", "device-fused-nw4"]
# every resident result of the correction but EC_BLOCK_OUT (below) and the sequences themselves
EC_NAMES = ["EC_N_SCM", "EC_SCM_OFF", "EC_KMER", "EC_MPOS", "EC_SMER", "EC_SCM_COV", "EC_SCM_DEL", "EC_SCM_OCC_OFF", "EC_SCM_OCC", "EC_ERR_DEL", "EC_SCM_FWD",
            "EC_VTX_SRC", "EC_BLOCK_WORK"]
# EcBlockOut, 12 words per block: all but path_off (2, 3: the pool hands out chunks by atomics) and ticks (10: a clock)
OUT_COLS = [0, 1, 4, 5, 6, 7, 8, 9, 11]


def set_variant(hip, monkeypatch, graph):
    """the solver's knobs exactly as tests/test_gpu_ec.py sets them for a variant of that name"""
    monkeypatch.setenv("OATK_DEBUG_EC_FUSED_MIN_NW", graph[len("device-fused-nw"):] if graph.startswith("device-fused-nw") else "0")
    t0, t1 = (48, 160) if graph.startswith("device-tiers") or graph == "device-heavy-mix" else ((48, 0) if graph.startswith("device-heavy") or graph.startswith("device-fused") else (0, 0))
    monkeypatch.setenv("OATK_DEBUG_EC_STEP_BUDGET", "1" if graph.startswith("device-fused") else ("8" if graph == "device-heavy-mix" else "0"))
    monkeypatch.setenv("OATK_DEBUG_EC_SERIAL_TIERS", "1" if graph == "device-tiers-serial" else "0")
    if graph in ("device", "host"):
        monkeypatch.delenv("OATK_DEBUG_EC_HEAVY", raising=False)
    else:
        monkeypatch.setenv("OATK_DEBUG_EC_HEAVY", "0" if graph.startswith("device-tiers") else "1")
    monkeypatch.setenv("OATK_DEBUG_EC_HEAVY_CAP2", "400" if graph == "device-heavy-mix" else "0")
    monkeypatch.setenv("OATK_DEBUG_EC_HEAVY_FL", "64" if graph in ("device-heavy-spill", "device-fused-spill") else "0")
    hip._check(hip.L.oatk_hip_debug_ec_tiers(hip.h, t0, t1), "oatk_hip_debug_ec_tiers")


def device_run(hip, G_host, c, keep_seq):
    """one correction (against the host's flattened graph, or one built on the device) and every resident result of it"""
    if G_host is None:
        hip.ec_graph()
    st = hip.ec(MAX_EDIST, c, ARC_F, graph=G_host, keep_seq=keep_seq)
    got = {k: hip.fetch(k) for k in EC_NAMES}
    got["EC_BLOCK_OUT"] = hip.fetch("EC_BLOCK_OUT").reshape(-1, 12)[:, OUT_COLS].copy()
    got["stats"] = st
    return got


def assert_same_results(on, off, what):
    for k in off:
        assert on[k].dtype == off[k].dtype and np.array_equal(on[k], off[k]), "%s: %s differs between a correction with and without the switch" % (what, k)


def reference_setup(hip, reads, K, S, c, tmp_path):
    """reference-layout structs from the device scan + count (the batch stays resident), the reference's EC graph, the hoco strings, and -- LAST, it rewrites the
    structs -- the reference's corrected reads"""
    db, scm = device_dbs(hip, reads, K, S)
    L = R.lib()
    g = L.refx_make_graph(db, scm, 0, 0.0)                  # run_syncasm.c:109
    L.refx_consensus(db, g, 1, 1)                           # run_syncasm.c:117
    G_host = E.flatten_graph(g)
    rdb = object.__new__(R.SrDb)
    rdb._h, rdb.K, rdb.S = db, K, S
    hoco = U.hoco_strings(rdb.flatten())
    want = [s for _, s in U.parse_fo(U.reference_ec_fo(db, g, MAX_EDIST, c, ARC_F, tmp_path / "ref.fo"))]
    assert len(want) == len(reads)

    def close():
        L.refx_scg_destroy(g)
        L.refx_scmdb_destroy(scm)
        L.refx_srdb_destroy(db)
    return G_host, hoco, want, close


def check_sequences(hip, got, want, hoco, what):
    """the device's strings against the reference's lines; the side array against the outcomes; reads without a replaced block against their own strings"""
    seqs = hip.corrected_reads()
    assert len(seqs) == len(want)
    bad = [i for i in range(len(want)) if seqs[i] != want[i]]
    assert not bad, "%s: %d of %d corrected reads differ from the reference's, first read %d" % (what, len(bad), len(want), bad[0])
    work, out = got["EC_BLOCK_WORK"].reshape(-1, 12), hip.fetch("EC_BLOCK_OUT").reshape(-1, 12)
    qend = hip.fetch("EC_BLOCK_QEND")
    replaced = ((out[:, 0] == 1) | (out[:, 0] == 2)) & (out[:, 5] == 0)
    assert len(qend) == len(work) and np.array_equal(qend > 0, replaced), "%s: EC_BLOCK_QEND is set exactly where a block's bases are replaced" % what
    touched = np.zeros(len(want), bool)
    touched[work[replaced, 4]] = True
    for i in np.flatnonzero(~touched):
        assert seqs[i] == hoco[i], "%s: read %d has no replaced block and must equal its hoco string" % (what, i)
    return seqs, int((~touched).sum())


PARITY_CASES = [0, 1, 4, 5, 6, 7]


@pytest.mark.parametrize("case", PARITY_CASES)
def test_corrected_reads_match_reference(hip, case, monkeypatch, tmp_path):
    K, S, c, mk = G.CASES[case]
    reads = mk()
    G_host, hoco, want, close = reference_setup(hip, reads, K, S, c, tmp_path)
    try:
        # the inputs exercise the feature (on the reference's output alone): reads changed inside their first / last k bases -- the first k only a leading block
        # can change, the last k only a trailing one -- and reads that come out as they went in
        head = sum(w[:K] != h[:K] for w, h in zip(want, hoco))
        tail = sum(w[-K:] != h[-K:] for w, h in zip(want, hoco))
        same = sum(w == h for w, h in zip(want, hoco))
        print("case %d: %d reads, changed %d (head %d, tail %d), unchanged %d" % (case, len(want), len(want) - same, head, tail, same))
        assert head >= 40 and tail >= 40 and same >= 9
        first = None
        for graph in VARIANTS:
            set_variant(hip, monkeypatch, graph)
            Gh = G_host if graph == "host" else None
            off = device_run(hip, Gh, c, False)
            with pytest.raises(_lib.OatkHipError):
                hip.corrected_reads()                       # the switch was off
            on = device_run(hip, Gh, c, True)
            assert_same_results(on, off, graph)
            check_sequences(hip, on, want, hoco, graph)
            raw = {k: hip.fetch(k) for k in ("EC_CSEQ", "EC_CSEQ_LEN", "EC_CSEQ_OFF")}
            assert np.all(raw["EC_CSEQ_OFF"] % 16 == 0) and len(raw["EC_CSEQ"]) == int(raw["EC_CSEQ_OFF"][-1])
            if first is None:
                first = raw
            for k in raw:
                assert np.array_equal(raw[k], first[k]), "%s: %s differs from the %s variant's" % (graph, k, VARIANTS[0])
            if graph != "host" and graph != "device":
                assert int(on["stats"][11]) > 0             # blocks did fall through the tiny first tier
    finally:
        hip._check(hip.L.oatk_hip_debug_ec_tiers(hip.h, 0, 0), "oatk_hip_debug_ec_tiers")
        close()


# kernel variants (EcBlockOut.tier), as tests/test_gpu_ec_routes.py names them
T_LDS, T_SLAB, T_HYBRID = 0, 1, 2
T_CLASS = (16 + 4, 16 + 8, 8 + 6)


def test_long_corrected_blocks(hip, monkeypatch, tmp_path):
    """Blocks of 1400 .. 38 400 bases that the search corrects, on the shipping caps: their optimum consensus is hundreds to thousands of words and leaves the
    solver from every kind of kernel.  Three runs choose the routes: round 4's tiers (first LDS tier, hybrid tier, slabs), the classes (one wave with 4 / 8
    registers per lane, four waves with 6; what they cannot hold goes to the slabs), and the classes with a step budget of 1 (everything on to the second stage's
    fused classes)."""
    reads, truth = U.long_corrected_reads()
    G_host, hoco, want, close = reference_setup(hip, reads, U.LONG_K, U.LONG_S, U.LONG_C, tmp_path)
    try:
        assert want[:60] == hoco[:60] and want[60:] == truth, "the reference restores the 18 long reads to the genome and leaves the clean ones"
        for k in ("OATK_DEBUG_EC_FUSED_MIN_NW", "OATK_DEBUG_EC_SERIAL_TIERS", "OATK_DEBUG_EC_HEAVY_CAP2", "OATK_DEBUG_EC_HEAVY_FL"):
            monkeypatch.setenv(k, "0")
        hip._check(hip.L.oatk_hip_debug_ec_tiers(hip.h, 0, 0), "oatk_hip_debug_ec_tiers")
        tags = set()
        for heavy, budget in (("0", "0"), ("1", "0"), ("1", "1")):
            monkeypatch.setenv("OATK_DEBUG_EC_HEAVY", heavy)
            monkeypatch.setenv("OATK_DEBUG_EC_STEP_BUDGET", budget)
            what = "OATK_DEBUG_EC_HEAVY=%s OATK_DEBUG_EC_STEP_BUDGET=%s" % (heavy, budget)
            on = device_run(hip, None, U.LONG_C, True)
            seqs, _ = check_sequences(hip, on, want, hoco, what)
            assert seqs[60:] == truth
            work, out = on["EC_BLOCK_WORK"].reshape(-1, 12), hip.fetch("EC_BLOCK_OUT").reshape(-1, 12)
            long_ok = (work[:, 6].astype(np.int32) >= 1400) & (out[:, 0] == 1)
            assert int(long_ok.sum()) == len(U.LONG_LENGTHS), what
            run_tags = set(int(t) for t in out[long_ok, 11])
            print("%s: long corrected blocks finished by kernels %s" % (what, sorted(run_tags)))
            tags |= run_tags
        assert T_LDS in tags, "no long corrected block finished in a first LDS tier"
        assert tags & {T_SLAB, T_HYBRID}, "no long corrected block finished in a slab or hybrid tier"
        assert tags & set(T_CLASS), "no long corrected block finished in a class of the first stage"
        assert any(t >= 32 for t in tags), "no long corrected block finished in a fused class of the second stage"
    finally:
        close()


def edge_reads():
    """K 101, S 11, c 3.  Clean reads tile a homopolymer-free genome; then, in this order: a read with a substitution every 350 bases (more than 64 blocks, all
    closed: the clean anchors between them are longer than k + 10), a read shorter than k, a read from elsewhere (every syncmer seen once: no good syncmer, the
    whole string comes out), two reads with N (one inside a run of the same base: the run closes over it in hoco space), and a read whose errors sit in its ends."""
    rng = np.random.default_rng(424242)
    h = A.rand_nohp(rng, 30000)
    reads = tiled(h, 50, 3000, 0, 3)
    many = bytearray(h[1000:28000])
    for p in range(300, len(many) - 300, 350):
        many[p] = nohp_base(rng, {many[p], many[p - 1], many[p + 1]})
    short = h[5000:5060]
    lone = A.rand_nohp(rng, 2500)
    n1 = bytearray(h[7000:10000])
    n1[1500] = ord("N")
    n2 = bytearray(h[12000:15000])
    n2[700:703] = b"NNN"
    n2[2000] = n2[1999]
    ends = bytearray(h[16000:19000])
    for p in (20, 55, 2950, 2990):
        ends[p] = nohp_base(rng, {ends[p], ends[p - 1], ends[p + 1]})
    return reads + [bytes(many), short, lone, bytes(n1), bytes(n2), A.revcomp(bytes(ends))], 50


@pytest.mark.parametrize("alone", [False, True])
def test_edges(hip, alone, monkeypatch, tmp_path):
    K, S, c = 101, 11, 3
    reads, n_clean = edge_reads()
    if alone:
        reads = [reads[3]]                                  # one read alone: every syncmer is seen once
    G_host, hoco, want, close = reference_setup(hip, reads, K, S, c, tmp_path)
    try:
        set_variant(hip, monkeypatch, "device")
        on = device_run(hip, None, c, True)
        seqs, n_untouched = check_sequences(hip, on, want, hoco, "edges")
        work = on["EC_BLOCK_WORK"].reshape(-1, 12)
        n_scm = hip.fetch("N_SCM")
        if alone:
            assert len(work) == 0 and seqs == hoco
        else:
            many, short, lone = n_clean, n_clean + 1, n_clean + 2
            assert int((work[:, 4] == many).sum()) > 64, "the read with a substitution every 350 bases has more than 64 blocks"
            assert seqs[many] != hoco[many]
            assert n_scm[short] == 0 and len(hoco[short]) < K and seqs[short] == hoco[short]
            assert n_scm[lone] > 0 and not (work[:, 4] == lone).any() and seqs[lone] == hoco[lone], "a read without a good syncmer has no block and keeps its string"
            assert n_untouched >= 2
    finally:
        hip._check(hip.L.oatk_hip_debug_ec_tiers(hip.h, 0, 0), "oatk_hip_debug_ec_tiers")
        close()


def test_call_order(hip, monkeypatch):
    K, S, c, mk = G.CASES[6]
    reads = mk()
    set_variant(hip, monkeypatch, "device")
    n = C.c_uint64(0)
    corrected = lambda: hip.L.oatk_hip_ec_corrected_reads(hip.h, C.byref(n))
    hip.scan_host(*pack_reads(reads), K, S)
    hip.count()
    hip.ec_graph()
    # without the switch
    hip.ec(MAX_EDIST, c, ARC_F, keep_seq=False)
    assert corrected() == _lib.E_STATE
    for name in ("EC_CSEQ", "EC_CSEQ_LEN", "EC_CSEQ_OFF", "EC_BLOCK_QEND"):
        with pytest.raises(_lib.OatkHipError):
            hip.fetch(name)
    # with it: the sequences are there once oatk_hip_ec_corrected_reads has run, not before
    hip.ec(MAX_EDIST, c, ARC_F, keep_seq=True)
    assert len(hip.fetch("EC_BLOCK_QEND")) == len(hip.fetch("EC_BLOCK_WORK")) // 12
    with pytest.raises(_lib.OatkHipError):
        hip.fetch("EC_CSEQ")
    assert corrected() == _lib.OK and n.value > 0
    first = hip.fetch("EC_CSEQ")
    assert corrected() == _lib.OK                           # again, from the same resident correction
    assert np.array_equal(hip.fetch("EC_CSEQ"), first)
    # a later correction with the switch off leaves nothing stale to read
    hip.ec(MAX_EDIST, c, ARC_F, keep_seq=False)
    assert corrected() == _lib.E_STATE
    for name in ("EC_CSEQ", "EC_CSEQ_LEN", "EC_CSEQ_OFF", "EC_BLOCK_QEND"):
        with pytest.raises(_lib.OatkHipError):
            hip.fetch(name)
    # a scan since the correction
    hip.ec(MAX_EDIST, c, ARC_F, keep_seq=True)
    assert corrected() == _lib.OK
    hip.scan_host(*pack_reads(reads[:50]), K, S)
    assert corrected() == _lib.E_STATE
    with pytest.raises(_lib.OatkHipError):
        hip.fetch("EC_CSEQ")
    # a sharded context (global syncmer ids; the map is only stored here, any resident u32[n_scm] will do for it): refused as such
    hip.count()
    hip.ec_graph()
    hip.ec(MAX_EDIST, c, ARC_F, keep_seq=True)
    assert corrected() == _lib.OK
    ns = int(hip.info()["n_scm"])
    cov, s = hip.buffer("SCM_COV")[0], hip.buffer("SCM_S")[0]
    try:
        hip.ec_set_global(ns, cov, cov, s)
        assert corrected() == _lib.E_STATE and b"sharded" in hip.L.oatk_hip_last_error(hip.h)
    finally:
        hip.ec_set_global(0, None, None, None)
        hip.ec_keep_seq(False)


def named_dbs(hip, reads, K, S, names):
    """device_dbs with read names (malloc'ed: the structs adopt them and the reference's destructor frees them)"""
    H = host_lib()
    seq, off, lens = pack_reads(reads)
    arr = (C.c_void_p * len(reads))(*[U.libc().strdup(nm) for nm in names])
    db = H.oatk_sr_db_new(K, S)
    rc = H.oatk_sr_read_packed(hip.h, db, seq.ctypes.data, off.ctypes.data, lens.ctypes.data, len(reads), seq.size, arr)
    assert rc == 0, hip.L.oatk_hip_last_error(hip.h)
    rcc = C.c_int(0)
    scm = H.oatk_collect_syncmer_from_reads(hip.h, db, C.byref(rcc))
    assert rcc.value == 0 and scm
    return db, scm


def flat_chains(db, K, S):
    rdb = object.__new__(R.SrDb)
    rdb._h, rdb.K, rdb.S = db, K, S
    f = rdb.flatten()
    return {k: f[k] for k in ("n_scm", "k_mer", "m_pos", "s_mer")}


@pytest.mark.parametrize("host_graph", [False, True])
def test_adaptor_writes_the_reference_file(hip, host_graph, monkeypatch, tmp_path):
    """oatk_read_error_correction_fo (liboatk_host.so): the file the reference writes, names included, and the chains oatk_read_error_correction writes back"""
    K, S, c, mk = G.CASES[6]
    reads = mk()
    names = [b"read/%d some text" % i if i % 7 else b"r%d" % i for i in range(len(reads))]
    set_variant(hip, monkeypatch, "device")
    H = host_lib()
    vp = C.c_void_p
    args = [vp, vp, vp, vp, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double]
    H.oatk_read_error_correction.argtypes = args + [vp]
    H.oatk_read_error_correction_fo.argtypes = args + [vp, vp]
    L = R.lib()
    # the reference, on structs of its own
    db, scm = named_dbs(hip, reads, K, S, names)
    g = L.refx_make_graph(db, scm, 0, 0.0)
    L.refx_consensus(db, g, 1, 1)
    want = U.reference_ec_fo(db, g, MAX_EDIST, c, ARC_F, tmp_path / "ref.fo")
    want_chains = flat_chains(db, K, S)
    L.refx_scg_destroy(g), L.refx_scmdb_destroy(scm), L.refx_srdb_destroy(db)
    # the adaptor
    db, scm = named_dbs(hip, reads, K, S, names)
    g = None
    if host_graph:
        g = L.refx_make_graph(db, scm, 0, 0.0)
        L.refx_consensus(db, g, 1, 1)
    asmg = C.cast(g, C.POINTER(vp))[1] if g else None      # scg_t: { scm_db, utg_asmg, ... } (syncasm.h)
    st = np.zeros(12, np.uint64)
    fo = U.libc().fopen(str(tmp_path / "dev.fo").encode(), b"w")
    rc = H.oatk_read_error_correction_fo(hip.h, db, scm, asmg, MAX_EDIST, c, 10 * c, c, ARC_F, fo, st.ctypes.data)
    U.libc().fclose(fo)
    assert rc == 0, hip.L.oatk_hip_last_error(hip.h)
    got = open(tmp_path / "dev.fo", "rb").read()
    assert got == want, "the adaptor's file differs from the reference's"
    assert got.count(b">read/8 some text\n") == 1
    got_chains = flat_chains(db, K, S)
    if g:
        L.refx_scg_destroy(g)
    L.refx_scmdb_destroy(scm), L.refx_srdb_destroy(db)
    # the same without a file
    db, scm = named_dbs(hip, reads, K, S, names)
    st2 = np.zeros(12, np.uint64)
    rc = H.oatk_read_error_correction(hip.h, db, scm, None, MAX_EDIST, c, 10 * c, c, ARC_F, st2.ctypes.data)
    assert rc == 0, hip.L.oatk_hip_last_error(hip.h)
    plain = flat_chains(db, K, S)
    L.refx_scmdb_destroy(scm), L.refx_srdb_destroy(db)
    for k in plain:
        assert np.array_equal(got_chains[k], plain[k]) and np.array_equal(got_chains[k], want_chains[k]), k
    assert np.array_equal(st[:11], st2[:11])
    # the switch is the call's own: the handle is left without it
    with pytest.raises(_lib.OatkHipError):
        hip.corrected_reads()
