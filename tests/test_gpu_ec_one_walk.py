"""GPU: the error blocks listed in ONE walk over the chains (ec.hpp: ec_stage_blocks_wave_kernel stages a descriptor per block, ec_fill_work_kernel builds
the work items behind the scan) against the two walks it replaces (ec_count_blocks_wave_kernel, ec_list_blocks_wave_kernel, kept behind
OATK_DEBUG_EC_LIST_WALK=1) and, where oracle/_ref is built, against the compiled reference's read_error_correction.

The read sets are tests/test_gpu_ec_assemble.py's, whose test_cases_are_present holds them to the cases that matter here as well: reads with no block, clean
reads (the leading and the open block only), 64 and 65 syncmers (the last chain a wave walks, the first that lane 0 walks alone), more than 64 blocks, a
read count that is no multiple of the four reads of a workgroup, sid0 > 0, a batch assembled by oatk_hip_scan_append.

What is compared: the work list (EC_BLOCK_WORK: every byte of every EcWork, `pad` included), the blocks' outcomes (EC_BLOCK_OUT) and every array the
correction leaves (test_gpu_ec_assemble.OUT) -- copy_n, keep_all and the descriptors reach nothing else.  Of EcBlockOut's twelve words two are no function of
the input on either route and are left out, as tests/test_gpu_ec_seq.py leaves them out: path_off (the pool hands out chunks by atomics) and ticks (a clock)."""
import os

import numpy as np
import pytest

import ref_lib as R
import test_gpu_ec_assemble as EA
from oatk_amd import HipSyncasm, pack_reads
from test_gpu_ec_seq import OUT_COLS

pytestmark = pytest.mark.gpu

K, S, C_MIN, EDIST, ARC_F = EA.K, EA.S, EA.C_MIN, EA.EDIST, EA.ARC_F
SWITCH = "OATK_DEBUG_EC_LIST_WALK"


def correct(h, list_walk):
    """one correction on the resident scan + count + graph, the blocks listed by the second walk or from the staged descriptors; what it left"""
    old = os.environ.get(SWITCH)
    os.environ[SWITCH] = "1" if list_walk else "0"
    try:
        st = h.ec(EDIST, C_MIN, ARC_F)
    finally:
        if old is None:
            del os.environ[SWITCH]
        else:
            os.environ[SWITCH] = old
    got = {k: h.fetch(k) for k in EA.OUT}
    got["EC_BLOCK_WORK"] = h.fetch("EC_BLOCK_WORK").reshape(-1, 12).copy()
    got["EC_BLOCK_OUT"] = h.fetch("EC_BLOCK_OUT").reshape(-1, 12)[:, OUT_COLS].copy()
    got["stats"] = np.array(st[:11], np.uint64)
    return got


def assert_same(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.fixture(scope="module")
def runs(hip):
    reads = EA.case_reads(hip)
    ref = None
    if R.available():
        from test_gpu_dropin import device_dbs
        db, scm = device_dbs(hip, reads, K, S)            # the device's scan + count, resident, and as the reference's structs
    else:
        seq, off, lens = pack_reads(reads)
        hip.scan_host(seq, off, lens, K, S)
        hip.count()
    n_scm = hip.fetch("N_SCM")
    hip.ec_graph()
    two = correct(hip, True)
    one = correct(hip, False)
    if R.available():
        from test_gpu_ec_routes import reference_run
        ref = reference_run(db, scm, K, S, EDIST, C_MIN, 10 * C_MIN, C_MIN, ARC_F)
    return {"reads": reads, "n_scm": n_scm, "two": two, "one": one, "ref": ref}


def test_one_walk_gives_what_two_walks_give(runs):
    assert_same(runs["two"], runs["one"], "one walk against two")
    assert len(runs["one"]["EC_BLOCK_WORK"]) > 0 and int(runs["one"]["EC_N_SCM"].sum()) == len(runs["one"]["EC_KMER"]) > 0


def test_cases_are_present(runs):
    """the cases the read set is there for, from the work list of the one walk (EcWork: word 4 the read, 7 r, 2 and 3 end_utg)"""
    w = runs["one"]["EC_BLOCK_WORK"]
    n_scm, n_reads = runs["n_scm"].astype(np.int64), len(runs["reads"])
    read, lead, is_open = w[:, 4].astype(np.int64), w[:, 7] != 0, (w[:, 2] == 0xFFFFFFFF) & (w[:, 3] == 0xFFFFFFFF)
    nb = np.bincount(read, minlength=n_reads)
    assert n_reads % 4 != 0
    assert np.all(np.diff(read) >= 0)                      # read order, a read's blocks together
    first = np.flatnonzero(np.r_[True, np.diff(read) != 0])
    last = np.r_[first[1:], len(read)] - 1
    assert np.all(lead[first]) and np.count_nonzero(lead) == len(first) and np.all(is_open[last])
    none = np.flatnonzero(nb == 0)
    assert np.any(n_scm[none] > 0) and np.any(n_scm[none] == 0)       # no block: with and without syncmers
    assert np.array_equal(runs["one"]["EC_N_SCM"][none], runs["n_scm"][none])
    assert np.any(nb == 2)                                  # clean reads: the leading and the open block only
    for n in (64, 65):
        assert np.any((n_scm == n) & (nb == 2)) and np.any((n_scm == n) & (nb > 2)), n
    assert nb.max() > 64
    assert np.all(nb <= n_scm + 1)                          # the bound the staging array relies on


@pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")
def test_one_walk_gives_what_the_reference_gives(runs):
    sr1, sc1, summary, marks = runs["ref"]
    for name, got in (("two", runs["two"]), ("one", runs["one"])):
        assert np.array_equal(got["EC_N_SCM"], sr1["n_scm"]), name
        assert np.array_equal(got["EC_KMER"], sr1["k_mer"]), name
        assert np.array_equal(got["EC_MPOS"], sr1["m_pos"]), name
        assert np.array_equal(got["EC_SMER"], sr1["s_mer"]), name
        assert np.array_equal(got["EC_SCM_COV"], sc1["cov"]), name
        assert np.array_equal(got["EC_SCM_DEL"], sc1["del"]), name
        assert np.array_equal(got["EC_SCM_OCC"], sc1["occ"]), name
        st = got["stats"]
        assert int(st[0] + st[5] + st[10]) == summary["total"] and int(st[2] + st[7]) == summary["corrected"], name


@pytest.mark.parametrize("drop", [1, 2, 3])
def test_last_workgroup_partly_filled(hip, drop):
    """the last workgroup of the walk holds fewer than its four reads, and the last one of the kernel that builds the work items fewer than its 256"""
    reads = EA.case_reads(hip)[:-drop]
    seq, off, lens = pack_reads(reads)
    hip.scan_host(seq, off, lens, K, S)
    hip.count()
    hip.ec_graph()
    assert_same(correct(hip, True), correct(hip, False), "drop %d" % drop)


def test_sid0_above_zero(hip, runs):
    reads = runs["reads"]
    seq, off, lens = pack_reads(reads)
    sid0 = 70001
    hip.scan_host(seq, off, lens, K, S, sid0=sid0)
    hip.count()
    hip.ec_graph()
    two, one = correct(hip, True), correct(hip, False)
    assert_same(two, one, "sid0")
    for k in ("EC_N_SCM", "EC_KMER", "EC_MPOS", "EC_SMER", "EC_SCM_COV"):
        assert np.array_equal(one[k], runs["one"][k]), k
    assert np.array_equal(one["EC_SCM_OCC"], runs["one"]["EC_SCM_OCC"] + (np.uint64(sid0) << np.uint64(32)))


def test_appended_batch(hip, runs):
    reads = runs["reads"]
    cuts = (0, 1, 203, 204, len(reads))
    piece, main = HipSyncasm(0), HipSyncasm(0)
    try:
        main.scan_begin(K, S)
        for a, b in zip(cuts[:-1], cuts[1:]):
            sq, of, ln = pack_reads(reads[a:b])
            piece.scan_host(sq, of, ln, K, S, sid0=a)
            main.scan_append(piece)
        main.count()
        main.ec_graph()
        two, one = correct(main, True), correct(main, False)
        assert_same(two, one, "appended")
        assert_same({k: one[k] for k in EA.OUT}, {k: runs["one"][k] for k in EA.OUT}, "appended against one scan")
    finally:
        piece.close()
        main.close()
