"""GPU: the error blocks listed in ONE walk over the chains (ec.hpp: ec_stage_blocks_wave_kernel stages a descriptor per block, ec_fill_work_kernel builds
the work items behind the scan) against the blocks the CPU oracle's driver visits on the same scan and count (oracle/ec.c: orc_ec_reads_blocks, through
tests/ec_util.py: oracle_round) and, where oracle/_ref is built, against the compiled reference's read_error_correction.

The read sets are tests/test_gpu_ec_assemble.py's, whose test_cases_are_present holds them to the cases that matter here as well: reads with no block, clean
reads (the leading and the open block only), 64 and 65 syncmers (the last chain a wave walks, the first that lane 0 walks alone), more than 64 blocks, a
read count that is no multiple of the four reads of a workgroup, sid0 > 0, a batch assembled by oatk_hip_scan_append.

What is compared: the work list (EC_BLOCK_WORK, twelve words per EcWork).  Words 0 - 7 (beg_utg, end_utg, read, beg_pos, l, r) are the oracle's block, row
by row in read and chain order; word 11 (`pad`) follows from the oracle's beg and end and the chain's length by the formula in ec_work_of.  Words 8 - 10
(hs16, lp, ln) are indices into this handle's layout -- where the read's hoco string lies, where the live arcs of beg_utg lie -- which the oracle has no
counterpart for and the solver consumes: a wrong one gives a block another outcome, so they are held by EC_BLOCK_OUT (the statistics counted from its
status column are the oracle's; between runs on the same reads its columns OUT_COLS are the same) and by the corrected chains, which are the oracle's
(test_gpu_ec_assemble.OUT).  copy_n, keep_all and the descriptors reach nothing but those chains.  Of EcBlockOut's twelve words two are no function of the
input and are left out, as tests/test_gpu_ec_seq.py leaves them out: path_off (the pool hands out chunks by atomics) and ticks (a clock)."""
import numpy as np
import pytest

import ref_lib as R
import test_gpu_ec_assemble as EA
from oatk_amd import HipSyncasm, pack_reads
from test_gpu_ec_assemble import runs  # noqa: F401  (the module's fixture: one correction of the case reads, the oracle's round and block list beside it)
from test_gpu_ec_seq import OUT_COLS

pytestmark = pytest.mark.gpu

K, S = EA.K, EA.S


def blocks_of(h):
    """the work list and the outcomes the last correction on `h` left"""
    return h.fetch("EC_BLOCK_WORK").reshape(-1, 12).copy(), h.fetch("EC_BLOCK_OUT").reshape(-1, 12).copy()


def assert_work_is_the_oracles(work, out, blocks, n_scm, stats, what):
    """blocks: the oracle's rows (read, beg, end, beg_utg, end_utg, beg_pos, l, r); stats: its block statistics"""
    assert len(work) == len(blocks), what
    m32 = np.uint64(0xFFFFFFFF)
    want = np.zeros((len(blocks), 8), np.uint32)
    for w, col in ((0, 3), (2, 4)):
        want[:, w], want[:, w + 1] = (blocks[:, col] & m32).astype(np.uint32), (blocks[:, col] >> np.uint64(32)).astype(np.uint32)
    for w, col in ((4, 0), (5, 5), (6, 6), (7, 7)):
        want[:, w] = (blocks[:, col] & m32).astype(np.uint32)
    for w in range(8):
        assert np.array_equal(work[:, w], want[:, w]), (what, "word %d" % w)
    # pad, as ec_work_of has it: what the read keeps of the block when it is not corrected
    read, beg, end, lead = blocks[:, 0].astype(np.int64), blocks[:, 1].astype(np.int64), blocks[:, 2].astype(np.int64), blocks[:, 7] != 0
    n = n_scm.astype(np.int64)[read]
    last = np.minimum(end, n)
    pad = np.where(lead, beg, np.where((beg + 1 < n) & (last > beg + 1), last - beg - 1, 0))
    assert np.array_equal(work[:, 11].astype(np.int64), pad), (what, "pad")
    assert np.all(np.bincount(read, minlength=len(n_scm)) <= n_scm.astype(np.int64) + 1), what      # the bound the staging array relies on
    # the statistics, counted from the outcomes the way ec_block_stats_kernel counts them
    is_open, status, short = (work[:, 2] == 0xFFFFFFFF) & (work[:, 3] == 0xFFFFFFFF), out[:, 0].astype(np.int64), out[:, 5] != 0
    st = np.zeros(11, np.int64)
    st[10] = int(short.sum())
    for base, sel in ((0, is_open & ~short), (5, ~is_open & ~short)):
        st[base] = int(sel.sum())
        st[base + 1:base + 5] = np.bincount(status[sel], minlength=4)[:4]
    assert np.array_equal(st, stats.astype(np.int64)), (what, "statistics")


def test_one_walk_gives_what_two_walks_give(runs):
    """(the walk it is held to is the oracle's, which visits every block as syncerr.c does)"""
    assert_work_is_the_oracles(runs["work"], runs["out"], runs["blocks"], runs["n_scm"], runs["oracle"]["stats"], "one walk against the oracle's")
    EA.assert_same(runs["oracle"], runs["seg"], "one walk against the oracle's round")
    assert len(runs["work"]) > 0 and int(runs["seg"]["EC_N_SCM"].sum()) == len(runs["seg"]["EC_KMER"]) > 0


def test_cases_are_present(runs):
    """the cases the read set is there for, from the work list of the one walk (EcWork: word 4 the read, 7 r, 2 and 3 end_utg)"""
    w = runs["work"]
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
    assert np.array_equal(runs["seg"]["EC_N_SCM"][none], runs["n_scm"][none])
    assert np.any(nb == 2)                                  # clean reads: the leading and the open block only
    for n in (64, 65):
        assert np.any((n_scm == n) & (nb == 2)) and np.any((n_scm == n) & (nb > 2)), n
    assert nb.max() > 64
    assert np.all(nb <= n_scm + 1)                          # the bound the staging array relies on


@pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")
def test_one_walk_gives_what_the_reference_gives(runs):
    sr1, sc1, summary, marks = runs["ref"]
    got = runs["seg"]
    assert np.array_equal(got["EC_N_SCM"], sr1["n_scm"])
    assert np.array_equal(got["EC_KMER"], sr1["k_mer"])
    assert np.array_equal(got["EC_MPOS"], sr1["m_pos"])
    assert np.array_equal(got["EC_SMER"], sr1["s_mer"])
    assert np.array_equal(got["EC_SCM_COV"], sc1["cov"])
    assert np.array_equal(got["EC_SCM_DEL"], sc1["del"])
    assert np.array_equal(got["EC_SCM_OCC"], sc1["occ"])
    st = got["stats"]
    assert int(st[0] + st[5] + st[10]) == summary["total"] and int(st[2] + st[7]) == summary["corrected"]


@pytest.mark.parametrize("drop", [1, 2, 3])
def test_last_workgroup_partly_filled(hip, drop):
    """the last workgroup of the walk holds fewer than its four reads, and the last one of the kernel that builds the work items fewer than its 256"""
    reads = EA.case_reads(hip)[:-drop]
    seq, off, lens = pack_reads(reads)
    hip.scan_host(seq, off, lens, K, S)
    hip.count()
    hip.ec_graph()
    got = EA.correct(hip)
    work, out = blocks_of(hip)
    orc, blocks = EA.oracle(hip, off, blocks=True)
    assert_work_is_the_oracles(work, out, blocks, hip.fetch("N_SCM"), orc["stats"], "drop %d" % drop)
    EA.assert_same(orc, got, "drop %d" % drop)


def test_sid0_above_zero(hip, runs):
    reads = runs["reads"]
    seq, off, lens = pack_reads(reads)
    sid0 = 70001
    hip.scan_host(seq, off, lens, K, S, sid0=sid0)
    hip.count()
    hip.ec_graph()
    one = EA.correct(hip)
    work, out = blocks_of(hip)
    # the same blocks with the same outcomes as at sid0 = 0, which test_one_walk_gives_what_two_walks_give holds to the oracle; the occurrences' read ids moved by sid0
    assert work.tobytes() == runs["work"].tobytes() and out[:, OUT_COLS].tobytes() == runs["out"][:, OUT_COLS].tobytes()
    for k in ("EC_N_SCM", "EC_SCM_OFF", "EC_KMER", "EC_MPOS", "EC_SMER", "EC_SCM_COV", "EC_SCM_DEL", "EC_SCM_OCC_OFF", "stats"):
        assert np.array_equal(one[k], runs["seg"][k]), k
    assert np.array_equal(one["EC_SCM_OCC"], runs["seg"]["EC_SCM_OCC"] + (np.uint64(sid0) << np.uint64(32)))


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
        one = EA.correct(main)
        work, out = blocks_of(main)
        assert_work_is_the_oracles(work, out, runs["blocks"], runs["n_scm"], runs["oracle"]["stats"], "appended against the oracle's blocks for these reads")
        EA.assert_same(runs["oracle"], one, "appended against the oracle's round on these reads")
        # against one scan: everything but hs16 (word 8), which says where the read lies in this batch's stream
        cols = [c for c in range(12) if c != 8]
        assert work[:, cols].tobytes() == runs["work"][:, cols].tobytes() and out[:, OUT_COLS].tobytes() == runs["out"][:, OUT_COLS].tobytes()
        EA.assert_same(one, runs["seg"], "appended against one scan")
    finally:
        piece.close()
        main.close()
