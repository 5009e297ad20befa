"""GPU: the way of a syncmer record from kernel B's shard regions to its slot.  The k-mer hash kernel reads the records where kernel B left
them and writes every per-slot array, the sort's key and value and the 32-byte slot record the count gathers; oatk_hip_count packs the slot
records itself only for a batch that was assembled from pieces.  Every per-slot array and everything the count derives from the slot records
-- ids, occurrence lists, and the k-mer locators as the EC graph's vertices see them (EC_VTX_SRC) -- against the CPU oracle, bit for bit:
(a) an ordinary batch, (b) a batch whose first pass overflows the shard regions, (c) a batch assembled by append, (d) masked hashes."""
import numpy as np
import pytest

import adversarial as A
import oracle_lib as O
from oatk_amd import HipSyncasm, pack_reads

pytestmark = pytest.mark.gpu

FULL = 0xFFFFFFFFFFFFFFFF


def oracle(reads, K, S, mask=FULL):
    """scan and count of the oracle; with a mask the count sees the hashes ANDed down (the per-read hashes stay whole, as POS_HASH does)"""
    oseq, ooff = O.pack_reads(reads)
    L = O.lib()
    out, p = O.scan_raw(oseq, ooff, K, S, 0)
    n = int(p.contents.tot_scm)
    scan = {"m_pos": np.array(out["m_pos"], copy=True), "s_mer": np.array(out["s_mer"], copy=True), "k_mer": np.array(out["k_mer"], copy=True),
            "n_scm": np.array(out["n_scm"], copy=True)}
    assert len(scan["k_mer"]) == n
    if mask != FULL:
        for i in range(n):
            p.contents.k_mer[i] &= mask
    cp = L.orc_count(p, K)
    cc = cp.contents
    want = {"n_scm": int(cc.n_scm), "h": O._arr(cc.h, cc.n_scm, np.uint64), "s": O._arr(cc.s, cc.n_scm, np.uint64),
            "cov": O._arr(cc.cov, cc.n_scm, np.uint32), "occ": O._arr(cc.occ, cc.tot_occ, np.uint64),
            "k_id": O._arr(cc.k_id, cc.tot_occ, np.uint64)}
    L.orc_count_free(cp)
    L.orc_scan_free(p)
    return scan, want


def check(hip, off, scan, want, c=5, a=0.35):
    """the resident scan of `hip` (reads at byte offsets `off`), counted here, against the oracle's"""
    off = np.asarray(off, np.uint64)
    assert np.array_equal(hip.fetch("N_SCM"), scan["n_scm"])
    scm_off = hip.fetch("SCM_OFF")
    assert np.array_equal(scm_off, np.concatenate([[0], np.cumsum(scan["n_scm"], dtype=np.uint64)]).astype(np.uint64))
    for name, f in (("POS_MPOS", "m_pos"), ("POS_SMER", "s_mer"), ("POS_HASH", "k_mer")):
        assert np.array_equal(hip.fetch(name), scan[f]), name
    hip.count()
    got = hip.fetch_count()
    assert got["n_scm"] == want["n_scm"] and got["n_scm"] > 0
    for f in ("h", "s", "cov", "occ", "k_id"):
        assert np.array_equal(got[f], want[f]), f
    occ_off = np.concatenate([[0], np.cumsum(want["cov"], dtype=np.uint64)]).astype(np.uint64)
    assert np.array_equal(got["occ_off"], occ_off)
    # a syncmer's k-mer is read where its FIRST occurrence lies: the hoco string of that read (a byte offset; two bits a base)
    first_read = (want["occ"][occ_off[:-1].astype(np.int64)] >> np.uint64(32)).astype(np.int64)
    hip.ec_graph()
    hip.ec_mark(c, a)
    assert np.array_equal(hip.fetch("EC_VTX_SRC"), off[first_read] // np.uint64(4))
    return got


def test_ordinary_batch(hip):
    K, S = 1001, 31
    reads = A.reads(K, S) + A.hifi_like(80, 40000, 9000, seed=4)
    seq, off, lens = pack_reads(reads)
    hip.scan_host(seq, off, lens, K, S)
    check(hip, off, *oracle(reads, K, S))
    # ... and a second count of the same scan finds the slot records it left
    check(hip, off, *oracle(reads, K, S))


def test_shard_regions_overflow_and_the_scan_runs_again():
    """a new handle sizes its shard regions from the batch's bytes; a dense small k (a syncmer every ten bases) does not fit them"""
    K, S = 25, 5
    reads = A.hifi_like(70, 40000, 9000, seed=9)
    seq, off, lens = pack_reads(reads)
    h = HipSyncasm(0)
    try:
        h.scan_host(seq, off, lens, K, S)
        assert h.info()["scan_retries"] >= 1
        check(h, off, *oracle(reads, K, S))
        # the regions are large enough now: the same batch in one pass, and a smaller one behind it (shards with fewer records than before)
        h.scan_host(seq, off, lens, K, S)
        assert h.info()["scan_retries"] == 0
        check(h, off, *oracle(reads, K, S))
        seq2, off2, lens2 = pack_reads(reads[:9])
        h.scan_host(seq2, off2, lens2, K, S)
        check(h, off2, *oracle(reads[:9], K, S))
    finally:
        h.close()


@pytest.mark.parametrize("K,S", [(301, 21), (1001, 31)])
def test_assembled_batch_packs_its_own_slot_records(K, S):
    reads = A.hifi_like(150, 50000, 2500 if K < 1000 else 7000, seed=K, err=0.001)
    cuts = (0, 1, 61, 150)
    piece, main = HipSyncasm(0), HipSyncasm(0)
    try:
        # the handle has scanned a batch of its own before (and holds that batch's slot records): the assembled one must not use them
        sq, of, ln = pack_reads(reads[40:130])
        main.scan_host(sq, of, ln, K, S)
        main.count()
        main.scan_begin(K, S)
        g_off, base = [], 0
        for a, b in zip(cuts[:-1], cuts[1:]):
            sq, of, ln = pack_reads(reads[a:b])
            piece.scan_host(sq, of, ln, K, S, sid0=a)
            main.scan_append(piece)
            g_off.extend((of + np.uint64(base)).tolist())
            base += int(sq.size)
        scan, want = oracle(reads, K, S)
        check(main, g_off, scan, want)
        # a piece behind a batch that was counted already: counted again, with the new slots
        more = A.hifi_like(30, 50000, 2500 if K < 1000 else 7000, seed=K + 1, err=0.001)
        sq, of, ln = pack_reads(more)
        piece.scan_host(sq, of, ln, K, S, sid0=len(reads))
        main.scan_append(piece)
        g_off.extend((of + np.uint64(base)).tolist())
        check(main, g_off, *oracle(reads + more, K, S))
        # ... and a scan of its own afterwards writes its slot records again
        sq, of, ln = pack_reads(reads[:50])
        main.scan_host(sq, of, ln, K, S)
        check(main, of, *oracle(reads[:50], K, S))
    finally:
        piece.close()
        main.close()


@pytest.mark.parametrize("mask", [0xFF, 0xFFC0000000FFFFFF])
def test_masked_hashes_split_and_gather_again(hip, mask):
    """hash groups that hold different k-mers: split_collisions / regather / finish_heads run on the slot records the scan wrote (0xFF), and a
    mask that merges nothing leaves the optimistic order alone"""
    K, S = 101, 11
    reads = A.hifi_like(200, 5000, 1500, seed=5)
    seq, off, lens = pack_reads(reads)
    hip.debug_hash_mask(mask)
    try:
        hip.scan_host(seq, off, lens, K, S)
        check(hip, off, *oracle(reads, K, S, mask))
        assert hip.info()["collisions"] == (1 if mask == 0xFF else 0)
    finally:
        hip.debug_hash_mask(FULL)
    # the mask is taken when the scan places the records: the next scan is whole again
    hip.scan_host(seq, off, lens, K, S)
    check(hip, off, *oracle(reads, K, S))
    assert hip.info()["collisions"] == 0
