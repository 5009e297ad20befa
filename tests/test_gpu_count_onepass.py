"""GPU: the count's one pass over the sorted records (count.hpp: gather_verify_kernel) -- gather through the permutation, the table's rows at the
heads, and the check of every record that is no head against its PREDECESSOR, k-mer and s-mer -- against the CPU oracle, bit for bit, at the edges
of its tiles (256 records), its strips (8 records) and its 32-base words.

The batches are made of reads of exactly K bases without homopolymers that hold ONE syncmer each (cut out of one random sequence at the positions
the oracle finds syncmers at): a read is a record, so the number of records, the size of every group and -- the groups sorted by the oracle's
hashes -- the place of every group in sorted order are chosen, not found.  Under debug_hash_mask(0) every hash is 0, the whole batch is one hash
group and the sorted order is the read order: there the place of every differing record is chosen too."""
import functools

import numpy as np
import pytest

import adversarial as A
import oracle_lib as O
import test_gpu_record_path as RP
from oatk_amd import HipSyncasm, pack_reads

pytestmark = pytest.mark.gpu

FULL = RP.FULL
K0, S0 = 31, 11          # one 32-base word; a reverse-strand k-mer at position 0 starts one base in front of its read's words


@functools.lru_cache(maxsize=None)
def pool(K, S, need):
    """`need` reads of K bases with one syncmer each and different k-mers, as (hash, read, rev) in ascending order of the hash"""
    rng = np.random.default_rng(1000 + K)
    found = {}
    while len(found) < need:
        seq = A.rand_nohp(rng, K + (need + 2) * (K - S + 1))
        sc = O.scan([seq], K, S)
        for mp, h in zip(sc["m_pos"].tolist(), sc["k_mer"].tolist()):
            found.setdefault(int(h), (seq[(mp >> 1):(mp >> 1) + K], mp & 1))
    return tuple((h, r, rev) for h, (r, rev) in sorted(found.items())[:need])


def fill(total, cyc=(5, 1, 11, 2, 17, 3)):
    """group sizes from the cycle until they sum to `total` (the last one cut)"""
    out = []
    while sum(out) < total:
        out.append(min(cyc[len(out) % len(cyc)], total - sum(out)))
    return out


def grouped_reads(K, S, sizes, seed=3, first_rev=False):
    """sizes[j] copies of the pool's j-th k-mer (ascending hash: group j is the j-th in sorted order), either strand, in a shuffled read order"""
    rng = np.random.default_rng(seed)
    P = pool(K, S, max(len(sizes), 4))
    reads = []
    for (h, r, rev), m in zip(P, sizes):
        reads += [r if rng.integers(0, 2) else A.revcomp(r) for _ in range(m)]
    reads = [reads[i] for i in rng.permutation(len(reads))]
    if first_rev:            # the first read of the batch (word index 0 of the hoco string) holds its k-mer on the reverse strand, and occurs again
        j = next(j for j, m in enumerate(sizes) if m >= 3)
        h, r, rev = P[j]
        i = next(i for i, x in enumerate(reads) if x in (r, A.revcomp(r)))
        reads[i] = reads[0]
        reads[0] = A.revcomp(r) if rev == 0 else r
    return reads


def run(hip, reads, K, S, mask=FULL, collisions=0):
    """scan + count of `reads` on the device against the oracle's; returns the oracle's count"""
    seq, off, lens = pack_reads(reads)
    hip.debug_hash_mask(mask)
    try:
        hip.scan_host(seq, off, lens, K, S)
        scan, want = RP.oracle(reads, K, S, mask)
        assert np.array_equal(hip.fetch("N_SCM"), scan["n_scm"]) and (scan["n_scm"] == 1).all()            # a read is a record
        hip.count()
        compare(hip, want, collisions)
    finally:
        hip.debug_hash_mask(FULL)
    return scan, want


def compare(hip, want, collisions):
    got = hip.fetch_count()
    assert got["n_scm"] == want["n_scm"] and got["n_scm"] > 0
    for f in ("h", "s", "cov", "occ", "k_id"):
        assert np.array_equal(got[f], want[f]), f
    assert np.array_equal(got["occ_off"], np.concatenate([[0], np.cumsum(want["cov"], dtype=np.uint64)]).astype(np.uint64))
    assert hip.info()["collisions"] == collisions


# name -> group sizes in sorted order.  Tiles end at 256 and 512, strips at every multiple of 8.
EDGES = {
    "n1": [1],
    "n7": [3, 4],
    "n8": [5, 3],
    "n9_group_over_a_strip_edge": [4, 5],                      # records 4 .. 8
    "n255": fill(255),
    "n256": fill(256),
    "n257_group_over_the_tile_edge_last_no_head": fill(250) + [7],                     # records 250 .. 256: the record in front of tile 1 comes from the extra lane
    "n257_tile_starts_with_a_head_last_a_head": fill(256) + [1],
    "n513": fill(250) + [20] + fill(242) + [1],               # a group over 256, a head at 512 that is the last record
    "n513_group_over_both_tile_edges": fill(200) + [313],
}


@pytest.mark.parametrize("name", list(EDGES))
def test_tile_and_strip_edges(hip, name):
    sizes = EDGES[name]
    assert sum(sizes) == int(name[1:].split("_")[0])
    scan, want = run(hip, grouped_reads(K0, S0, sizes, first_rev=name == "n256"), K0, S0)
    assert want["cov"].tolist() == sizes                       # the layout in sorted order is the one asked for
    if name == "n256":     # kmer_word_global's masked branch: a reverse-strand k-mer at position 0 of the batch's first read, compared as a head
        assert int(scan["m_pos"][0]) == 1


def single_group_reads(pattern, K=K0, S=S0):
    """reads in the order of `pattern`, a string over the pool's k-mers 'A', 'B', ...; every other copy on the other strand"""
    P = pool(K, S, 16)
    return [P[ord(c) - 65][1] if i % 2 == 0 else A.revcomp(P[ord(c) - 65][1]) for i, c in enumerate(pattern)]


@pytest.mark.parametrize("pattern", [
    "A" * 256 + "B" * 3,                # the differing record is the first of a tile
    "AABB",                             # ... in the middle of a group
    "A" * 9 + "B",                      # ... the last record
    "AAAABBBAACCCB",                    # more than eight records with three k-mers
    "ABCDEFGHIJKL" * 25,                # twelve k-mers over two tiles: every record differs from the one in front of it
], ids=["first_of_a_tile", "middle", "last_record", "three_kmers", "twelve_kmers"])
def test_forced_collisions_in_one_hash_group(hip, pattern):
    """mask 0: one hash group in read order.  The s-mers differ inside it too: the pessimistic order decides them again on its final clusters"""
    scan, want = run(hip, single_group_reads(pattern), K0, S0, mask=0, collisions=1)
    first_seen = list(dict.fromkeys(pattern))
    assert want["cov"].tolist() == [pattern.count(c) for c in first_seen]


@functools.lru_cache(maxsize=None)
def last_base_pair(K, S):
    """two reads of K bases, one forward-strand syncmer each, that differ in the LAST base only: the last base of the oriented k-mer's last word"""
    for h, r, rev in pool(K, S, 12):
        if rev:
            continue
        for c in b"ACGT":
            if c in (r[-1], r[-2]):
                continue
            r2 = r[:-1] + bytes([c])
            sc = O.scan([r2], K, S)
            if sc["n_scm"].tolist() == [1] and sc["m_pos"].tolist() == [0]:
                return r, r2
    raise AssertionError("no forward-strand syncmer survives a change of its last base")


@pytest.mark.parametrize("K,S", [(31, 11), (45, 11), (1001, 31), (1057, 31)])       # one word with idle lanes; no multiple of 32; 32 words; two trips of the word loop
def test_kmer_word_edges(hip, K, S):
    # equal groups through the ordinary path, over a strip edge, both strands
    scan, want = run(hip, grouped_reads(K, S, [3, 9, 2]), K, S)
    assert want["cov"].tolist() == [3, 9, 2]
    # one difference in the last base of the last word, in one hash group with its neighbour
    a, b = last_base_pair(K, S)
    rc = A.revcomp
    scan, want = run(hip, [a, rc(a), a, b, rc(b), a, b, b, rc(a), a, b], K, S, mask=0, collisions=1)
    assert want["cov"].tolist() == [6, 5]


def test_appended_batch():
    """two pieces moved into one batch: the slot records come from pack_slots_kernel"""
    sizes = fill(250) + [9] + [4]
    reads = grouped_reads(K0, S0, sizes, seed=8)
    piece, main = HipSyncasm(0), HipSyncasm(0)
    try:
        main.scan_begin(K0, S0)
        for a, b in ((0, 101), (101, len(reads))):
            sq, of, ln = pack_reads(reads[a:b])
            piece.scan_host(sq, of, ln, K0, S0, sid0=a)
            main.scan_append(piece)
        scan, want = RP.oracle(reads, K0, S0)
        assert want["cov"].tolist() == sizes
        main.count()
        compare(main, want, 0)
    finally:
        piece.close()
        main.close()
