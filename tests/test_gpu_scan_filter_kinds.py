"""GPU: kernel B's fast path (scan_syncmer_fast.hpp) across the forms its filter and its syncmer count choose between, bit-exact against the CPU oracle on
every field of test_gpu_scan.SCAN_FIELDS.

For every tile a wave first asks two cheap questions of its 64 lanes -- does any chunk hold a Close candidate (the chunk's minimum against the Close bound), does
any hold an Open candidate (the minima of the two groups of window starts against the two Open bounds) -- and then runs the per-position loop not at all, in a
form that only knows Close, in one that only knows Open, or in the form that knows both (the waves at a read's ends always take the last).  The syncmers it
found are then ranked inside the wave: nothing at all when there are none, a count of the lanes below when no lane holds two, a wave scan otherwise.  What can
go wrong is therefore tied to WHICH kinds meet in one wave and tile and to HOW the syncmers of a wave are spread over its lanes:

  * a wave-tile with only Close syncmers, with only Open syncmers, with both;
  * a tile in which one wave has syncmers and a later one has none, and the other way round (the count of the empty wave is still read by the other);
  * two syncmers inside one lane's chunk; two lanes of a wave with one each and no lane with two (ranks from the lane mask); a lane with two and another with
    one (ranks from the scan);
  * a syncmer in the first wave of a read in which a k-mer ends and in its last wave (the edge form);
  * tandem repeats of period 2, 3 and 7 (ties, repeat mode, tiles with more syncmers than a short list holds);
  * everything again with room for one and for two syncmers in the list (oatk_hip_debug_list_cap).

The reads are cut from one sequence the oracle has scanned, in the manner of test_gpu_scan_tile_parity.py: without ties the rule looks at the k-mer alone, so a
syncmer of the sequence stays one wherever the read is cut, and the cut decides the tile, the wave, the lane and the position inside the lane's chunk that its
k-mer ends on.  The sequence is searched (seed after seed, on the CPU) until it offers every arrangement; that each class occurs is then read from the oracle's
records of the READS, not from the construction: the kind of a record is Close where the strand bit of its s-mer code differs from that of its position (Close
stores the code with the bit flipped), Open where they agree.  Every target is placed in an odd and in an even tile in the full forms.

(K, S) = (1001, 31) is the headline form (two waves, tiles of 1024 positions), (1061, 31) the four-wave form on the 4096-slot ring (tiles of 2048), (1001, 29) a
form with S != 31; K = 1002 ... 1008 at S = 31 run a short set each (one tile parity, no repeats, the list's own capacity), which with 1001 covers the eight
alignments of the window against the chunks.  No read is filtered out anywhere: the number compared is asserted against the number constructed."""
import numpy as np
import pytest

import oracle_lib as O
from test_gpu_scan_tile_parity import TAIL, UNITS, WAVE, no_repeat_dna, takes_fast_path, tile_of

C = 8                               # positions of a lane per tile (one chunk)
FULL = [(1001, 31), (1061, 31), (1001, 29)]
SHORT = [(K, 31) for K in range(1002, 1009)]
CAPS = [0, 1, 2]                    # 0: the list's own capacity
BASE_LEN = 60000
SEEDS = 60
CLASSES = {"close_only", "open_only", "both", "has_then_none", "none_then_has", "two_in_lane", "mask_rank", "scan_rank", "edge_first", "edge_last"}


def records(want, K):
    """per read: k-mer ends and kinds (1 Close, 2 Open) of its syncmers, from the oracle's records"""
    off = np.r_[0, np.cumsum(want["n_scm"].astype(np.int64))]
    mp, sm = want["m_pos"].astype(np.int64), want["s_mer"]
    E = (mp >> 1) + K - 1
    kind = np.where(((sm ^ mp.astype(np.uint64)) & np.uint64(1)) == 1, 1, 2)
    return [(E[off[r]:off[r + 1]], kind[off[r]:off[r + 1]]) for r in range(len(off) - 1)]


def classes_of(want, K, T):
    """which of CLASSES occur in the reads the oracle scanned"""
    found, nw = set(), T // WAVE
    for (E, kind), hl in zip(records(want, K), want["hoco_l"].astype(np.int64)):
        if len(E) == 0:
            continue
        g = E // WAVE
        for gg in np.unique(g):
            e, k = E[g == gg], set(kind[g == gg].tolist())
            found.add({(1,): "close_only", (2,): "open_only", (1, 2): "both"}[tuple(sorted(k))])
            per_lane = np.bincount(e // C - gg * (WAVE // C))
            if per_lane.max() >= 2:
                found.add("two_in_lane")
            if per_lane.max() == 1 and per_lane.sum() >= 2:
                found.add("mask_rank")
            if per_lane.max() >= 2 and (per_lane > 0).sum() >= 2:
                found.add("scan_rank")
            if gg * WAVE + 1 < K:
                found.add("edge_first")
            if gg * WAVE + WAVE > hl:
                found.add("edge_last")
        for t in np.unique(E // T):
            # the waves of this tile that decide anything: a k-mer ends in them, and they start inside the read
            cnt = [(int(((E >= b) & (E < b + WAVE)).sum())) for b in range(t * T, (t + 1) * T, WAVE) if b + WAVE >= K and b < hl]
            for a in range(len(cnt)):
                for b in range(a + 1, len(cnt)):
                    if cnt[a] and not cnt[b]:
                        found.add("has_then_none")
                    if cnt[b] and not cnt[a]:
                        found.add("none_then_has")
    return found


class Missing(Exception):
    pass


def construct(base, Eb, kd, K, T, full, rng):
    """reads that put syncmers of `base` (k-mer ends Eb, ascending; kinds kd) where the docstring says"""
    n = len(Eb)
    gap_before = np.r_[Eb[0] - (K - 1), np.diff(Eb)]
    gap_after = np.r_[np.diff(Eb), len(base) - Eb[-1]]
    reads = []

    def cut(anchor, E, L=None):
        """the read in which base position `anchor` is position E; None if the sequence does not reach"""
        L = E + 1 + TAIL if L is None else L
        p = anchor - E
        return base[p:p + L] if p >= 0 and p + L <= len(base) and E >= K - 1 else None

    def put(cands, E, L=None):
        """the first candidate (an index into Eb) that can be cut that way"""
        for i in cands:
            r = cut(int(Eb[i]), E, L)
            if r is not None:
                reads.append(r)
                return
        raise Missing

    idx = np.arange(n)
    alone = (gap_before > WAVE + 16) & (gap_after > WAVE + 16)
    for tt in ((1, 2) if full else (1,)):
        t0 = tt * T
        put(idx[alone & (kd == 1)], t0 + 200)                                   # a wave-tile with one Close and nothing else (lane 25, position 0 of its chunk)
        put(idx[alone & (kd == 2)], t0 + WAVE + 301)                            # ... with one Open (second wave, position 5)
        put(idx[:-1][(kd[:-1] != kd[1:]) & (gap_after[:-1] < 400)], t0 + 50)    # a Close and an Open in one wave-tile
        put(idx[gap_after > WAVE + 16], t0 + WAVE - 4)                          # the last syncmer of wave 0, none in wave 1
        put(idx[1:][gap_before[1:] > WAVE + 16], t0 + WAVE + 3)                 # none in wave 0, the first of wave 1
        pair = idx[:-1][gap_after[:-1] < C]
        put(pair, t0 + C * 13)                                                  # two in one chunk (positions 0 and gap)
        put(pair, t0 + C * 13 + 7)                                              # the same two in neighbouring lanes
        put(idx[:-1][(gap_after[:-1] >= C) & (gap_after[:-1] < 400)], t0 + WAVE + 16)     # two lanes further apart
        # a lane with two and another lane with one: a pair and a neighbour within one wave, the pair's first on position 0 of a chunk
        done = False
        for a in pair:
            for grp in ([a - 1, a, a + 1], [a, a + 1, a + 2]):
                if grp[0] < 0 or grp[-1] >= n or Eb[grp[-1]] - Eb[grp[0]] > WAVE - 2 * C:
                    continue
                first = int(Eb[grp[0]])
                o = (C - (int(Eb[a]) - first) % C) % C                           # offset of the group's first in the wave: the pair's first lands on a multiple of 8
                r = cut(first, t0 + o)
                if r is not None and not done:
                    reads.append(r)
                    done = True
        if not done:
            raise Missing
        put(idx, t0 + 299, t0 + 300)                                            # the k-mer that ends on the read's last position, in the read's last wave
        put(idx, t0 + WAVE + 17, t0 + WAVE + 22)                                # ... and one a few positions in front of the end
    put(idx, K - 1)                                                             # a syncmer as the read's first k-mer: the first wave in which a k-mer ends
    if full:
        put(idx, K + 10)
        for unit in UNITS:
            for lead in (T + 5, 2 * T + 5):                 # the repeat starts in tile 1 (odd) / tile 2 (even), runs for three tiles, ordinary sequence follows
                rep = (unit * (3 * T // len(unit) + 1))[:3 * T]
                reads.append(no_repeat_dna(rng, lead, not_last=rep[0]) + rep + no_repeat_dna(rng, T + 300, not_first=rep[-1]))
    return reads


def n_expected(full):
    return 11 * 2 + 2 + 2 * len(UNITS) if full else 11 + 1


def build(K, S, full):
    """search the seeds for a sequence that offers every arrangement"""
    T = tile_of(K, S)
    for seed in range(SEEDS):
        rng = np.random.default_rng([K, S, int(full), seed])
        base = no_repeat_dna(rng, BASE_LEN)
        w = O.scan([base], K, S, mode=0)
        assert int(w["hoco_l"][0]) == BASE_LEN
        (Eb, kd), = records(w, K)
        assert np.all(np.diff(Eb) > 0)                      # (Close and Open at one position cancel: one record per k-mer end)
        try:
            reads = construct(base, Eb, kd, K, T, full, rng)
        except Missing:
            continue
        want = O.scan(reads, K, S, mode=0)
        if CLASSES <= classes_of(want, K, T):
            return reads, want
    raise AssertionError("no sequence among %d seeds offers every arrangement at K = %d, S = %d" % (SEEDS, K, S))


_cache = {}


def case(K, S, full):
    if (K, S) not in _cache:
        _cache[(K, S)] = build(K, S, full)
    return _cache[(K, S)]


@pytest.mark.parametrize("K,S,full", [(K, S, True) for K, S in FULL] + [(K, S, False) for K, S in SHORT])
def test_premises(K, S, full):
    """every class of the docstring occurs in the inputs, read from the oracle's output"""
    assert takes_fast_path(K, S)
    reads, want = case(K, S, full)
    T = tile_of(K, S)
    hl, n_scm = want["hoco_l"].astype(np.int64), want["n_scm"].astype(np.int64)
    assert len(hl) == len(reads) == n_expected(full)
    assert [len(r) for r in reads] == hl.tolist()                   # no two equal neighbours: hoco positions are bases
    assert all(K <= L <= 7 * T for L in hl)                         # every read holds a k-mer; a handful of tiles at the most (the repeats: six and a bit)
    assert classes_of(want, K, T) >= CLASSES
    if full:
        # the repeats: some tile holds more syncmers than a list of one or two, so the direct path of flush() is taken with both
        rec = records(want, K)
        per_tile = max(np.bincount(E // T).max() for E, _ in rec[-2 * len(UNITS):] if len(E))
        assert per_tile >= 3
        # ... and the targets sit in an odd and in an even tile
        assert {int(t) & 1 for E, _ in rec for t in E // T} == {0, 1}
    assert {(-(K - S)) % 8 for K, S in [FULL[0]] + SHORT} == set(range(8))


@pytest.mark.gpu
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("K,S", FULL)
def test_filter_kinds(hip, K, S, cap):
    import test_gpu_scan as G
    reads, want = case(K, S, True)
    hip.debug_list_cap(cap)
    try:
        got, _ = G.run_hip(hip, reads, K, S)
    finally:
        hip.debug_list_cap(0)
    assert got["hoco_l"].shape[0] == len(reads) == n_expected(True)
    G.compare_scan(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("K,S", SHORT)
def test_filter_kinds_window_alignments(hip, K, S):
    import test_gpu_scan as G
    reads, want = case(K, S, False)
    got, _ = G.run_hip(hip, reads, K, S)
    assert got["hoco_l"].shape[0] == len(reads) == n_expected(False)
    G.compare_scan(got, want)
