"""GPU: kernel B's fast path (scan_syncmer_fast.hpp) across the things it keeps from one tile to the next, bit-exact against the CPU oracle on every field of
test_gpu_scan.SCAN_FIELDS.

Between two tiles the kernel carries ring addresses that alternate between two values (a tile is half the ring), the parity of the count buffer and of the tie
flags, the pending set of the tile before (its syncmers are appended one tile late, behind the next tile's barrier), the list of the read's syncmers in LDS, and
repeat mode, which a tie switches on for the tile after next and two quiet tiles switch off again.  A wave may leave the loop a tile before the others.  What can go
wrong is therefore tied to WHICH tile something happens in -- an even or an odd one -- and to where the read ends against the tile and wave boundaries:

  * loop parity: reads of one to five tiles, each one position short of, on and one position behind every wave boundary of its last tile (the last is the tile
    boundary): the loop ends, and a later wave leaves early, after an even tile and after an odd one;
  * syncmers at tile edges: reads cut from one sequence the oracle has scanned, so that a known closed syncmer's k-mer ends on the last position of a tile, on the
    first of the next and one position inside, for an even-numbered and an odd-numbered tile (the rule looks at the k-mer alone: it stays a syncmer wherever the
    read is cut), and reads with a syncmer as their first k-mer (m_pos 0), whose ranges read ring slots that still hold the initial MAX;
  * the pending set and the list: everything again with room for one and for two syncmers in the list (oatk_hip_debug_list_cap), so that the list is written out in
    the middle of a read and a tile with more syncmers than it holds goes straight to records, at both parities;
  * ties: tandem repeats of period 2, 3 and 7, three tiles long, behind one tile and behind two of ordinary sequence, with ordinary sequence after them: repeat
    mode goes on and off in an even and in an odd tile.

(K, S) = (1001, 31) is the headline form (two waves, tiles of 1024 positions), (1061, 31) the four-wave form on the 4096-slot ring (tiles of 2048), (1001, 29) a
form with S != 31; K = 1002 ... 1008 at S = 31 run a short set each, which with 1001 covers the eight alignments of the window against the chunks.

The reads have no two equal neighbouring bases: homopolymer compression leaves them as they are, and a length in bases is a length in hoco positions (asserted
from the oracle's hoco_l).  No read is filtered out anywhere: the number compared is asserted against the number the construction gives."""
import numpy as np
import pytest

import oracle_lib as O

WAVE = 512                          # positions of a wave per tile (64 lanes, 8 positions each)
FULL = [(1001, 31), (1061, 31), (1001, 29)]
SHORT = [(K, 31) for K in range(1002, 1009)]
CAPS = [0, 1, 2]                    # 0: the list's own capacity
BASE_LEN = 24000
TAIL = 700                          # what follows an edge syncmer's k-mer: the tile after it is run as well
UNITS = (b"AC", b"ACG", b"ACGTAGC")


def tile_of(K, S):
    return 1024 if K - S < 1024 else 2048


def takes_fast_path(K, S):
    """scan_syncmer_fast.hpp: syncmer_fast_ring"""
    d = (K - S) // 8 - 1
    return 64 <= d < 128 and K + 2048 + 8 + 64 <= 4096


def no_repeat_dna(rng, n, not_first=None, not_last=None):
    """n bases, no two neighbours equal; the first / last base differs from the given one (so the piece can be joined to another)"""
    while True:
        a = (int(rng.integers(0, 4)) + np.r_[0, np.cumsum(rng.integers(1, 4, n - 1))]) % 4
        s = bytes(np.frombuffer(b"ACGT", np.uint8)[a])
        if (not_first is None or s[0] != not_first) and (not_last is None or s[-1] != not_last):
            return s


def parity_lengths(T, tiles):
    """for every number of tiles: one short of, on and one behind every wave boundary of the last tile"""
    out = []
    for n in tiles:
        for b in range(WAVE, T + 1, WAVE):
            out += [(n - 1) * T + b + d for d in (-1, 0, 1)]
    return out


def edge_targets(T):
    """k-mer ends on the last position of tile t, the first of tile t + 1 and one position inside it, t even and t odd"""
    return [(t + 1) * T + d for t in (0, 1) for d in (-1, 0, 1)]


def n_expected(K, S, full):
    T = tile_of(K, S)
    n = len(parity_lengths(T, (1, 2, 3, 4, 5) if full else (2, 3))) + len(edge_targets(T))
    n += 4 if full else 1                        # first-k-mer reads
    n += 2 * len(UNITS) if full else 0           # tandem repeats
    return n


def build(K, S, full):
    T = tile_of(K, S)
    rng = np.random.default_rng(K * 1000 + S * 10 + full)
    base = no_repeat_dna(rng, BASE_LEN)
    scm = np.sort(O.scan([base], K, S, mode=0)["m_pos"].astype(np.int64) >> 1)        # k-mer starts of the base sequence's closed syncmers
    assert len(scm) >= 16
    reads, kind = [], []
    for i, L in enumerate(parity_lengths(T, (1, 2, 3, 4, 5) if full else (2, 3))):
        p = (211 * i) % (BASE_LEN - L)
        reads.append(base[p:p + L]), kind.append(("parity", L, None))
    for i, E in enumerate(edge_targets(T)):                 # a syncmer's k-mer [j, j + K) with its end at position E of the read
        assert E >= K - 1
        ok = scm[(scm + K - 1 >= E) & (scm + K + TAIL <= BASE_LEN)]
        j = int(ok[(5 * i + 1) % len(ok)])
        p = j + K - 1 - E
        reads.append(base[p:p + E + 1 + TAIL]), kind.append(("edge", E + 1 + TAIL, E - K + 1))
    for i, L in enumerate((K, T + 1, 2 * T, 3 * T - 1) if full else (2 * T + 1,)):      # a syncmer as the first k-mer
        ok = scm[scm + L <= BASE_LEN]
        j = int(ok[(7 * i + 2) % len(ok)])
        reads.append(base[j:j + L]), kind.append(("first", L, 0))
    if full:
        for unit in UNITS:
            for lead in (T + 5, 2 * T + 5):                 # the repeat starts in tile 1 (odd) / tile 2 (even), runs for three tiles, ordinary sequence follows
                rep = (unit * (3 * T // len(unit) + 1))[:3 * T]
                r = no_repeat_dna(rng, lead, not_last=rep[0]) + rep + no_repeat_dna(rng, T + 300, not_first=rep[-1])
                reads.append(r), kind.append(("tandem", len(r), None))
    assert len(reads) == n_expected(K, S, full)
    return reads, kind


_cache = {}


def case(K, S, full):
    if (K, S) not in _cache:
        reads, kind = build(K, S, full)
        _cache[(K, S)] = (reads, kind, O.scan(reads, K, S, mode=0))
    return _cache[(K, S)]


@pytest.mark.parametrize("K,S,full", [(K, S, True) for K, S in FULL] + [(K, S, False) for K, S in SHORT])
def test_premises(K, S, full):
    """the inputs are what the docstring says, read from the oracle's output"""
    assert takes_fast_path(K, S)
    reads, kind, want = case(K, S, full)
    T = tile_of(K, S)
    hl, n_scm = want["hoco_l"].astype(np.int64), want["n_scm"].astype(np.int64)
    assert len(hl) == len(reads) == n_expected(K, S, full)
    off = np.r_[0, np.cumsum(n_scm)]
    for r, (what, L, start) in enumerate(kind):
        assert hl[r] == len(reads[r]) == L, (r, what, L)            # no two equal neighbours: hoco positions are bases
        if start is not None:                                        # the syncmer the read was cut around is one of the read's, where it was put
            pos = want["m_pos"][off[r]:off[r + 1]].astype(np.int64) >> 1
            assert start in pos, (what, L, start)
    ends = sorted(s + K - 1 for what, _, s in kind if what == "edge")
    assert ends == [T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1]
    # a read ends, and a wave leaves the loop a tile early, after an even and after an odd number of tiles
    tiles = {(-(-L // T)) & 1 for what, L, _ in kind if what == "parity" and L >= K}
    early = {(-(-L // T)) & 1 for what, L, _ in kind if what == "parity" and L >= K and L % T and L % T <= T - WAVE}
    assert tiles == {0, 1} and early == {0, 1}
    assert int(n_scm.sum()) > 0
    if full:
        # some tile holds more syncmers than a list of one or two: the direct path of flush() is taken with both
        per_tile = max(np.bincount(((want["m_pos"][off[r]:off[r + 1]].astype(np.int64) >> 1) + K - 1) // T).max() for r in range(len(reads)) if n_scm[r])
        assert per_tile >= 3
    assert {(-(K - S)) % 8 for K, S in [FULL[0]] + SHORT} == set(range(8))


@pytest.mark.gpu
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("K,S", FULL)
def test_tile_parity(hip, K, S, cap):
    import test_gpu_scan as G
    reads, kind, want = case(K, S, True)
    hip.debug_list_cap(cap)
    try:
        got, _ = G.run_hip(hip, reads, K, S)
    finally:
        hip.debug_list_cap(0)
    assert got["hoco_l"].shape[0] == len(reads) == n_expected(K, S, True)
    G.compare_scan(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("K,S", SHORT)
def test_window_alignments(hip, K, S):
    import test_gpu_scan as G
    reads, kind, want = case(K, S, False)
    got, _ = G.run_hip(hip, reads, K, S)
    assert got["hoco_l"].shape[0] == len(reads) == n_expected(K, S, False)
    G.compare_scan(got, want)
