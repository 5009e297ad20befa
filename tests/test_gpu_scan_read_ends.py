"""GPU: kernel B's fast path (scan_syncmer_fast.hpp) at the two ends of a read, bit-exact against the CPU oracle on every field of test_gpu_scan.SCAN_FIELDS.

The kernel classifies its waves once per tile: a wave wholly behind the read's end leaves the tile loop early and only keeps the workgroup's barriers
company, and a wave in which no k-mer ends (the first 512 positions of a read, the first 1024 on the four-wave form) hashes and skips the decision phase.
What can go wrong there is a syncmer lost or invented at the read's FIRST k-mer (its window is the first the decision phase sees) or at its LAST one (decided
in the wave that holds the read's end, beside waves that have already left), a count that reaches flush() from the wrong wave, or a barrier that a wave
misses (a hang).  So the read lengths sit on and around the wave and tile boundaries (512 positions per wave; tiles of 1024 on the 2048-slot ring, of 2048
on the 4096-slot ring), and for every length three reads are cut from one sequence the oracle has scanned: anywhere, with a closed syncmer as the first k-mer
(m_pos 0), and with one as the last (m_pos hoco_l - K) -- the rule looks at the k-mer alone, so a k-mer that is a syncmer stays one wherever the read is cut.

The reads have no two equal neighbouring bases: homopolymer compression leaves them as they are, and a length in bases is a length in hoco positions
(asserted from the oracle's hoco_l).  (K, S) = (1001, 31) is the headline form (two waves, w mod 8 = 2), (1007, 31) the same ring with w mod 8 = 0, and
(1061, 31) the 4096-slot ring with four waves and up to three of them behind the end."""
import numpy as np
import pytest

import oracle_lib as O

WAVE = 512                         # positions of a wave per tile (64 lanes, 8 positions each)
KS = [(1001, 31), (1007, 31), (1061, 31)]
BASE_LEN = 20000


def tile_of(K, S):
    return 1024 if K - S < 1024 else 2048


def takes_fast_path(K, S):
    """scan_syncmer_fast.hpp: syncmer_fast_ring"""
    d = (K - S) // 8 - 1
    return 64 <= d < 128 and K + 2048 + 8 + 64 <= 4096


def lengths(K, S):
    """K - 1, K, K + 1, then every wave boundary behind K up to three tiles (and one wave more): one below, on it, one above; all residues mod 8 behind the
    first boundary where a wave lies wholly behind the end"""
    out = [K - 1, K, K + 1, 1023, 1024, 1025, 1535, 1536, 1537]
    out += list(range(1537, 1545))
    for b in (2048, 2560, 3072):
        out += [b - 1, b, b + 1]
    if tile_of(K, S) == 2048:
        for b in (3584, 4096):
            out += [b - 1, b, b + 1]
    return sorted(set(out))


def no_repeat_dna(rng, n):
    """n bases, no two neighbours equal"""
    a = (int(rng.integers(0, 4)) + np.r_[0, np.cumsum(rng.integers(1, 4, n - 1))]) % 4
    return bytes(np.frombuffer(b"ACGT", np.uint8)[a])


def build(K, S):
    rng = np.random.default_rng(K * 100 + S)
    base = no_repeat_dna(rng, BASE_LEN)
    scm = np.sort(O.scan([base], K, S, mode=0)["m_pos"].astype(np.int64) >> 1)        # k-mer starts of the base sequence's closed syncmers
    assert len(scm) >= 8
    reads, kind = [], []
    for i, L in enumerate(lengths(K, S)):
        reads.append(base[137 * i:137 * i + L]), kind.append(("random", L))
        if L < K:
            continue
        first = scm[scm + L <= BASE_LEN]
        last = scm[scm + K >= L]
        p, q = int(first[i % len(first)]), int(last[i % len(last)])
        reads.append(base[p:p + L]), kind.append(("first", L))
        reads.append(base[q + K - L:q + K]), kind.append(("last", L))
    for unit in (b"AC", b"ACGTAGC"):                        # tandem repeats: every position ties; in an end wave, and beside a wave behind the end
        for L in (1536, 1537, 2049):
            reads.append((unit * (L // len(unit) + 1))[:L]), kind.append(("tandem", L))
    reads.append(no_repeat_dna(rng, S - 3)), kind.append(("short", S - 3))
    with_n = bytearray(no_repeat_dna(rng, 2000))
    with_n[1990] = ord("N")                                 # an N in the last wave: the general kernel, which nothing here changes
    reads.append(bytes(with_n)), kind.append(("n", 2000))
    return reads, kind


_cache = {}


def case(K, S):
    if (K, S) not in _cache:
        reads, kind = build(K, S)
        _cache[(K, S)] = (reads, kind, O.scan(reads, K, S, mode=0))
    return _cache[(K, S)]


@pytest.mark.parametrize("K,S", KS)
def test_premises(K, S):
    """the inputs are what the docstring says, read from the oracle's output: hoco lengths, and a syncmer at the first and at the last k-mer in a read whose
    last wave is partial, in one with a wave wholly behind the end, and in one whose length is a multiple of the tile"""
    assert takes_fast_path(K, S) and (-(K - S)) % 8 == {1001: 6, 1007: 0, 1061: 2}[K]
    reads, kind, want = case(K, S)
    T = tile_of(K, S)
    hl, n_scm = want["hoco_l"].astype(np.int64), want["n_scm"].astype(np.int64)
    off = np.r_[0, np.cumsum(n_scm)]
    seen = set()
    for r, (what, L) in enumerate(kind):
        if what != "n":
            assert hl[r] == len(reads[r]) == L, (r, what, L)
        if what not in ("first", "last"):
            continue
        pos = want["m_pos"][off[r]:off[r + 1]].astype(np.int64) >> 1
        assert (0 if what == "first" else L - K) in pos, (what, L)
        rest = L % T
        if L % WAVE:
            seen.add((what, "partial last wave"))
        if rest and rest <= T - WAVE:
            seen.add((what, "a wave behind the end"))
        if rest == 0:
            seen.add((what, "multiple of the tile"))
    for what in ("first", "last"):
        for where in ("partial last wave", "a wave behind the end", "multiple of the tile"):
            assert (what, where) in seen, (what, where)
    # the tandem reads tie everywhere and still carry syncmers or none -- either way the oracle decides; the short read has no s-mer
    assert n_scm[[k[0] for k in kind].index("short")] == 0
    # the four-wave form sees one, two and three waves behind the end
    if T == 2048:
        behind = {(T - L % T) // WAVE for _, L in kind if L % T}
        assert {1, 2, 3} <= behind


@pytest.mark.gpu
@pytest.mark.parametrize("K,S", KS)
def test_read_ends(hip, K, S):
    import test_gpu_scan as G
    reads, kind, want = case(K, S)
    got, _ = G.run_hip(hip, reads, K, S)
    G.compare_scan(got, want)
    assert int(want["n_scm"].sum()) > 0
