"""CPU: what the case lists of tests/gpu_inflate_cases.py are FOR, read off their token lists (no kernel, no decoder): the device sweeps of
tests/test_gpu_inflate_sweeps.py cover the wave-wide executor of csrc/inflate.hpp only as far as these members make it do the things below, so a list that is
thinned one day fails here instead of quietly covering less.  (That zlib and the byte-by-byte model agree on every text, and that every member fits a BGZF
member, is asserted where the lists are built.)"""
import gpu_inflate_cases as G
from bgzf_util import walk_blocks


def tokens_of(entries):
    for name, _, _ in entries:
        for tok in walk_blocks(G.BLOCKS[name]):
            yield (name,) + tok


def test_the_lists_are_whole():
    assert [n for n, _, _ in G.copy_sweep()] == ["copy_d%d" % d for d in list(range(1, 521)) + [1023, 1024, 1025, 4096, 16384, 32767, 32768]]
    assert [n for n, _, _ in G.batch_edges()] == ["edge_k%d" % k for k in list(range(60, 69)) + list(range(124, 133))] + ["literals_%d" % n for n in (63, 64, 65, 127, 128, 129)]
    names = [n for n, _, _ in G.mixed_blocks()]
    assert names[:48] == ["mixed_b%d_L%d" % (b, L) for L in (0, 1, 63, 64, 65, 1000) for b in range(8)]
    assert names[49:] == ["stored_slot_%d" % i for i in range(64)] and len(G.mixed_blocks()[48][2]) == 65536      # the longest stored run: the text fills a member
    assert [len(t) for _, _, t in G.phase_grid()] == [0, 1, 2, 15, 16, 17, 31, 32, 33, 47]
    assert [len(t) for _, _, t in G.crc_lengths()] == [1, 1023, 1024, 1025, 2047, 2048, 2049, 32767, 32768, 32769, 64511, 64512, 64513, 65535, 65536]
    for f in G.SWEEP_LISTS:
        for name, s, t in f():
            assert len(s) + 26 <= 65536 and len(t) <= 65536, name


def test_every_distance_with_every_length():
    seen = {}
    for _, _, kind, _, ln, d in tokens_of(G.copy_sweep()):
        if kind == "match":
            seen.setdefault(d, []).append(ln)
    for d in range(1, 521):
        assert seen[d] == list(range(3, 259)), d                # rising, so every match copies what the ones before it wrote
    for d in (1023, 1024, 1025, 4096, 16384, 32767, 32768):
        top = seen[d][-1]
        assert seen[d] == list(range(3, top + 1)) and top >= 255, d
        assert top == 258 or d + sum(seen[d]) + top + 1 > 65536, d           # cut only where the next length would not fit
    for d in range(1, 258):                                     # overlapped: the source period is shorter than the copy
        assert any(ln > d for ln in seen[d]), d
    assert any(ln > d for d in range(64, 258) for ln in seen[d])             # the first pass of the wave reads from[j], later passes wrap


def test_members_of_the_sweep_have_the_text_they_are_said_to():
    for (name, _, text), d in zip(G.copy_sweep(), G.SWEEP_DISTANCES):
        assert len(text) == d + sum(G.sweep_lengths(d)) and text == (text[:d] * (len(text) // d + 1))[:len(text)], name      # period d throughout


def test_every_place_of_the_batch_holds_a_match_and_a_stored_run():
    every = [t for f in (G.copy_sweep, G.batch_edges, G.mixed_blocks, G.phase_grid) for t in tokens_of(f())]
    assert {i % 64 for _, i, kind, _, _, _ in every if kind == "match"} == set(range(64))
    assert {i % 64 for _, i, kind, _, ln, d in every if kind == "match" and d < ln} == set(range(64))
    assert {i % 64 for _, i, kind, _, _, _ in every if kind == "stored"} == set(range(64))
    # around the batch's end: the first match of edge_k<k> is token k, overlapped exactly when k < 70
    for k in list(range(60, 69)) + list(range(124, 133)):
        toks = G.BLOCKS["edge_k%d" % k][0][1]
        assert len(set(toks[:k])) == k and all(isinstance(t, int) for t in toks[:k])
        assert toks[k:k + 4] == [(70, k), toks[k + 1], (258, 1), (3, k + 329)] and isinstance(toks[k + 1], int) and isinstance(toks[k + 4], int) and len(toks) == k + 5


def test_stored_headers_at_every_bit_and_matches_that_read_stored_runs():
    for L in (0, 1, 63, 64, 65, 1000):
        bits = set()
        for b in range(8):
            name = "mixed_b%d_L%d" % (b, L)
            blocks = G.BLOCKS[name]
            assert [k for k, _ in blocks] == ["fixed", "stored", "fixed", "stored"] and len(blocks[1][1]) == L and len(blocks[3][1]) == 5
            assert sum(t >= 144 for t in blocks[0][1]) == b and sum(t < 144 for t in blocks[0][1]) == 40
            bits.add(G.HEADER_BIT[name][1])
            lo, hi = b + 40, b + 40 + L                         # the stored run is text[lo:hi]
            m = [(o - d, o - d + min(ln, d), ln, d, o) for _, _, kind, o, ln, d in tokens_of([(name, 0, 0)]) if kind == "match"]
            assert any(lo <= s and e <= hi for s, e, ln, d, o in m) == (L >= 3), name                          # wholly inside the run
            assert any(s < lo and (e > lo or L == 0) and d >= ln for s, e, ln, d, o in m), name               # from the first block into the run
            assert any((lo <= s < hi or L == 0) and d < ln for s, e, ln, d, o in m), name                     # overlapped, the source starts inside the run
            assert any(d == o for s, e, ln, d, o in m), name                                                 # from the member's first byte
        assert bits == set(range(8)), L
    name = G.mixed_blocks()[48][0]
    run = len(G.BLOCKS[name][1][1])
    m = [(o - d, ln, d) for _, _, kind, o, ln, d in tokens_of([(name, 0, 0)]) if kind == "match"]
    assert run > 65000 and any(43 <= s and s + ln <= 43 + run for s, ln, d in m) and any(d < ln and 43 <= s < 43 + run for s, ln, d in m) and any(d == 32768 for s, ln, d in m)
    for i in range(64):                                         # i literals, a stored run, a match out of the run
        blocks = G.BLOCKS["stored_slot_%d" % i]
        assert len(blocks[0][1]) == i and blocks[1][0] == "stored" and len(blocks[1][1]) == 7 + i and blocks[2][1][0] == (9, 5)


def test_phase_members_are_of_both_kinds():
    kinds = [[k for k, _ in G.BLOCKS[name]] for name, _, _ in G.phase_grid()]
    assert kinds == [["stored"], ["fixed"]] * 5
    for name, _, text in G.phase_grid():
        toks = G.BLOCKS[name][0][1]
        if name.startswith("phase_fixed") and len(text) >= 5:
            assert isinstance(toks[-1], tuple) and toks[-1][1] < toks[-1][0], name
