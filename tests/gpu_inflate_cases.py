"""The members tests/test_gpu_inflate.py and tests/test_gpu_inflate_sweeps.py inflate on the device, made without one (tests/test_host_inflate_core_fuzz.py puts
the same ones to the decoder core on the CPU first): member shapes as (name, raw deflate stream, text), the fixed list of damaged members with the status each must
get, and the lists of the sweeps -- written token by token (bgzf_util.fixed_block / stored_block), so that what a member makes the kernel do is known: which
distances its overlapped copies have, at which place of the 64-token batch a match or a stored run falls, at which bit a stored header starts.  Every text of those
is computed twice, by zlib's inflate from the stream and by a byte-by-byte LZ77 model from the tokens, and the two must agree (tests/test_inflate_case_lists.py
asserts what the lists are for)."""
import struct
import zlib

import numpy as np

import bgzf_util as B


def acgt(n, seed):
    return bytes(np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].tolist())


def fasta_like(n, seed):
    rng = np.random.default_rng(seed)
    g, t, i = acgt(9000, seed + 100), b"", 0
    while len(t) < n:
        p, ln = int(rng.integers(0, 6000)), int(rng.integers(200, 3000))
        t += b">read/%d/ccs len=%d\n" % (i, ln) + g[p:p + ln] + b"\n"
        i += 1
    return t[:n]


def distance_32768():
    """(stream, text): 32768 random bases as literals, then the same again as matches of distance 32768 -- the largest there is; zlib's deflate stops at 32506, so
    the block is written here: a dynamic block with its own small codes and a distance code of one symbol (a single 1-bit code, which zlib's inflate takes)"""
    first = acgt(32768, 77)
    ll = {65: 2, 67: 2, 71: 3, 84: 3, 256: 3, 285: 3}
    llc = B.canonical(ll)
    cl = {s: (4 if s < 13 else 5) for s in range(19)}           # a complete code over all nineteen symbols; every length is sent as itself
    clc = B.canonical(cl)
    b = B.Bits().put(1, 1).put(2, 2).put(286 - 257, 5).put(30 - 1, 5).put(19 - 4, 4)
    for s in [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]:
        b.put(cl[s], 3)
    for s in range(286):
        b.code(*clc[ll.get(s, 0)])
    for s in range(30):
        b.code(*clc[1 if s == 29 else 0])
    for ch in first:
        b.code(*llc[ch])
    for _ in range(127):                                        # 127 x 258 = 32766 bytes, each copy from 32768 back
        b.code(*llc[285]).code(0, 1).put(32768 - 24577, 13)
    b.code(*llc[first[32766]]).code(*llc[first[32767]]).code(*llc[256])
    stream, text = b.bytes(), first + first
    assert zlib.decompressobj(-15).decompress(stream) == text
    return stream, text


_shapes = None


def member_shapes():
    global _shapes
    if _shapes is not None:
        return _shapes
    S = []
    S.append(("eof_marker", b"\x03\x00", b""))
    S.append(("stored_1", B.stored(b"x"), b"x"))
    t = bytes(np.random.default_rng(3).integers(0, 256, 65280, dtype=np.uint8).tolist())
    S.append(("stored_65280", B.stored(t), t))
    t = fasta_like(65536, 4)
    S.append(("isize_65536", B.raw_deflate(t, 6), t))
    for name, t in (("fixed_A700", b"A" * 700), ("fixed_AC400", b"AC" * 400), ("fixed_ACG300", b"ACG" * 300)):
        S.append((name, B.raw_deflate(t, 6, zlib.Z_FIXED), t))
    S.append(("dynamic_distance_32768",) + distance_32768())
    t = fasta_like(40000, 5)
    S.append(("three_blocks", B.raw_deflate(t, 6, flush_at=[(13000, zlib.Z_FULL_FLUSH), (26001, zlib.Z_SYNC_FLUSH)]), t))
    t = fasta_like(30000, 6)
    S.append(("huffman_only", B.raw_deflate(t, 6, zlib.Z_HUFFMAN_ONLY), t))
    for lv in (1, 6, 9):
        t = acgt(30011, 10 + lv)
        S.append(("acgt_level%d" % lv, B.raw_deflate(t, lv), t))
    S.append(("repeat_across_the_boundary",) + B.repeat_across_the_boundary())
    for name, s, t in S:
        assert len(s) + 26 <= 65536 and len(t) <= 65536, name
    _shapes = S
    return S


GOOD = [acgt(5003, 21), fasta_like(20001, 22), acgt(777, 23)]


def good_member(i):
    return B.member(B.raw_deflate(GOOD[i], 6), GOOD[i])


def damage_cases():
    """(name, member bytes, edit of the member's table row or None, expected status).  One bad member each; the test puts good ones around it."""
    t = acgt(4001, 31)
    st = bytearray(B.stored(t))
    st[5 + 1234] ^= 0x10                                        # a bit of a stored byte: only the CRC can tell
    c = B.raw_deflate(fasta_like(30000, 32), 6)
    ct = fasta_like(30000, 32)
    crc = zlib.crc32(ct)

    def cut(n):
        def edit(row):
            row["in_len"] -= n(int(row["in_len"][0]))                # (row: a slice of one member of the table)
        return edit
    hand = lambda s, n: B.member(s, crc=0, isize=n)             # noqa: E731
    return [
        ("stored_bit_flipped", B.member(bytes(st), t), None, 3),
        ("crc_field_flipped", B.member(c, crc=crc ^ 0x00400000, isize=len(ct)), None, 3),
        ("isize_plus_1", B.member(c, crc=crc, isize=len(ct) + 1), None, 2),
        ("isize_minus_1", B.member(c, crc=crc, isize=len(ct) - 1), None, 2),
        ("in_len_cut_by_1", B.member(c, ct), cut(lambda n: 1), 1),
        ("in_len_cut_by_half", B.member(c, ct), cut(lambda n: n // 2), 1),
        ("first_token_is_a_match", hand(B.first_token_is_a_match(), 3), None, 1),
        ("distance_one_beyond", hand(B.distance_one_beyond(), 5), None, 1),
        ("oversubscribed_code_lengths", hand(B.oversubscribed(), 0), None, 1),
        ("block_type_3", hand(B.block_type_3(), 0), None, 1),
        ("stored_len_nlen_mismatch", hand(B.stored_len_mismatch(), 5), None, 1),
    ]


def isize_of(m):
    return struct.unpack("<I", m[-4:])[0]


# ---- the sweeps of tests/test_gpu_inflate_sweeps.py ----
BLOCKS = {}             # name -> the member's blocks, [("fixed", tokens) | ("stored", bytes)], for the entries written token by token
HEADER_BIT = {}         # name -> the bit offset 0..7 at which each of those blocks' headers starts
_lists = {}


def zlib_text(stream):
    z = zlib.decompressobj(-15)
    t = z.decompress(stream)
    assert z.eof and not z.unused_data and not z.unconsumed_tail
    return t


def _checked(name, stream, text):
    assert len(stream) + 26 <= 65536 and len(text) <= 65536, (name, len(stream), len(text))
    assert zlib_text(stream) == text, name
    return name, stream, text


def _entry(name, blocks):
    """(name, stream, text) of a block list: zlib's text of the stream written from it has to be the model's text of the tokens"""
    stream, at = B.write_blocks(blocks)
    BLOCKS[name], HEADER_BIT[name] = blocks, at
    return _checked(name, stream, B.lz_model(blocks))


def _cached(fn):
    def get():
        if fn.__name__ not in _lists:
            _lists[fn.__name__] = fn()
        return _lists[fn.__name__]
    get.__name__, get.__doc__ = fn.__name__, fn.__doc__
    return get


def _bytes(rng, n, lo=0, hi=256):
    return [int(x) for x in rng.integers(lo, hi, n)]


SWEEP_DISTANCES = list(range(1, 521)) + [1023, 1024, 1025, 4096, 16384, 32767, 32768]


def sweep_lengths(d):
    """the match lengths of copy_sweep's member of distance d: 3..258, cut from the top until d + their sum fits a member"""
    top = 258
    while d + (top * (top + 1) // 2 - 3) > 65536:
        top -= 1
    return range(3, top + 1)


@_cached
def copy_sweep():
    """one member per distance d: d random bytes as literals, then a match of every length at distance d in rising order, each copying what the ones before it wrote;
    d + 256 tokens, so the matches fall on every place of the 64-token batch as d varies"""
    out = []
    for d in SWEEP_DISTANCES:
        out.append(_entry("copy_d%d" % d, [("fixed", _bytes(np.random.default_rng(5000 + d), d) + [(ln, d) for ln in sweep_lengths(d)])]))
    return out


@_cached
def batch_edges():
    """k distinct literals, match (70, k) -- overlapped exactly when k < 70 --, a literal, match (258, 1), match (3, produced) that reaches the member's first byte,
    a literal: the first match sits at place k of the batch, for k around 64 and 128; and members of literals alone that end on, before and behind a full batch"""
    out = []
    for k in list(range(60, 69)) + list(range(124, 133)):
        rng = np.random.default_rng(6000 + k)
        lits = [int(x) for x in rng.permutation(256)[:k]]
        toks = lits + [(70, k), int(rng.integers(0, 256)), (258, 1), (3, k + 70 + 1 + 258), int(rng.integers(0, 256))]
        out.append(_entry("edge_k%d" % k, [("fixed", toks)]))
    for n in (63, 64, 65, 127, 128, 129):
        out.append(_entry("literals_%d" % n, [("fixed", _bytes(np.random.default_rng(6500 + n), n))]))
    return out


def _mixed(b, L, seed):
    """a fixed block of b 9-bit and 40 8-bit literals (so the stored header behind it starts at bit (3 + 9 b + 40 * 8 + 7) % 8 = (b + 2) % 8), a stored run of L
    bytes, a fixed block whose matches read the run, a final stored block of 5 bytes"""
    rng = np.random.default_rng(seed)
    first = _bytes(rng, b, 144, 256) + _bytes(rng, 40, 0, 144)
    run = bytes(_bytes(rng, L))
    p1 = b + 40                                                 # the run is text[p1 : p1 + L]
    toks, at = [], [p1 + L]

    def match(ln, d, overlapped):
        assert (d < ln) == overlapped and 1 <= d <= min(at[0], 32768)
        toks.append((ln, d))
        at[0] += ln
        toks.append(int(rng.integers(0, 256)))                  # a literal between the matches
        at[0] += 1
    if L >= 3:                                                  # wholly inside the run
        ln, d = min(L, 30), min(L, 32768)
        assert p1 <= at[0] - d and at[0] - d + ln <= p1 + L
        match(ln, d, False)
    if at[0] - (p1 - 5) <= 32768:                               # starts in the first block, ends in the run (as far as there is one)
        match(5 + min(L, 10), at[0] - (p1 - 5), False)
    src = p1 + L - min(L, b + 1) if L else p1 - 1               # overlapped, its source starting inside the run, among the run's last bytes: the distance stays
    match(200, at[0] - src, True)                               # below 64, so that the first 64 bytes of the copy already wrap
    assert toks[-2][1] < 64
    match(50, min(at[0], 32768), False)                         # from the member's first byte (or as far back as a distance reaches)
    return [("fixed", first), ("stored", run), ("fixed", toks), ("stored", bytes(_bytes(rng, 5)))]


@_cached
def mixed_blocks():
    """stored and Huffman blocks in one member: the stored header at every bit offset, at each run length; one member whose run is as long as a member allows
    (its text is 65536 bytes); and, so that a stored run falls on every place of the batch, i literals, a run, and a match that reads it, for i = 0..63"""
    out = []
    for L in (0, 1, 63, 64, 65, 1000):
        for b in range(8):
            out.append(_entry("mixed_b%d_L%d" % (b, L), _mixed(b, L, 7000 + 8 * L + b)))
    L = 65535
    while True:
        blocks = _mixed(3, L, 7999)
        over = max(len(B.write_blocks(blocks)[0]) + 26 - 65536, sum(ln for _, _, _, ln, _ in B.walk_blocks(blocks)) - 65536, 0)
        if not over:
            break
        L -= over
    out.append(_entry("mixed_b3_L%d" % L, blocks))
    for i in range(64):
        rng = np.random.default_rng(7100 + i)
        out.append(_entry("stored_slot_%d" % i, [("fixed", _bytes(rng, i)), ("stored", bytes(_bytes(rng, 7 + i))), ("fixed", [(9, 5), int(rng.integers(0, 256))])]))
    return out


PHASE_LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47)


@_cached
def phase_grid():
    """texts shorter than, as long as and longer than one, two and three 16-byte granules; a single stored block and fixed literals that end in an overlapped match
    (where the length allows one) take turns"""
    out = []
    for i, n in enumerate(PHASE_LENGTHS):
        rng = np.random.default_rng(8000 + n)
        if i % 2 == 0:
            out.append(_entry("phase_stored_%d" % n, [("stored", bytes(_bytes(rng, n)))]))
        else:
            k = n // 4 + 1
            out.append(_entry("phase_fixed_%d" % n, [("fixed", _bytes(rng, k) + [(n - k, k)] if n - k >= 3 else _bytes(rng, n))]))
    return out


CRC_LENGTHS = (1, 1023, 1024, 1025, 2047, 2048, 2049, 32767, 32768, 32769, 64511, 64512, 64513, 65535, 65536)


@_cached
def crc_lengths():
    """compressible text that ends on, before and behind the 1 KiB pieces the kernel takes the CRC in -- the first, the second, the middle and the last one"""
    out = []
    for i, n in enumerate(CRC_LENGTHS):
        t = (fasta_like, acgt)[i % 2](n, 9000 + i)
        out.append(_checked("crc_n%d" % n, B.raw_deflate(t, 1), t))
    return out


SWEEP_LISTS = (copy_sweep, batch_edges, mixed_blocks, phase_grid, crc_lengths)
