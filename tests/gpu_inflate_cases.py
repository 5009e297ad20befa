"""The members tests/test_gpu_inflate.py inflates on the device, made without one (tests/test_host_inflate_core_fuzz.py puts the same ones to the decoder core on
the CPU first): member shapes as (name, raw deflate stream, text), and the fixed list of damaged members with the status each must get."""
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
    head, parts = b, []
    # (the body in pieces: one long integer per 1024 tokens keeps the bit writer linear)
    body = B.Bits()
    body.v, body.n = head.v, head.n
    for i, ch in enumerate(first):
        body.code(*llc[ch])
        if body.n >= 8192 and body.n % 8 == 0:
            parts.append(body.bytes())
            body = B.Bits()
    for _ in range(127):                                        # 127 x 258 = 32766 bytes, each copy from 32768 back
        body.code(*llc[285]).code(0, 1).put(32768 - 24577, 13)
    body.code(*llc[first[32766]]).code(*llc[first[32767]]).code(*llc[256])
    parts.append(body.bytes())
    stream, text = b"".join(parts), first + first
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
