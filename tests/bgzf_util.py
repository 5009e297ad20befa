"""BGZF members made by hand for the inflater's tests (tests/test_host_inflate_core_fuzz.py on the CPU, tests/test_gpu_inflate.py on the device): members of every
shape from raw deflate streams of Python's zlib, and streams zlib never writes, bit by bit -- a first token that is a match, a distance one beyond the produced
bytes, over-subscribed code lengths, block type 3, LEN != ~NLEN, and code-length repeat codes that run from the literal/length lengths into the distance lengths."""
import bisect
import struct
import zlib

import numpy as np


def raw_deflate(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=()):
    """a raw deflate stream; flush_at: (position, flush mode) pairs that end a block inside the member"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, at = b"", 0
    for pos, mode in flush_at:
        out += c.compress(text[at:pos]) + c.flush(mode)
        at = pos
    return out + c.compress(text[at:]) + c.flush()


def member(stream, text=None, crc=None, isize=None):
    """a BGZF member around a raw deflate stream: bgzip's 18-byte header (BC field), the stream, CRC-32 and ISIZE"""
    if crc is None:
        crc = zlib.crc32(text)
    if isize is None:
        isize = len(text)
    bsize = 18 + len(stream) + 8
    assert bsize <= 65536, "not a BGZF member: %d bytes" % bsize
    return b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize - 1) + stream + struct.pack("<II", crc & 0xFFFFFFFF, isize)


EOF_MARKER = member(b"\x03\x00", b"")
assert len(EOF_MARKER) == 28


def stored(text):
    return raw_deflate(text, 0)


class Bits:
    """a deflate stream bit by bit: values LSB first, Huffman codes MSB first (RFC 1951 3.1.1)"""

    def __init__(self):
        self.v, self.n, self.parts = 0, 0, []

    def put(self, value, nbits):
        self.v |= value << self.n
        self.n += nbits
        return self.spill() if self.n >= 4096 else self

    def spill(self):
        """whole bytes leave the integer, so that a long stream costs what it holds and not its square"""
        k = self.n >> 3
        self.parts.append((self.v & ((1 << (k << 3)) - 1)).to_bytes(k, "little"))
        self.v >>= k << 3
        self.n &= 7
        return self

    def code(self, code, nbits):
        for i in range(nbits - 1, -1, -1):
            self.put((code >> i) & 1, 1)
        return self

    def align(self):
        self.n = (self.n + 7) // 8 * 8
        return self

    def bytes(self):
        return b"".join(self.parts) + self.v.to_bytes((self.n + 7) // 8, "little")


def canonical(lens):
    """{symbol: (code, length)} of the canonical Huffman code with these lengths (RFC 1951 3.2.2)"""
    out, code = {}, 0
    for ln in range(1, 16):
        for s in sorted(k for k, v in lens.items() if v == ln):
            out[s] = (code, ln)
            code += 1
        code <<= 1
    return out


def _fixed_lit(b, sym):
    if sym < 144:
        return b.code(0x30 + sym, 8)
    if sym < 256:
        return b.code(0x190 + sym - 144, 9)
    if sym < 280:
        return b.code(sym - 256, 7)
    return b.code(0xC0 + sym - 280, 8)


def _msb_first(code, nbits):
    return int(format(code, "0%db" % nbits)[::-1], 2)


def _fixed_tables():
    """what a fixed-Huffman block writes for a literal, a length and a distance, each as (bits LSB first, how many): RFC 1951 3.2.5 and 3.2.6"""
    sym = []
    for s in range(288):
        code, n = (0x30 + s, 8) if s < 144 else (0x190 + s - 144, 9) if s < 256 else (s - 256, 7) if s < 280 else (0xC0 + s - 280, 8)
        sym.append((_msb_first(code, n), n))
    length = {}
    for c in range(257, 285):                                   # eight codes without extra bits, then four codes for each number of extra bits from 1 to 5
        e = 0 if c < 265 else (c - 261) >> 2
        base = c - 254 if c < 265 else 3 + ((4 + ((c - 261) & 3)) << e)
        for x in range(1 << e):
            v, n = sym[c]
            length[base + x] = (v | x << n, n + e)
    length[258] = sym[285]                                      # (code 284 with extra 31 would say 258 too; deflate writes 285)
    assert sorted(length) == list(range(3, 259))
    dist = []                                                   # per distance code: (first distance, code bits LSB first, extra bits)
    for c in range(30):
        e = 0 if c < 4 else (c >> 1) - 1
        dist.append((c + 1 if c < 4 else 1 + ((2 + (c & 1)) << e), _msb_first(c, 5), e))
    return sym, length, dist


_FIXED_SYM, _FIXED_LEN, _FIXED_DIST = _fixed_tables()
_FIXED_DIST_FIRST = [f for f, _, _ in _FIXED_DIST]


def fixed_block(bits, tokens, final):
    """a fixed-Huffman block appended to `bits`; tokens: an int is a literal, (length, distance) a match (3..258, 1..32768)"""
    bits.put(1 if final else 0, 1).put(1, 2)
    for t in tokens:
        if isinstance(t, tuple):
            ln, d = t
            assert 3 <= ln <= 258 and 1 <= d <= 32768, t
            bits.put(*_FIXED_LEN[ln])
            first, code, e = _FIXED_DIST[bisect.bisect_right(_FIXED_DIST_FIRST, d) - 1]
            bits.put(code | (d - first) << 5, 5 + e)
        else:
            bits.put(*_FIXED_SYM[t])
    bits.put(*_FIXED_SYM[256])
    return bits


def stored_block(bits, data, final):
    """a stored block appended to `bits`: the header, zeros up to the byte boundary, LEN, ~LEN, the bytes"""
    assert len(data) <= 65535
    bits.put(1 if final else 0, 1).put(0, 2).align().put(len(data), 16).put(~len(data) & 0xFFFF, 16).spill()
    assert bits.n == 0
    bits.parts.append(bytes(data))
    return bits


def write_blocks(blocks):
    """[("fixed", tokens) | ("stored", bytes)] -> (raw deflate stream, the bit offset 0..7 at which each block's header starts); the last block is the final one"""
    b, at = Bits(), []
    for i, (kind, body) in enumerate(blocks):
        at.append(b.n & 7)
        (fixed_block if kind == "fixed" else stored_block)(b, body, i == len(blocks) - 1)
    return b.bytes(), at


def walk_blocks(blocks):
    """the tokens as the decoder hands them out, one (index, kind, output offset, length, distance) each: kind "lit", "match" or "stored"; index counts tokens, so
    index % 64 is a token's place in the kernel's batch (an empty stored block is no token)"""
    i = o = 0
    for kind, body in blocks:
        if kind == "stored":
            if len(body):
                yield i, "stored", o, len(body), 0
                i, o = i + 1, o + len(body)
            continue
        for t in body:
            ln, d = t if isinstance(t, tuple) else (1, 0)
            yield i, "match" if d else "lit", o, ln, d
            i, o = i + 1, o + ln


def lz_model(blocks):
    """the text of a block list, by the definition of LZ77: one byte at a time, a match reading what was written a moment ago"""
    out = bytearray()
    for kind, body in blocks:
        if kind == "stored":
            for x in body:
                out.append(x)
            continue
        for t in body:
            if isinstance(t, tuple):
                ln, d = t
                assert d <= len(out), (t, len(out))
                for _ in range(ln):
                    out.append(out[-d])
            else:
                out.append(t)
    return bytes(out)


def first_token_is_a_match():
    """a fixed block whose first token is (length 3, distance 1): there is nothing to copy from"""
    b = Bits().put(1, 1).put(1, 2)
    _fixed_lit(b, 257).code(0, 5)
    return _fixed_lit(b, 256).bytes()


def distance_one_beyond():
    """literals 'A' 'B', then (length 3, distance 3): one before the member's first byte"""
    b = Bits().put(1, 1).put(1, 2)
    _fixed_lit(_fixed_lit(b, 65), 66)
    _fixed_lit(b, 257).code(2, 5)
    return _fixed_lit(b, 256).bytes()


def oversubscribed():
    """a dynamic block whose nineteen code-length codes all have length 1"""
    b = Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(15, 4)
    for _ in range(19):
        b.put(1, 3)
    return b.put(0, 32).bytes()


def block_type_3():
    return Bits().put(1, 1).put(3, 2).put(0, 13).bytes()


def stored_len_mismatch(text=b"hello"):
    return Bits().put(1, 1).put(0, 2).align().put(len(text), 16).put((~len(text) & 0xFFFF) ^ 0x0100, 16).bytes() + text


def repeat_across_the_boundary():
    """(stream, text): a dynamic block whose code lengths end ... [256] = 3, then repeat code 16 six times over [257] and the first five DISTANCE lengths, then
    three times more -- zlib's deflate never writes this (it sends the two sets of lengths separately); other compressors do.  zlib's inflate reads it."""
    ll = {65: 2, 67: 2, 71: 3, 84: 3, 256: 3, 257: 3}
    dd = {i: 3 for i in range(8)}
    cl = {0: 3, 2: 3, 3: 2, 16: 3, 17: 3, 18: 2}
    clc, llc, ddc = canonical(cl), canonical(ll), canonical(dd)
    b = Bits().put(1, 1).put(2, 2).put(258 - 257, 5).put(8 - 1, 5).put(16 - 4, 4)
    for s in [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2]:
        b.put(cl.get(s, 0), 3)

    def sym(s, extra=None):
        b.code(*clc[s])
        if extra:
            b.put(*extra)
    sym(18, (65 - 11, 7)); sym(2); sym(0); sym(2); sym(17, (0, 3)); sym(3); sym(18, (12 - 11, 7)); sym(3)         # noqa: E702
    sym(18, (138 - 11, 7)); sym(18, (33 - 11, 7)); sym(3)                                                        # noqa: E702  ... [256]
    sym(16, (6 - 3, 2)); sym(16, (3 - 3, 2))                                                                     # noqa: E702  [257] and distance lengths 0..4; 5..7
    for ch in b"ACGTTGCA":
        b.code(*llc[ch])
    b.code(*llc[257]).code(*ddc[3])            # length 3, distance 4: "TGC"
    b.code(*llc[257]).code(*ddc[0])            # length 3, distance 1: "CCC"
    b.code(*llc[256])
    stream = b.bytes()
    text = zlib.decompressobj(-15).decompress(stream)
    assert text == b"ACGTTGCATGCCCC", text
    return stream, text


def table(members_and_texts):
    """a file of members laid end to end -> (bytes, record array in the layout of oatk_bgzf_member_t): what oatk_bgzf_index makes of it, computed here"""
    from oatk_amd import _lib
    data, rows, out = b"", [], 0
    for m in members_and_texts:
        isize = struct.unpack("<I", m[-4:])[0]
        rows.append((len(data) + 18, len(m) - 26, isize, out, struct.unpack("<I", m[-8:-4])[0], 0))
        data += m
        out += isize
    return data, np.array(rows, dtype=_lib.BGZF_MEMBER)
