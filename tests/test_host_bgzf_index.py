"""CPU: oatk_bgzf_index (include/oatk_inflate.h, host/gzsrc.c) lists the members the host reader's BGZF path would take in one go -- the two share the code that reads
a member's header -- for files written by synth.write_fasta(mode=FA_BGZF) and for hand-made ones: bgzip's end marker in the middle, a text cap that cuts between
members, a member cap, a truncated last member, a plain gzip member following."""
import ctypes as C
import gzip
import struct
import zlib

import numpy as np

import adversarial as A
import bgzf_util as B
from oatk_amd import _lib, bgzf_index, pack_reads, synth


def walk(data, text_cap=1 << 62, member_cap=1 << 62):
    """the same table from the format's definition (SAM spec 4.1), written independently of the C code"""
    rows, p, out = [], 0, 0
    while len(rows) < member_cap and p + 18 <= len(data):
        if data[p:p + 4] != b"\x1f\x8b\x08\x04":
            break
        xlen = struct.unpack("<H", data[p + 10:p + 12])[0]
        q, bsize = p + 12, 0
        while q + 4 <= p + 12 + xlen:
            slen = struct.unpack("<H", data[q + 2:q + 4])[0]
            if data[q:q + 2] == b"BC" and slen == 2:
                bsize = struct.unpack("<H", data[q + 4:q + 6])[0] + 1
            q += 4 + slen
        hl = 12 + xlen
        if not bsize or p + bsize > len(data) or bsize < hl + 8:
            break
        crc, isize = struct.unpack("<II", data[p + bsize - 8:p + bsize])
        if isize > 65536 or out + isize > text_cap:
            break
        rows.append((p + hl, bsize - hl - 8, isize, out, crc, 0))
        p, out = p + bsize, out + isize
    return np.array(rows, dtype=_lib.BGZF_MEMBER), out, p


def same(data, **kw):
    m, t, c = bgzf_index(data, **{k: v for k, v in kw.items()})
    wm, wt, wc = walk(data, **kw)
    assert (t, c) == (wt, wc) and len(m) == len(wm)
    for f in ("in_off", "in_len", "out_len", "out_off", "crc"):
        assert np.array_equal(m[f], wm[f]), f
    return m, t, c


def members_of(texts):
    return [B.EOF_MARKER if t is None else B.member(B.raw_deflate(t, 6), t) for t in texts]


def test_written_fasta_and_the_host_reader_agree(tmp_path):
    reads = A.hifi_like(120, 20000, 3000, seed=3)
    seq, off, lens = pack_reads(reads)
    path = str(tmp_path / "r.fa.gz")
    synth.write_fasta(path, seq, off, lens, mode=synth.FA_BGZF)
    data = open(path, "rb").read()
    text = gzip.decompress(data)
    m, t, c = same(data)
    assert c == len(data) and t == len(text) and len(m) > 3
    for r in m[:3]:                                     # a row says where a raw deflate stream lies and what comes out of it
        s = data[int(r["in_off"]):int(r["in_off"]) + int(r["in_len"])]
        assert zlib.decompressobj(-15).decompress(s) == text[int(r["out_off"]):int(r["out_off"]) + int(r["out_len"])]
        assert zlib.crc32(text[int(r["out_off"]):int(r["out_off"]) + int(r["out_len"])]) == int(r["crc"])
    # the host reader (oatk_gzsrc_read -> bgzf_read) asked for the same room takes the same members: it has consumed comp_bytes when it returns the text
    H = _lib.load_host()
    H.oatk_gzsrc_open.restype = C.c_void_p
    H.oatk_gzsrc_open.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    H.oatk_gzsrc_read.restype = C.c_int64
    H.oatk_gzsrc_read.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    H.oatk_gzsrc_tell_in.restype = C.c_uint64
    H.oatk_gzsrc_tell_in.argtypes = [C.c_void_p]
    H.oatk_gzsrc_close.argtypes = [C.c_void_p]
    for k in (1, 2, len(m) // 2, len(m)):
        cap = int(m["out_off"][k - 1] + m["out_len"][k - 1])        # room for exactly k members
        mk, tk, ck = same(data, text_cap=cap)
        assert len(mk) == k and tk == cap
        rc = C.c_int()
        g = H.oatk_gzsrc_open(path.encode(), 4, C.byref(rc))
        assert g and rc.value == 0
        buf = np.zeros(cap, np.uint8)
        assert H.oatk_gzsrc_read(g, buf.ctypes.data, cap) == cap and buf.tobytes() == text[:cap]
        assert H.oatk_gzsrc_tell_in(g) == ck
        H.oatk_gzsrc_close(g)


def test_hand_made_files():
    t = [b"ACGT" * 1000, b"x", b"N" * 65536, b">r\nAC\n"]
    ms = members_of([t[0], t[1], None, t[2], t[3], None])          # the end marker in the middle and at the end
    data = b"".join(ms)
    m, tb, cb = same(data)
    assert len(m) == 6 and cb == len(data) and tb == sum(map(len, t)) and list(m["out_len"]) == [4000, 1, 0, 65536, 6, 0]
    # a text cap that cuts between members: whole members only
    for cap, n in ((0, 0), (3999, 0), (4000, 1), (4001, 3), (4001 + 65535, 3), (4001 + 65536, 4), (4001 + 65536 + 6, 6)):
        mm, tt, cc = same(data, text_cap=cap)
        assert len(mm) == n and cc == sum(len(x) for x in ms[:n]), cap
    # a member cap
    mm, tt, cc = same(data, member_cap=2)
    assert len(mm) == 2 and tt == 4001 and cc == len(ms[0]) + len(ms[1])
    # a truncated last member: the walk ends in front of it
    for cut in (1, 8, 20, len(ms[5]) - 1):
        mm, tt, cc = same(data[:-cut])
        assert len(mm) == 5 and cc == len(data) - len(ms[5])
    mm, tt, cc = same(data[:len(ms[0]) + 10])
    assert len(mm) == 1
    # a plain gzip member following: the BGZF members in front of it, no more
    plain = gzip.compress(b">q\nACGT\n")
    mm, tt, cc = same(ms[0] + ms[1] + plain + ms[3])
    assert len(mm) == 2 and cc == len(ms[0]) + len(ms[1])
    # not BGZF at all, and nothing
    assert same(plain)[2] == 0 and same(b"")[2] == 0 and same(b"\x1f\x8b")[2] == 0
