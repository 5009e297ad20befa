"""Unaligned BAM for the tests of oatk_hip_ingest_bam (tests/test_host_bam_core.py on the CPU, tests/test_gpu_bam.py on the device): a writer with struct, BGZF
framing over tests/bgzf_util.py, and a plain-Python reading of the same stream -- header walk, the predicates whole(o) / ok(o), the candidate list, the serial
chain walk and what it stops at -- which is the oracle for offsets, names and letters.  Written from the SAM/BAM specification as include/oatk_hip_ingest.h and
oatk_amd/csrc/bam_core.hpp restate it; no samtools, no pysam."""
import struct

import numpy as np

import bgzf_util as B

CODES = "=ACMGRSVTWYHKDBN"
CODE_OF = {c: i for i, c in enumerate(CODES)}
MIN_BLOCK, MAX_BLOCK = 32, 1 << 28
CLEAN, CUT, BAD = 0, 1, 2


def header(text=b"@HD\tVN:1.6\tSO:unknown\n", refs=()):
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, ln in refs:
        out += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", ln)
    return out


def pack_bases(seq):
    s = seq.upper()
    codes = [CODE_OF[chr(c)] for c in s] + ([0] if len(s) & 1 else [])
    return bytes(codes[i] << 4 | codes[i + 1] for i in range(0, len(codes), 2))


def record(name, seq, qual=None, tags=b"", flag=4, n_cigar=0):
    """one alignment record; name without its NUL; qual: bytes of len(seq), or None for 0xFF"""
    if qual is None:
        qual = b"\xff" * len(seq)
    assert len(qual) == len(seq) and len(name) + 1 <= 255
    body = struct.pack("<iiBBHHHIiii", -1, -1, len(name) + 1, 255, 4680, n_cigar, flag, len(seq), -1, -1, 0)
    body += name + b"\0" + b"".join(struct.pack("<I", (7 + i) << 4 | 4) for i in range(n_cigar)) + pack_bases(seq) + qual + tags
    return struct.pack("<i", len(body)) + body


def stream(reads, text=b"@HD\tVN:1.6\tSO:unknown\n", refs=()):
    """reads: dicts / tuples for record() -> the inflated BAM stream"""
    return header(text, refs) + b"".join(record(**r) if isinstance(r, dict) else record(*r) for r in reads)


def bgzf(data, member_text=65280, level=6):
    """the bytes of a .bam file: BGZF members of member_text bytes of content each, and the end marker"""
    out = b""
    for i in range(0, len(data), member_text):
        t = data[i:i + member_text]
        s = B.raw_deflate(t, level)
        if 18 + len(s) + 8 > 65536:
            s = B.stored(t)
        out += B.member(s, t)
    return out + B.EOF_MARKER


def tag_int(key, v):
    return key + b"i" + struct.pack("<i", v)


def tag_bytes(key, payload):
    """a B-type tag of unsigned bytes holding payload"""
    return key + b"BC" + struct.pack("<I", len(payload)) + payload


# ---- the oracle ----
def header_walk(b):
    """('ok', length) | ('more', bytes needed) | ('bad', 0) for the header in b"""
    have = len(b)
    if b[:4] != b"BAM\x01"[:min(4, have)]:
        return "bad", 0
    if have < 8:
        return "more", 8
    l_text = struct.unpack_from("<i", b, 4)[0]
    if l_text < 0:
        return "bad", 0
    p = 8 + l_text
    if have < p + 4:
        return "more", p + 4
    n_ref = struct.unpack_from("<i", b, p)[0]
    if n_ref < 0:
        return "bad", 0
    p += 4
    for _ in range(n_ref):
        if have < p + 4:
            return "more", p + 4
        l_name = struct.unpack_from("<i", b, p)[0]
        if l_name < 0:
            return "bad", 0
        p += 4 + l_name + 4
    if have < p:
        return "more", p
    return "ok", p


def whole(b, o):
    n = len(b)
    if o + 4 > n:
        return False
    bs = struct.unpack_from("<i", b, o)[0]
    return MIN_BLOCK <= bs <= MAX_BLOCK and o + 4 + bs <= n


def ok(b, o):
    if not whole(b, o):
        return False
    bs = struct.unpack_from("<i", b, o)[0]
    lrn, ncig, lseq = b[o + 12], struct.unpack_from("<H", b, o + 16)[0], struct.unpack_from("<I", b, o + 20)[0]
    if lrn < 1 or 32 + lrn + 4 * ncig + (lseq + 1) // 2 + lseq > bs:
        return False
    return b[o + 36 + lrn - 1] == 0


def candidates(b, s0):
    """every offset >= s0 with ok(o), by numpy for the block_size test and by ok() for what passes it"""
    a = np.frombuffer(b, np.uint8)
    n = len(a)
    if n < s0 + 36:
        return []
    w = a[:n - 3].astype(np.int64) | a[1:n - 2].astype(np.int64) << 8 | a[2:n - 1].astype(np.int64) << 16 | a[3:].astype(np.int64) << 24
    o = np.arange(n - 3, dtype=np.int64)
    pre = np.flatnonzero((w >= MIN_BLOCK) & (w <= MAX_BLOCK) & (o + 4 + w <= n) & (o >= s0))
    return [int(x) for x in pre if ok(b, int(x))]


def chain(b, s0):
    """the serial walk from s0: (record offsets, t, CLEAN | CUT | BAD)"""
    n, o, recs = len(b), s0, []
    while True:
        if o == n:
            return recs, o, CLEAN
        if o + 4 > n:
            return recs, o, CUT
        bs = struct.unpack_from("<i", b, o)[0]
        if not MIN_BLOCK <= bs <= MAX_BLOCK:
            return recs, o, BAD
        if o + 4 + bs > n:
            return recs, o, CUT
        if not ok(b, o):
            return recs, o, BAD
        recs.append(o)
        o += 4 + bs


def read_at(b, o):
    """(name, letters, flag) of the record at o"""
    lrn, ncig, flag, lseq = b[o + 12], struct.unpack_from("<H", b, o + 16)[0], struct.unpack_from("<H", b, o + 18)[0], struct.unpack_from("<I", b, o + 20)[0]
    raw = b[o + 36:o + 36 + lrn]
    name = raw[:raw.index(b"\0")]
    p = o + 36 + lrn + 4 * ncig
    packed = np.frombuffer(b, np.uint8, (lseq + 1) // 2, p)
    codes = np.empty(2 * len(packed), np.uint8)
    codes[0::2], codes[1::2] = packed >> 4, packed & 15
    return name, np.frombuffer(CODES.encode(), np.uint8)[codes[:lseq]].tobytes(), flag


def parse(b):
    """the whole stream: (names, reads, record offsets)"""
    v, s0 = header_walk(b)
    assert v == "ok"
    recs, t, why = chain(b, s0)
    assert why == CLEAN, (t, why)
    got = [read_at(b, o) for o in recs]
    return [g[0] for g in got], [g[1] for g in got], recs


def fasta(names, reads):
    return b"".join(b">" + n + b"\n" + r + b"\n" for n, r in zip(names, reads))


# ---- made streams ----
SWEEP_LENS = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2049]


def sweep_reads(tags, n_cigar, seed=3):
    """every length of SWEEP_LENS with every name length 1 .. 16 (the packed bases start at every offset modulo 16); the letters run through the sixteen codes with a
    stride that puts each at even and at odd positions, from a start that differs from read to read"""
    rng = np.random.default_rng(seed)
    out, k = [], 0
    for ln in SWEEP_LENS:
        for nl in range(1, 17):
            name = (b"r%d_" % k + b"x" * 16)[:nl]
            seq = "".join(CODES[(k + 7 * i + i // 16) & 15] for i in range(ln)).encode()
            tg = (tag_int(b"np", int(rng.integers(0, 40))) + b"rqf" + struct.pack("<f", 0.999) + b"zmZ" + b"m%d" % k + b"\0") if tags else b""
            out.append(dict(name=name, seq=seq, tags=tg, n_cigar=n_cigar))
            k += 1
    return out


def short_reads_with_int_tags(n, seed):
    """records of 50 .. 600 bases with integer tags: zero bytes in front of record starts make false candidates"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ln = int(rng.integers(50, 601))
        seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, ln)].tobytes()
        tg = tag_int(b"np", int(rng.integers(0, 200))) + tag_int(b"ec", int(rng.integers(0, 60))) + tag_int(b"zm", i)
        out.append(dict(name=b"m64011_%d/ccs" % i, seq=seq, qual=rng.integers(0, 94, ln, dtype=np.uint8).tobytes(), tags=tg))
    return out


def nested_fake_records():
    """reads whose tags hold complete records: two fake ones back to back in a B tag that ends with the enclosing record (their chain rejoins the true one), and a fake
    one in the first record's tag, in front of where the first record's successor starts"""
    fake1, fake2 = record(b"fakeA", b"TTTTGGGG"), record(b"fakeB", b"CCCCCAAAAAC")
    early = record(b"early", b"GATTACA")
    return [dict(name=b"first", seq=b"ACGTACGTAC", tags=tag_bytes(b"xe", early) + tag_int(b"np", 3)),
            dict(name=b"host", seq=b"ACGTNACGTN" * 7, tags=tag_int(b"np", 0) + tag_bytes(b"xf", fake1 + fake2)),
            dict(name=b"after", seq=b"GGGGCCCCAAAATTTTA"),
            dict(name=b"last", seq=b"", tags=tag_bytes(b"xg", fake2))]


def damage_cases():
    """{name: (stream, expected verdict)}: 'arg' or 'split' for the whole stream given as the final chunk"""
    good = [dict(name=b"a", seq=b"ACGTACGTACGTACGTAC"), dict(name=b"bb", seq=b"TTGCA" * 9, tags=tag_int(b"np", 9)), dict(name=b"ccc", seq=b"GGA")]
    h = header()
    r = [record(**x) for x in good]
    at = len(h) + len(r[0])                                       # the second record

    def patched(off, fmt, v):
        b = bytearray(h + b"".join(r))
        struct.pack_into(fmt, b, at + off, v)
        return bytes(b)
    cases = {
        "wrong magic": (b"BAM\x02" + (h + b"".join(r))[4:], "arg"),
        "negative l_text": (b"BAM\x01" + struct.pack("<i", -5) + (h + b"".join(r))[8:], "arg"),
        "block_size 31": (patched(0, "<i", 31), "arg"),
        "block_size -1": (patched(0, "<i", -1), "arg"),
        "block_size 2^28+1": (patched(0, "<i", (1 << 28) + 1), "arg"),
        "l_seq larger than the block": (patched(20, "<I", 100000), "arg"),
        "l_read_name 0": (patched(12, "<B", 0), "arg"),
        "name without NUL": (patched(36 + 2, "<B", ord("x")), "arg"),
        "final chunk cut mid-record": ((h + b"".join(r))[:-7], "arg"),
        "flag 0x10": (h + r[0] + record(flag=0x10, **good[1]) + r[2], "split"),
        "flag 0x100": (h + r[0] + record(flag=0x100, **good[1]) + r[2], "split"),
        "flag 0x800": (h + r[0] + r[1] + record(flag=0x800, **good[2]), "split"),
    }
    return cases

