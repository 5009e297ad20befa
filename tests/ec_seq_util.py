"""Helpers for the corrected-sequence tests (tests/test_gpu_ec_seq.py, tests/ec_seq_time.py): the COMPILED REFERENCE's read_error_correction
(syncerr.c:819) with its FILE *fo, called directly through ctypes with one thread -- it then writes the reads in order -- and the inputs the tests share."""
import ctypes as C
import os

import numpy as np

import adversarial as A
import ref_lib as R

_libc = None


def libc():
    global _libc
    if _libc is None:
        L = C.CDLL(None)
        L.fopen.restype = C.c_void_p
        L.fopen.argtypes = [C.c_char_p, C.c_char_p]
        L.fclose.argtypes = [C.c_void_p]
        L.strdup.restype = C.c_void_p
        L.strdup.argtypes = [C.c_char_p]
        _libc = L
    return _libc


def reference_ec_fo(db, g, max_edist, c, a, path):
    """read_error_correction(db, g, max_edist, c, 10 c, c, a, 1 thread, fo = path, quiet) of liboatk_ref.so; the file's bytes"""
    L = R.lib()
    L.read_error_correction.restype = None
    L.read_error_correction.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_int, C.c_void_p, C.c_int]
    fo = libc().fopen(str(path).encode(), b"w")
    assert fo
    try:
        L.read_error_correction(db, g, max_edist, c, 10 * c, c, a, 1, fo, 0)
    finally:
        libc().fclose(fo)
    with open(path, "rb") as f:
        return f.read()


def parse_fo(text):
    """[(name, sequence)] of a file of '>name\\nSEQ\\n' records (an empty sequence is an empty line)"""
    lines = text.split(b"\n")
    assert lines[-1] == b"" and len(lines) % 2 == 1
    out = []
    for i in range(0, len(lines) - 1, 2):
        assert lines[i][:1] == b">"
        out.append((lines[i][1:], lines[i + 1]))
    return out


def hoco_strings(flat):
    """the reads' hoco strings over ACGT from SrDb.flatten(): hoco_s packs four bases to a byte, first base in the top bits, every read from a fresh byte"""
    nt = np.frombuffer(b"ACGT", np.uint8)
    out, at = [], 0
    for l in flat["hoco_l"]:
        l = int(l)
        b = flat["hoco_s"][at:at + (l + 3) // 4]
        codes = np.stack([(b >> s) & 3 for s in (6, 4, 2, 0)], axis=1).reshape(-1)[:l]
        out.append(nt[codes].tobytes())
        at += (l + 3) // 4
    return out


# ---- long blocks that the search CORRECTS (tests/test_gpu_ec_routes.py's long blocks all fail: their inserts are unique to their reads) ----
LONG_K, LONG_S, LONG_C = 1001, 31, 3
LONG_LENGTHS = [1400, 1600, 2600, 2800, 3000, 3200, 5400, 5600, 6200, 6400, 11000, 11200, 12600, 12800, 22200, 22400, 38200, 38400]


def long_corrected_reads():
    """60 clean reads tiling a homopolymer-free genome at 6 x, and per planned length l one read genome[s0 : s0 + 2500 + l + 2500] with a substitution (that
    makes no homopolymer) every 600 bases from offset 2800 on through the middle stretch -- every k-mer that touches the stretch is seen once, so the read has one
    closed block of about l bases whose search walks the clean reads' chain and restores the genome; odd ones are reverse-complemented.  Returns (reads, the 18
    genome slices in the reads' orientation): the long reads are reads[60:]."""
    from test_gpu_ec_routes import nohp_base, tiled
    rng = np.random.default_rng(20261017)
    h = A.rand_nohp(rng, 60000)
    reads = tiled(h, 60, 6000, 0, 3)
    truth = []
    for j, l in enumerate(LONG_LENGTHS):
        s0 = (j * 3001) % (60000 - l - 5001)
        t = h[s0:s0 + 2500 + l + 2500]
        r = bytearray(t)
        for p in range(2800, 2500 + l, 600):
            r[p] = nohp_base(rng, {r[p], r[p - 1], r[p + 1]})
        r = bytes(r)
        if j & 1:
            r, t = A.revcomp(r), A.revcomp(t)
        reads.append(r)
        truth.append(t)
    return reads, truth
