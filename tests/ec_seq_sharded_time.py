#!/usr/bin/env python3
"""What the corrected reads' sequences cost with the reads spread over several handles (include/oatk_multi.h: oatk_multi_read_error_correction_fo; DESIGN.md
8.4), for the record: config-2-sized reads (oatk_amd.synth CONFIGS) from a FASTA file, one handle (oatk_read_error_correction_fo) and then two handles on ONE
GPU (the in-process communicator group), the adaptor with fo = /dev/null against fo = NULL, the median of 3, every sample on a state of its own (files read,
table collected).  Two handles on one GPU share the card: no speed-up is to be expected from them; the figure of several GPUs is not measured here.
Development aid.
usage: python tests/ec_seq_sharded_time.py [n_reads]"""
import ctypes as C
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oatk_amd import HipSyncasm, _lib  # noqa: E402
from oatk_amd.synth import CONFIGS, ReadSet  # noqa: E402

vp = C.c_void_p
K, S = 1001, 31
H = _lib.load_host()
H.oatk_sr_read_files.argtypes = [vp, vp, C.POINTER(C.c_char_p), C.c_int]
H.oatk_collect_syncmer_from_reads.restype = vp
H.oatk_collect_syncmer_from_reads.argtypes = [vp, vp, C.POINTER(C.c_int)]
_args = [vp, vp, vp, vp, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double]
H.oatk_read_error_correction.argtypes = _args + [vp]
H.oatk_read_error_correction_fo.argtypes = _args + [vp, vp]
H.oatk_sr_db_clean.argtypes = [vp]
H.oatk_syncmer_db_destroy.argtypes = [vp]
libc = C.CDLL(None)
libc.fopen.restype = vp
libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
libc.fclose.argtypes = [vp]


def sample(files, c, n_handles, with_fo):
    """one state of its own: the files read, the table collected; the adaptor timed"""
    st = np.zeros(12, np.uint64)
    fo = libc.fopen(b"/dev/null", b"w") if with_fo else None
    rc = C.c_int(0)
    db = H.oatk_sr_db_new(K, S)
    if n_handles == 1:
        hip = HipSyncasm(0)
        assert H.oatk_sr_read_files(hip.h, db, files, 1) == 0, hip.L.oatk_hip_last_error(hip.h)
        scm = H.oatk_collect_syncmer_from_reads(hip.h, db, C.byref(rc))
        assert scm and rc.value == 0
        t0 = time.perf_counter()
        r = H.oatk_read_error_correction_fo(hip.h, db, scm, None, 0.02, c, 10 * c, c, 0.35, fo, st.ctypes.data)
        dt = time.perf_counter() - t0
        assert r == 0, hip.L.oatk_hip_last_error(hip.h)
        hip.close()
    else:
        m = H.oatk_multi_create((C.c_int * n_handles)(*([0] * n_handles)), n_handles)
        assert m
        assert H.oatk_multi_sr_read_files(m, db, files, 1) == 0, H.oatk_multi_last_error(m)
        scm = H.oatk_multi_collect_syncmer_from_reads(m, db, C.byref(rc))
        assert scm and rc.value == 0, H.oatk_multi_last_error(m)
        t0 = time.perf_counter()
        r = H.oatk_multi_read_error_correction_fo(m, db, scm, 0.02, c, 10 * c, c, 0.35, fo, st.ctypes.data)
        dt = time.perf_counter() - t0
        assert r == 0, H.oatk_multi_last_error(m)
        H.oatk_multi_destroy(m)
    if fo:
        libc.fclose(fo)
    H.oatk_syncmer_db_destroy(scm)
    H.oatk_sr_db_clean(db)
    return dt, int(st[0] + st[5] + st[10])


def run(n):
    cfg = CONFIGS["config2"]
    c = cfg["min_k_cov"]
    rs = ReadSet(cfg["genome_len"], n, cfg["mean_len"])
    tmp = tempfile.mkdtemp()
    fa = os.path.join(tmp, "reads.fa")
    bases = 0
    with open(fa, "wb") as f:
        step = 20000
        for first in range(0, n, step):
            cnt = min(step, n - first)
            seq, off, lens = rs.slice(first, cnt, threads=16)
            bases += int(lens.sum())
            for i in range(cnt):
                f.write(b">r%d\n" % (first + i) + seq[int(off[i]):int(off[i]) + int(lens[i])].tobytes() + b"\n")
    print("%d reads, %.2f Gbases (config-2 shape), k %d, c %d" % (n, bases / 1e9, K, c), flush=True)
    files = (C.c_char_p * 1)(fa.encode())
    try:
        sample(files, c, 1, False)                             # warm-up: the libraries, the page cache
        for n_handles in (1, 2):
            med = {}
            for with_fo in (False, True):
                ts = []
                for _ in range(3):
                    dt, blocks = sample(files, c, n_handles, with_fo)
                    ts.append(dt)
                med[with_fo] = statistics.median(ts)
                print("  %d handle%s, fo = %-9s %7.3f s  (%s; %d error blocks)" % (n_handles, " " if n_handles == 1 else "s", "/dev/null" if with_fo else "NULL", med[with_fo],
                                                                                  ", ".join("%.3f" % t for t in ts), blocks), flush=True)
            print("  %d handle%s: the sequences add %.3f s" % (n_handles, " " if n_handles == 1 else "s", med[True] - med[False]), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print("  (two handles on one GPU share the card: no speed-up is expected; several GPUs: not measured)", flush=True)


if __name__ == "__main__":
    run(int(sys.argv[1]) if len(sys.argv) > 1 else CONFIGS["config2"]["n_reads"])
