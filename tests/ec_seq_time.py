#!/usr/bin/env python3
"""What the corrected reads' sequences cost (include/oatk_hip_ec.h: oatk_hip_ec_keep_seq, oatk_hip_ec_corrected_reads), at config 2 and config 3
(oatk_amd.synth CONFIGS), the median of 3 each:
  - the solve (the library's ec_solve timer) and the whole correction without and with the recording of q_end and the optimum consensus;
  - the length pass and the write kernel (HIP events, OATK_DEBUG_EC_STAGES), the latter held against bytes read + written / 6.3 TB/s;
  - oatk_read_error_correction_fo to /dev/null against oatk_read_error_correction: what building, fetching, expanding and writing the strings adds.
Development aid.
usage: python tests/ec_seq_time.py [config2|config3 ...] [--no-adaptor]"""
import ctypes as C
import os
import re
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
HBM_TBS = 6.3            # what the part sustains (MI355X_MICROARCH)


def med(ts):
    return statistics.median(ts), ", ".join("%.2f" % t for t in ts)


def stderr_of(fn):
    """fn()'s result and what the library wrote to stderr meanwhile"""
    fd, path = tempfile.mkstemp()
    saved = os.dup(2)
    os.dup2(fd, 2)
    try:
        r = fn()
    finally:
        os.dup2(saved, 2)
        os.close(fd)
        os.close(saved)
    txt = open(path).read()
    os.unlink(path)
    return r, txt


def run(name, adaptor):
    cfg = CONFIGS[name]
    n, c = cfg["n_reads"], cfg["min_k_cov"]
    rs = ReadSet(cfg["genome_len"], n, cfg["mean_len"])
    seq, off, lens = rs.slice(0, n, threads=16)
    print("%s: %d reads, %.2f Gbases" % (name, n, int(lens.sum()) / 1e9), flush=True)
    hip = HipSyncasm(0)
    hip.set_timing(True)
    hip.scan_host(seq, off, lens, K, S)
    hip.count()
    hip.ec_graph(light_c=c)
    hip.ec(0.02, c, 0.35)                                    # warm-up: buffers, streams
    for keep in (False, True):
        solve, wall = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            st = hip.ec(0.02, c, 0.35, keep_seq=keep)
            wall.append(1e3 * (time.perf_counter() - t0))
            solve.append(hip.timing()["ec_solve"])
        print("  correction %s recording: ec_solve %8.2f ms (%s), mark + solve + refresh wall %8.2f ms (%s)" % (("with   " if keep else "without"), *med(solve), *med(wall)), flush=True)
    n_blocks = int(st[0] + st[5] + st[10])
    nb = C.c_uint64(0)
    lens_ms, str_ms, walls, out_bytes = [], [], [], 0
    os.environ["OATK_DEBUG_EC_STAGES"] = "1"
    for _ in range(3):
        t0 = time.perf_counter()
        rc, txt = stderr_of(lambda: hip.L.oatk_hip_ec_corrected_reads(hip.h, C.byref(nb)))
        walls.append(1e3 * (time.perf_counter() - t0))
        assert rc == 0, hip.L.oatk_hip_last_error(hip.h)
        m = re.search(r"lengths \+ offsets ([0-9.]+) ms, strings ([0-9.]+) ms \((\d+) reads, (\d+) blocks, (\d+) bytes written\)", txt)
        lens_ms.append(float(m.group(1))), str_ms.append(float(m.group(2)))
        out_bytes = int(m.group(5))
    del os.environ["OATK_DEBUG_EC_STAGES"]
    floor_ms = 2 * out_bytes / (HBM_TBS * 1e12) * 1e3
    s_med, s_all = med(str_ms)
    print("  %d blocks, %.3f G corrected bases, %.3f GB of packed strings" % (n_blocks, nb.value / 1e9, out_bytes / 1e9))
    print("  length pass + offsets  %8.3f ms (%s)" % med(lens_ms))
    print("  write kernel           %8.3f ms (%s): %.2f TB/s read + written, %.1f x the %.3f ms that %.1f TB/s allows" % (s_med, s_all, 2 * out_bytes / s_med / 1e9, s_med / floor_ms, floor_ms, HBM_TBS))
    print("  oatk_hip_ec_corrected_reads, wall  %8.2f ms (%s)" % med(walls), flush=True)
    if adaptor:
        H = C.CDLL(_lib.HOST_LIB_PATH)
        H.oatk_sr_db_new.restype = vp
        H.oatk_sr_db_new.argtypes = [C.c_int, C.c_int]
        H.oatk_sr_read_packed.argtypes = [vp, vp, vp, vp, vp, C.c_uint64, C.c_uint64, vp]
        H.oatk_collect_syncmer_from_reads.restype = vp
        H.oatk_collect_syncmer_from_reads.argtypes = [vp, vp, C.POINTER(C.c_int)]
        args = [vp, vp, vp, vp, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double]
        H.oatk_read_error_correction.argtypes = args + [vp]
        H.oatk_read_error_correction_fo.argtypes = args + [vp, vp]
        H.oatk_sr_db_clean.argtypes = [vp]
        H.oatk_syncmer_db_destroy.argtypes = [vp]
        libc = C.CDLL(None)
        libc.fopen.restype = vp
        libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
        libc.fclose.argtypes = [vp]
        res = {}
        for with_fo in (False, True):
            db = H.oatk_sr_db_new(K, S)
            assert H.oatk_sr_read_packed(hip.h, db, seq.ctypes.data, off.ctypes.data, lens.ctypes.data, n, seq.size, None) == 0
            rc = C.c_int(0)
            scm = H.oatk_collect_syncmer_from_reads(hip.h, db, C.byref(rc))
            assert scm and rc.value == 0
            st = np.zeros(12, np.uint64)
            fo = libc.fopen(b"/dev/null", b"w") if with_fo else None
            t0 = time.perf_counter()
            if with_fo:
                r = H.oatk_read_error_correction_fo(hip.h, db, scm, None, 0.02, c, 10 * c, c, 0.35, fo, st.ctypes.data)
            else:
                r = H.oatk_read_error_correction(hip.h, db, scm, None, 0.02, c, 10 * c, c, 0.35, st.ctypes.data)
            res[with_fo] = time.perf_counter() - t0
            assert r == 0, hip.L.oatk_hip_last_error(hip.h)
            if fo:
                libc.fclose(fo)
            H.oatk_syncmer_db_destroy(scm)
            H.oatk_sr_db_clean(db)
        print("  adaptor: oatk_read_error_correction %.2f s, oatk_read_error_correction_fo to /dev/null %.2f s: the sequences add %.2f s (%.2f Gbases/s of text)"
              % (res[False], res[True], res[True] - res[False], nb.value / 1e9 / max(res[True] - res[False], 1e-9)), flush=True)
    hip.close()


if __name__ == "__main__":
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or ["config2", "config3"]
    for nm in names:
        run(nm, "--no-adaptor" not in sys.argv)
