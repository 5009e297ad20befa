#!/usr/bin/env python3
"""Device time of the mini-circle repeat units (oatk_hip_ra_minicircle_units on the alignments resident in the handle) per phase -- units, valid records and
their paths, distinct paths -- between events on the handle's stream, and beside it the time of merely downloading RA_ALN_OFF + RA_FRG_UID, which is the floor
of the host route the call replaces (extract_minicircles_with_anchor, path_finder.c:640, reads every record on the host).  The median of 20 runs after 5 warm-up
runs each.  The reads are oatk_amd.synth CONFIG1S (200 k reads, two organelles over a nuclear background); scan, count, EC and the alignment on the device,
graph and unitigs by the compiled reference: needs oracle/_ref (built where the reference sources exist).  The anchor is the unitig with the most fragments.
Development aid.
usage: python tests/minicircle_time.py [n_reads [output file]]      (default output: profiles/minicircle_time.txt)"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # tests/ may use the compiled reference; tools/ may not
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import minicircle_util as MC  # noqa: E402
import test_gpu_align as GA  # noqa: E402
from oatk_amd import HipSyncasm, synth  # noqa: E402

vp = C.c_void_p
K, S = 1001, 31
WARM, RUNS = 5, 20


def main(n, out_path):
    cfg = dict(synth.CONFIG1S)
    cfg["n_reads"] = n
    c = cfg["min_k_cov"]
    L, H = GA.setup_libs()
    H.oatk_sr_db_new.restype = vp
    H.oatk_sr_db_new.argtypes = [C.c_int, C.c_int]
    H.oatk_sr_read_packed.argtypes = [vp, vp, vp, vp, vp, C.c_uint64, C.c_uint64, vp]
    H.oatk_collect_syncmer_from_reads.restype = vp
    H.oatk_collect_syncmer_from_reads.argtypes = [vp, vp, C.POINTER(C.c_int)]
    L.refx_make_graph.restype = vp
    L.refx_make_graph.argtypes = [vp, vp, C.c_uint32, C.c_double]
    L.refx_scg_destroy.argtypes = [vp]
    rs = synth.MixReadSet(**cfg)
    seq, off, lens = rs.slice(0, n)
    lines = ["%d reads, %.2f Gbases (CONFIG1S), k = %d" % (n, int(lens.sum()) / 1e9, K)]
    print(lines[-1], flush=True)
    hip = HipSyncasm(0)
    db = H.oatk_sr_db_new(K, S)
    assert H.oatk_sr_read_packed(hip.h, db, seq.ctypes.data, off.ctypes.data, lens.ctypes.data, n, seq.size, None) == 0
    del seq
    rc = C.c_int(0)
    scm = H.oatk_collect_syncmer_from_reads(hip.h, db, C.byref(rc))
    assert scm and rc.value == 0
    st = np.zeros(12, np.uint64)
    assert H.oatk_read_error_correction(hip.h, db, scm, None, 0.02, c, 10 * c, c, 0.35, st.ctypes.data) == 0
    g = L.refx_make_graph(db, scm, c, 0.35)
    assert g
    L.refx_process_unitigs(g)
    v = L.refx_ra_new()
    nsk = C.c_uint64(0)
    assert H.oatk_scg_read_alignment(hip.h, db, v, g, 0, C.byref(nsk), None) == 0      # leaves the alignments resident
    a_off, f_uid = hip.fetch("RA_ALN_OFF"), hip.fetch("RA_FRG_UID")
    n_frg = np.diff(a_off.astype(np.int64))
    anchor = int(np.bincount((f_uid >> np.uint64(1)).astype(np.int64)).argmax())
    lines.append("%d alignment records, %d fragments (%d records of 1-4, %d over %d, the longest %d), anchor = unitig %d"
                 % (len(n_frg), len(f_uid), int(((n_frg >= 1) & (n_frg <= 4)).sum()), int((n_frg > 32).sum()), 32, int(n_frg.max()), anchor))
    print(lines[-1], flush=True)
    # the device call
    ms, wall = [], []
    for it in range(WARM + RUNS):
        t0 = time.perf_counter()
        got = hip.L.oatk_hip_ra_minicircle_units(hip.h, None, anchor, *[C.byref(x) for x in (C.c_uint64(), C.c_uint64(), C.c_uint64())])
        t1 = time.perf_counter()
        assert got == 0, hip.L.oatk_hip_last_error(hip.h)
        if it >= WARM:
            ms.append(hip.ra_minicircle_times()[0])
            wall.append(1e3 * (t1 - t0))
    unit, p_off, p_v, p_cnt = hip.ra_minicircle_units(anchor)
    mcs, paths, cnt = MC.extract(a_off, f_uid, anchor)
    assert np.array_equal(unit, mcs) and p_cnt.tolist() == cnt and np.array_equal(p_v, MC.flat_paths(paths)[1]), "the device differs from the model"
    lines.append("%d valid records, %d distinct paths (equal to the model of tests/minicircle_util.py)" % (int(p_cnt.sum()), len(p_cnt)))
    for k, name in enumerate(("units", "paths", "distinct")):
        x = [m[k] for m in ms]
        lines.append("  device, %-22s %8.3f ms   (min %.3f, max %.3f)" % (name, statistics.median(x), min(x), max(x)))
    x = [sum(m) for m in ms]
    lines.append("  device, %-22s %8.3f ms   (min %.3f, max %.3f)" % ("the three together", statistics.median(x), min(x), max(x)))
    lines.append("  %-30s %8.3f ms   (min %.3f, max %.3f)" % ("the call, host clock", statistics.median(wall), min(wall), max(wall)))
    # the floor of the host route: the two arrays it reads, into host memory that is there already
    bufs = [(hip.buffer(b), np.zeros_like(h)) for b, h in (("RA_ALN_OFF", a_off), ("RA_FRG_UID", f_uid))]
    dl = []
    for it in range(WARM + RUNS):
        t0 = time.perf_counter()
        for (p, b), h in bufs:
            assert hip.L.oatk_hip_d2h(hip.h, h.ctypes.data, p, b) == 0
        if it >= WARM:
            dl.append(1e3 * (time.perf_counter() - t0))
    assert np.array_equal(bufs[1][1], f_uid)
    lines.append("  %-30s %8.3f ms   (min %.3f, max %.3f; %.1f MB)" % ("download of off + uid alone", statistics.median(dl), min(dl), max(dl),
                                                                         sum(b for (p, b), h in bufs) / 1e6))
    print("\n".join(lines[2:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    L.refx_ra_destroy(v)
    L.refx_scg_destroy(g)
    L.refx_scmdb_destroy(scm)
    L.refx_srdb_destroy(db)
    hip.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else synth.CONFIG1S["n_reads"],
         sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "minicircle_time.txt"))
