#!/usr/bin/env python3
"""Wall clock of scg_consensus (syncasm.c:716-823; run_syncasm.c calls it four to eight times per assembly) on the unitig graph of the corrected reads, three ways,
the median of 3 each, every sample on a graph of its own:
  device      oatk_scg_consensus(hoco = 0, save_seq = 1): one plan to the device, the text back (with the HIP-event times of the length and fill kernels and
              the bytes per second they reach, from shapes: 4 k + k / 4 bytes read per piece and kernel, plus the bytes written)
  host        the route there was before: oatk_consensus_fetch (CONS_RL to the host) + oatk_scg_unitig_consensus over every live unitig
  reference   the compiled reference's scg_consensus
and the bytes each of the first two copies to the host: 4 * k * n_sel against total_bytes + 17 * n_seq.  The graphs the device and the reference leave are
compared array by array first.  The reads are oatk_amd.synth CONFIG1S (200 k reads, two organelles over a nuclear background); scan, count and EC on the device.
Needs oracle/_ref (built where the reference sources exist).  Development aid.
usage: python tests/cons_strings_time.py [n_reads]"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # tests/ may use the compiled reference; tools/ may not
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ec_util as E  # noqa: E402
import ref_lib as R  # noqa: E402
from oatk_amd import HipSyncasm, _lib, synth  # noqa: E402
from racov_util import Scg  # noqa: E402

vp = C.c_void_p
K, S = 1001, 31


class KString(C.Structure):
    _fields_ = [("l", C.c_size_t), ("m", C.c_size_t), ("s", C.c_void_p)]


def main(n):
    cfg = dict(synth.CONFIG1S)
    cfg["n_reads"] = n
    c = cfg["min_k_cov"]
    L, H = R.lib(), C.CDLL(_lib.HOST_LIB_PATH)
    H.oatk_sr_db_new.restype = vp
    H.oatk_sr_db_new.argtypes = [C.c_int, C.c_int]
    H.oatk_sr_read_packed.argtypes = [vp, vp, vp, vp, vp, C.c_uint64, C.c_uint64, vp]
    H.oatk_collect_syncmer_from_reads.restype = vp
    H.oatk_collect_syncmer_from_reads.argtypes = [vp, vp, C.POINTER(C.c_int)]
    H.oatk_read_error_correction.argtypes = [vp, vp, vp, vp, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, vp]
    H.oatk_overlap_fetch.restype = vp
    H.oatk_overlap_fetch.argtypes = [vp, C.POINTER(C.c_int)]
    H.oatk_consensus_fetch.restype = vp
    H.oatk_consensus_fetch.argtypes = [vp, C.c_uint32, C.c_int, C.POINTER(C.c_int)]
    H.oatk_consensus_destroy.argtypes = [vp]
    H.oatk_scg_unitig_consensus.restype = C.c_int64
    H.oatk_scg_unitig_consensus.argtypes = [vp, vp, vp, vp, C.c_uint64, C.POINTER(KString), C.c_int]
    H.oatk_scg_consensus.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp]
    L.refx_process_unitigs.argtypes = [vp]
    libc = C.CDLL(None)
    libc.free.argtypes = [vp]
    rs = synth.MixReadSet(**cfg)
    seq, off, lens = rs.slice(0, n)
    print("%d reads, %.2f Gbases (CONFIG1S), k = %d" % (n, int(lens.sum()) / 1e9, K), flush=True)
    hip = HipSyncasm(0)
    db = H.oatk_sr_db_new(K, S)
    assert H.oatk_sr_read_packed(hip.h, db, seq.ctypes.data, off.ctypes.data, lens.ctypes.data, n, seq.size, None) == 0
    del seq
    rc = C.c_int(0)
    scm = H.oatk_collect_syncmer_from_reads(hip.h, db, C.byref(rc))
    assert scm and rc.value == 0
    st = np.zeros(12, np.uint64)
    assert H.oatk_read_error_correction(hip.h, db, scm, None, 0.02, c, 10 * c, c, 0.35, st.ctypes.data) == 0
    ov = H.oatk_overlap_fetch(hip.h, C.byref(rc))
    assert ov and rc.value == 0
    hip.set_timing(True)

    def graph():
        g = L.refx_make_graph(db, scm, c, 0.35)
        assert g
        L.refx_process_unitigs(g)
        return g

    ts = {"device: oatk_hip_consensus": [], "device: oatk_scg_consensus": [], "host: fetch + unitig strings": [], "reference: scg_consensus": []}
    kern = []
    for it in range(3):
        g_dev, g_host, g_ref = graph(), graph(), graph()
        t0 = time.perf_counter()
        hip.consensus(c)
        t1 = time.perf_counter()
        r = H.oatk_scg_consensus(hip.h, ov, db, g_dev, 0, 1, None)
        t2 = time.perf_counter()
        assert r == 0, hip.L.oatk_hip_last_error(hip.h)
        ts["device: oatk_hip_consensus"].append(t1 - t0)
        ts["device: oatk_scg_consensus"].append(t2 - t1)
        ms_len, ms_fill, n_piece = hip.consensus_strings_times()
        total, n_seq = hip.buffer("CONS_STR")[1], hip.buffer("CONS_STR_LEN")[1] // 8
        n_sel = hip.buffer("CONS_SEL")[1] // 4
        kern.append((ms_len, ms_fill))
        # the route there was: the tables to the host, every unitig's string appended there
        a = C.cast(g_host, C.POINTER(Scg)).contents.utg_asmg.contents
        t0 = time.perf_counter()
        cs = H.oatk_consensus_fetch(hip.h, c, K, C.byref(rc))
        assert cs and rc.value == 0
        host_bytes = 0
        for i in range(a.n_vtx):
            if a.vtx[i].del_:
                continue
            ks = KString(0, 0, None)
            l = H.oatk_scg_unitig_consensus(cs, ov, db, a.vtx[i].a, a.vtx[i].n, C.byref(ks), 0)
            assert l >= 0
            host_bytes += l
            libc.free(ks.s)
        H.oatk_consensus_destroy(cs)
        ts["host: fetch + unitig strings"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        L.refx_consensus(db, g_ref, 0, 1)
        ts["reference: scg_consensus"].append(time.perf_counter() - t0)
        if it == 0:
            A, B = E.flatten_graph(g_dev), E.flatten_graph(g_ref)
            for f in ("vtx_len", "vtx_cov", "seq", "arc_ls"):
                assert np.array_equal(A[f], B[f]), f
            assert host_bytes == int(A["vtx_len"].sum())
            print("  %d unitigs, %d arcs, %d sequences in the plan, %d pieces, %d selected syncmers, %d bytes of text; the graphs of device and reference are identical"
                  % (A["n_vtx"], A["n_arc"], n_seq, n_piece, n_sel, total), flush=True)
        for g in (g_dev, g_host, g_ref):
            L.refx_scg_destroy(g)
    for name, t in ts.items():
        print("  %-30s %9.1f ms   (%s)" % (name, 1e3 * statistics.median(t), ", ".join("%.1f" % (1e3 * x) for x in t)), flush=True)
    ms_len, ms_fill = statistics.median(x[0] for x in kern), statistics.median(x[1] for x in kern)
    rd = n_piece * (4 * K + K // 4)
    print("  length kernel %.3f ms (%.1f GB/s: %d bytes read), fill kernel %.3f ms (%.1f GB/s: %d read + %d written)"
          % (ms_len, rd / ms_len / 1e6 if ms_len else 0.0, rd, ms_fill, (rd + total) / ms_fill / 1e6 if ms_fill else 0.0, rd, total))
    print("  copied to the host: %d bytes by the host route (4 * k * n_sel), %d by the device route (total_bytes + 17 * n_seq)" % (4 * K * n_sel, total + 17 * n_seq))
    H.oatk_overlap_destroy.argtypes = [vp]
    H.oatk_overlap_destroy(ov)
    L.refx_scmdb_destroy(scm)
    L.refx_srdb_destroy(db)
    hip.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else synth.CONFIG1S["n_reads"])
