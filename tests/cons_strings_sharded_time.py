#!/usr/bin/env python3
"""Wall clock of scg_consensus (syncasm.c:716-823) with the reads sharded over 2 and 4 handles on one GPU (include/oatk_multi.h), two ways, the median of 3 each,
every sample on a graph of its own:
  device   oatk_multi_consensus + oatk_multi_scg_consensus(hoco = 0, save_seq = 1): the first call after a consensus exchanges the k-mer table (one all-reduce),
           a second call on the same consensus exchanges nothing -- both are timed, with the HIP-event time of the k-mer kernel on handle 0
  host     the route there was before: oatk_multi_consensus_fetch (the sharded consensus, then CONS_RL to the host) + oatk_scg_unitig_consensus over every
           live unitig
and the bytes each copies to the host (4 * k * n_sel against total_bytes + 17 * n_seq) and the bytes of the k-mer table every handle puts into the all-reduce.
The text of the device route is compared with the host route's, unitig by unitig, first.  The reads are oatk_amd.synth CONFIG1S cut to n_reads (default 40 000:
the handles read them from a FASTA file written to a temporary directory, 15 kb a read); scan, count and EC on the devices.  Over the in-process communicator
group the "all-reduce" is device-to-device copies and a kernel on one GPU: the times say what the calls cost there, not what xGMI would.
Needs oracle/_ref (built where the reference sources exist) for the unitig graph.  Development aid.
usage: python tests/cons_strings_sharded_time.py [n_reads]"""
import ctypes as C
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # tests/ may use the compiled reference; tools/ may not
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_lib as R  # noqa: E402
from oatk_amd import _lib, synth  # noqa: E402
from racov_util import Scg  # noqa: E402

vp = C.c_void_p
K, S = 1001, 31


class KString(C.Structure):
    _fields_ = [("l", C.c_size_t), ("m", C.c_size_t), ("s", C.c_void_p)]


def buf_bytes(Lh, ctx, name):
    d, b = C.c_void_p(), C.c_uint64()
    assert Lh.oatk_hip_buffer(ctx, _lib.BUF[name], C.byref(d), C.byref(b)) == 0, name
    return int(b.value)


def run(n_handles, fa, c, out):
    L, H, Lh = R.lib(), _lib.load_host(), _lib.load()
    H.oatk_multi_consensus_fetch.restype = vp
    H.oatk_multi_consensus_fetch.argtypes = [vp, C.c_uint32, C.c_int, C.POINTER(C.c_int)]
    H.oatk_consensus_destroy.argtypes = [vp]
    H.oatk_scg_unitig_consensus.restype = C.c_int64
    H.oatk_scg_unitig_consensus.argtypes = [vp, vp, vp, vp, C.c_uint64, C.POINTER(KString), C.c_int]
    L.refx_process_unitigs.argtypes = [vp]
    libc = C.CDLL(None)
    libc.free.argtypes = [vp]
    m = H.oatk_multi_create((C.c_int * n_handles)(*([0] * n_handles)), n_handles)
    assert m
    db = H.oatk_sr_db_new(K, S)
    assert H.oatk_multi_sr_read_files(m, db, R._files_arg([fa]), 1) == 0, H.oatk_multi_last_error(m)
    rc = C.c_int(0)
    scm = H.oatk_multi_collect_syncmer_from_reads(m, db, C.byref(rc))
    assert scm and rc.value == 0, H.oatk_multi_last_error(m)
    st = np.zeros(12, np.uint64)
    assert H.oatk_multi_read_error_correction(m, db, scm, 0.02, c, 10 * c, c, 0.35, st.ctypes.data) == 0, H.oatk_multi_last_error(m)
    ov = H.oatk_multi_overlap_fetch(m, c, C.byref(rc))
    assert ov and rc.value == 0, H.oatk_multi_last_error(m)
    ctx0 = H.oatk_multi_ctx(m, 0)
    for r in range(n_handles):
        Lh.oatk_hip_set_timing(H.oatk_multi_ctx(m, r), 1)

    def graph():
        g = L.refx_make_graph(db, scm, c, 0.35)
        assert g
        L.refx_process_unitigs(g)
        return g

    names = ["device: oatk_multi_consensus", "device: oatk_multi_scg_consensus, first (k-mer table)", "device: oatk_multi_scg_consensus, again", "host: oatk_multi_consensus_fetch",
             "host: unitig strings"]
    ts = {k: [] for k in names}
    kern = []
    for it in range(3):
        g_dev, g_dev2, g_host = graph(), graph(), graph()
        t0 = time.perf_counter()
        assert H.oatk_multi_consensus(m, c) == 0, H.oatk_multi_last_error(m)
        t1 = time.perf_counter()
        assert H.oatk_multi_scg_consensus(m, ov, db, g_dev, 0, 1, None) == 0, H.oatk_multi_last_error(m)
        t2 = time.perf_counter()
        assert H.oatk_multi_scg_consensus(m, ov, db, g_dev2, 0, 1, None) == 0, H.oatk_multi_last_error(m)
        t3 = time.perf_counter()
        for k, t in zip(names[:3], (t1 - t0, t2 - t1, t3 - t2)):
            ts[k].append(t)
        ms, table = C.c_float(), C.c_uint64()
        assert Lh.oatk_hip_consensus_kmer_time(ctx0, C.byref(ms), C.byref(table)) == 0
        kern.append(float(ms.value))
        total, n_seq, n_sel = buf_bytes(Lh, ctx0, "CONS_STR"), buf_bytes(Lh, ctx0, "CONS_STR_LEN") // 8, buf_bytes(Lh, ctx0, "CONS_SEL") // 4
        # the route there was: the tables to the host, every unitig's string appended there
        a, d = (C.cast(g, C.POINTER(Scg)).contents.utg_asmg.contents for g in (g_host, g_dev))
        t0 = time.perf_counter()
        cs = H.oatk_multi_consensus_fetch(m, c, K, C.byref(rc))
        assert cs and rc.value == 0, H.oatk_multi_last_error(m)
        t1 = time.perf_counter()
        n_utg = 0
        for i in range(a.n_vtx):
            if a.vtx[i].del_:
                continue
            ks = KString(0, 0, None)
            ln = H.oatk_scg_unitig_consensus(cs, ov, db, a.vtx[i].a, a.vtx[i].n, C.byref(ks), 0)
            assert ln >= 0
            if it == 0:
                assert ln == d.vtx[i].len and C.string_at(ks.s, ln) == C.string_at(d.vtx[i].seq, ln), "unitig %d: the device text differs from the host route's" % i
            n_utg += 1
            libc.free(ks.s)
        t2 = time.perf_counter()
        H.oatk_consensus_destroy(cs)
        ts[names[3]].append(t1 - t0)
        ts[names[4]].append(t2 - t1)
        if it == 0:
            print("  %d handles: %d unitigs, %d sequences in the plan, %d selected syncmers, %d bytes of text; device and host route give the same text"
                  % (n_handles, n_utg, n_seq, n_sel, total), file=out, flush=True)
        for g in (g_dev, g_dev2, g_host):
            L.refx_scg_destroy(g)
    for name, t in ts.items():
        print("    %-56s %9.1f ms   (%s)" % (name, 1e3 * statistics.median(t), ", ".join("%.1f" % (1e3 * x) for x in t)), file=out, flush=True)
    print("    k-mer kernel on handle 0: %.3f ms for a table of %d bytes (what every handle puts into the one all-reduce; CONS_TOT, all-reduced by the consensus, is %d)"
          % (statistics.median(kern), int(table.value), 8 * K * n_sel), file=out)
    print("    copied to the host: %d bytes by the host route (4 * k * n_sel), %d by the device route (total_bytes + 17 * n_seq)" % (4 * K * n_sel, total + 17 * n_seq),
          file=out, flush=True)
    H.oatk_overlap_destroy(ov)
    L.refx_scmdb_destroy(scm)
    L.refx_srdb_destroy(db)
    H.oatk_multi_destroy(m)


def main(n):
    cfg = dict(synth.CONFIG1S)
    cfg["n_reads"] = n
    c = cfg["min_k_cov"]
    rs = synth.MixReadSet(**cfg)
    seq, off, lens = rs.slice(0, n, threads=16)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp, open(os.path.join(ROOT, "profiles", "cons_strings_sharded_time.txt"), "w") as out:
        fa = os.path.join(tmp, "reads.fa")
        synth.write_fasta(fa, seq, off, lens, threads=16)
        print("%d reads, %.2f Gbases (CONFIG1S), k = %d, every handle on device 0 (in-process communicator group)" % (n, int(lens.sum()) / 1e9, K), file=out, flush=True)
        del seq
        for n_handles in (2, 4):
            run(n_handles, fa, c, out)
    print(open(os.path.join(ROOT, "profiles", "cons_strings_sharded_time.txt")).read())


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 40_000)
