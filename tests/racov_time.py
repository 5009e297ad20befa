#!/usr/bin/env python3
"""Wall clock of the coverage estimates from read alignments at run_syncasm.c:295-297: the compiled reference's scg_ra_utg_coverage +
scg_ra_arc_coverage(refine = 1) against the device adaptor pair (oatk_scg_ra_utg_coverage + oatk_scg_ra_arc_coverage + the reference's
scg_refine_arc_coverage), once with the alignments and chains resident in the handle and once uploaded; the median of 3 each, after checking
that every vtx[].cov and arc[].cov is the same.  The state is the real one: config-3 reads (oatk_amd.synth CONFIGS), scan, count, EC and
assembly graph on the device, then the reference's tail from the unitigging on with the alignments on the device, stopped at :295.
Needs oracle/_ref (built where the reference sources exist).  Development aid.
usage: python tests/racov_time.py [n_reads ...]      (default: 200000 2000000; at 2 M reads the uploaded pair must take <= 1/3 of the reference's)"""
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
from oatk_amd import HipSyncasm, _lib  # noqa: E402
from oatk_amd.synth import CONFIGS, ReadSet  # noqa: E402
from racov_util import Scg  # noqa: E402

vp = C.c_void_p
K, S, T = 1001, 31, 16
L = R.lib()
H = C.CDLL(_lib.HOST_LIB_PATH)
H.oatk_sr_db_new.restype = vp
H.oatk_sr_db_new.argtypes = [C.c_int, C.c_int]
H.oatk_sr_read_packed.argtypes = [vp, vp, vp, vp, vp, C.c_uint64, C.c_uint64, vp]
H.oatk_collect_syncmer_from_reads.restype = vp
H.oatk_collect_syncmer_from_reads.argtypes = [vp, vp, C.POINTER(C.c_int)]
H.oatk_read_error_correction.argtypes = [vp, vp, vp, vp, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, vp]
H.oatk_make_syncmer_asmg.restype = vp
H.oatk_make_syncmer_asmg.argtypes = [vp, vp, C.c_uint32, C.c_double, C.POINTER(C.c_int)]
H.oatk_scg_read_alignment.argtypes = [vp, vp, vp, vp, C.c_int, C.POINTER(C.c_uint64), C.POINTER(vp)]
H.oatk_scg_ra_utg_coverage.argtypes = [vp, vp, vp, vp, C.c_uint, C.c_int]
H.oatk_scg_ra_arc_coverage.argtypes = [vp, vp, vp, vp, C.c_uint, C.c_int]
L.refx_syncasm_tail_graph.restype = C.c_int
L.refx_syncasm_tail_graph.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_char_p]
L.refx_set_aligner.argtypes = [vp]
L.scg_ra_utg_coverage.argtypes = [vp, vp, vp, C.c_int]
L.scg_ra_arc_coverage.argtypes = [vp, vp, vp, C.c_int, C.c_int]
L.scg_refine_arc_coverage.argtypes = [vp, C.c_int]


def covs(g):
    a = C.cast(g, C.POINTER(Scg)).contents.utg_asmg.contents
    return (np.array([a.vtx[i].cov for i in range(a.n_vtx)], np.uint32), np.array([a.arc[i].cov for i in range(a.n_arc)], np.uint32))


def restore(g, snap):
    a = C.cast(g, C.POINTER(Scg)).contents.utg_asmg.contents
    for i in range(a.n_vtx):
        a.vtx[i].cov = int(snap[0][i])
    for i in range(a.n_arc):
        a.arc[i].cov = int(snap[1][i])


def measure(hip, db, v, g):
    a = C.cast(g, C.POINTER(Scg)).contents.utg_asmg.contents
    snap = covs(g)
    out = {}

    def ref():
        L.scg_ra_utg_coverage(g, db, v, 0)
        L.scg_ra_arc_coverage(g, db, v, 1, 0)

    def dev(flags_u, flags_a):
        def run():
            assert H.oatk_scg_ra_utg_coverage(hip.h, db, v, g, flags_u, 0) == 0, hip.L.oatk_hip_last_error(hip.h)
            assert H.oatk_scg_ra_arc_coverage(hip.h, db, v, g, flags_a, 0) == 0, hip.L.oatk_hip_last_error(hip.h)
            L.scg_refine_arc_coverage(g, 0)
        return run

    want = None
    for name, fn in (("reference", ref), ("device, resident", dev(3, 2)), ("device, uploaded", dev(0, 0))):
        ts = []
        for _ in range(3):
            restore(g, snap)
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
            got = covs(g)
            if want is None:
                want = got
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
        out[name] = statistics.median(ts)
        print("  %-18s %9.1f ms   (%s)" % (name, 1e3 * out[name], ", ".join("%.1f" % (1e3 * t) for t in ts)), flush=True)
    restore(g, snap)
    print("  %d unitigs, %d arcs, %d alignment records (%s)" % (a.n_vtx, a.n_arc, C.cast(v, C.POINTER(C.c_size_t))[0], "the covs of all three are identical"))
    return out


def run(n):
    cfg = CONFIGS["config3"]
    cov = cfg["min_k_cov"]
    rs = ReadSet(cfg["genome_len"], n, cfg["mean_len"])
    seq, off, lens = rs.slice(0, n, threads=16)
    print("%d reads, %.2f Gbases (config-3 shape)" % (n, int(lens.sum()) / 1e9), flush=True)
    hip = HipSyncasm(0)
    db = H.oatk_sr_db_new(K, S)
    assert H.oatk_sr_read_packed(hip.h, db, seq.ctypes.data, off.ctypes.data, lens.ctypes.data, n, seq.size, None) == 0
    del seq
    rc = C.c_int(0)
    scm = H.oatk_collect_syncmer_from_reads(hip.h, db, C.byref(rc))
    st = np.zeros(12, np.uint64)
    assert H.oatk_read_error_correction(hip.h, db, scm, None, 0.02, cov, 10 * cov, cov, 0.35, st.ctypes.data) == 0
    asmg = H.oatk_make_syncmer_asmg(hip.h, scm, cov, 0.35, C.byref(rc))
    assert asmg and rc.value == 0
    state = {"no_unzip": 0, "res": None}

    def aligner(db_, v, g, n_threads, for_unzip):
        nsk = C.c_uint64(0)
        assert H.oatk_scg_read_alignment(hip.h, db_, v, g, for_unzip, C.byref(nsk), None) == 0 and nsk.value == 0
        if for_unzip == 0:
            state["no_unzip"] += 1
            if state["no_unzip"] == 2:                     # :295, after the unzip rounds and the demultiplexing (:259)
                state["res"] = measure(hip, db_, v, g)

    cb = C.CFUNCTYPE(None, vp, vp, vp, C.c_int, C.c_int)(aligner)
    L.refx_set_aligner(cb)
    out = os.path.join(tempfile.mkdtemp(), "dev")
    assert L.refx_syncasm_tail_graph(db, scm, asmg, K, 100000, 10000, cov, 0.35, 0.3, 3, T, out.encode()) == 0
    L.refx_set_aligner(None)
    L.refx_scmdb_destroy(scm)
    L.refx_srdb_destroy(db)
    hip.close()
    r = state["res"]
    assert r is not None, "the tail never reached run_syncasm.c:295"
    print("  uploaded / reference = %.3f, resident / reference = %.3f" % (r["device, uploaded"] / r["reference"], r["device, resident"] / r["reference"]), flush=True)
    return r


if __name__ == "__main__":
    sizes = [int(x) for x in sys.argv[1:]] or [200000, 2000000]
    res = {n: run(n) for n in sizes}
    for n, r in res.items():
        if n >= 2000000:
            assert r["device, uploaded"] <= r["reference"] / 3, "at %d reads the uploaded pair takes more than a third of the reference's" % n
