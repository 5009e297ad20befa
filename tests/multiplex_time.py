#!/usr/bin/env python3
"""Wall clock of scg_multiplex's spanning-triplet table in the first unzip round (run_syncasm.c:219-232): the plan from the device
(oatk_scg_multiplex_plan: flatten, table on the device, decisions) with the alignments resident in the handle and uploaded, and -- as the
upper bound of what the table's loop can cost -- the compiled reference's WHOLE scg_multiplex (table, decisions and rewrite of the graph) on
the same structures; the median of 3 each.  scg_multiplex rewrites its graph, so every sample is taken on a state of its own: graph,
unitigs, alignment and coverage update are redone from the corrected reads, the device is timed first (it changes nothing), the reference
last, and the plan's `updated` must be what the reference then returns.
The reads are oatk_amd.synth CONFIG1S (200 k reads, two organelles over a nuclear background); scan, count and EC on the device.
Needs oracle/_ref (built where the reference sources exist).  Development aid.
usage: python tests/multiplex_time.py [n_reads]"""
import ctypes as C
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # tests/ may use the compiled reference; tools/ may not
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multiplex_util as MX  # noqa: E402
import ref_lib as R  # noqa: E402
import test_gpu_align as GA  # noqa: E402
from oatk_amd import HipSyncasm, _lib, synth  # noqa: E402

vp = C.c_void_p
K, S = 1001, 31


def main(n):
    cfg = dict(synth.CONFIG1S)
    cfg["n_reads"] = n
    c = cfg["min_k_cov"]
    L, H = GA.setup_libs()
    H.oatk_sr_db_new.restype = vp
    H.oatk_sr_db_new.argtypes = [C.c_int, C.c_int]
    H.oatk_sr_read_packed.argtypes = [vp, vp, vp, vp, vp, C.c_uint64, C.c_uint64, vp]
    H.oatk_collect_syncmer_from_reads.restype = vp
    H.oatk_collect_syncmer_from_reads.argtypes = [vp, vp, C.POINTER(C.c_int)]
    H.oatk_scg_multiplex_plan.argtypes = [vp, vp, vp, C.c_uint, C.c_uint32, C.c_double, C.c_double, vp, C.POINTER(C.c_int), vp]
    L.refx_make_graph.restype = vp
    L.refx_make_graph.argtypes = [vp, vp, C.c_uint32, C.c_double]
    L.refx_scg_destroy.argtypes = [vp]
    rs = synth.MixReadSet(**cfg)
    seq, off, lens = rs.slice(0, n)
    print("%d reads, %.2f Gbases (CONFIG1S)" % (n, int(lens.sum()) / 1e9), flush=True)
    hip = HipSyncasm(0)
    db = H.oatk_sr_db_new(K, S)
    assert H.oatk_sr_read_packed(hip.h, db, seq.ctypes.data, off.ctypes.data, lens.ctypes.data, n, seq.size, None) == 0
    del seq
    rc = C.c_int(0)
    scm = H.oatk_collect_syncmer_from_reads(hip.h, db, C.byref(rc))
    assert scm and rc.value == 0
    st = np.zeros(12, np.uint64)
    assert H.oatk_read_error_correction(hip.h, db, scm, None, 0.02, c, 10 * c, c, 0.35, st.ctypes.data) == 0
    max_n_scm = int(math.ceil(30000.0 / K))
    ts = {"device, resident": [], "device, uploaded": [], "reference, whole scg_multiplex": []}
    for it in range(3):
        g = L.refx_make_graph(db, scm, c, 0.35)
        assert g
        L.refx_process_unitigs(g)
        v = L.refx_ra_new()
        nsk = C.c_uint64(0)
        assert H.oatk_scg_read_alignment(hip.h, db, v, g, 1, C.byref(nsk), None) == 0 and nsk.value == 0
        L.refx_update_utg_cov(g)
        nu = MX.C.cast(g, C.POINTER(MX.Scg)).contents.utg_asmg.contents.n_vtx
        mv, upd = np.zeros(max(nu, 1), np.uint8), [C.c_int(-1), C.c_int(-1)]
        for k, (name, flags) in enumerate((("device, resident", 2), ("device, uploaded", 0))):
            t0 = time.perf_counter()
            rc_ = H.oatk_scg_multiplex_plan(hip.h, v, g, flags, max_n_scm, 10.0, 0.3, mv.ctypes.data, C.byref(upd[k]), None)
            ts[name].append(time.perf_counter() - t0)
            assert rc_ == 0, hip.L.oatk_hip_last_error(hip.h)
        if it == 0:
            aln = MX.flat_aln(GA.flatten(L, v))
            got = hip.ra_triplet_scores(MX.flatten_graph(g))
            print("  %d unitigs, %d alignment records, %d of three or more fragments, %d triplet slots, %d pairs, %d with a score"
                  % (nu, len(aln["sid"]), *MX.triplet_records(aln), len(got["have"]), int(got["have"].sum())), flush=True)
        t0 = time.perf_counter()
        updated = L.refx_multiplex(g, v, max_n_scm, 10.0, 0.3)
        ts["reference, whole scg_multiplex"].append(time.perf_counter() - t0)
        assert upd[0].value == updated and upd[1].value == updated, (upd[0].value, upd[1].value, updated)
        L.refx_ra_destroy(v)
        L.refx_scg_destroy(g)
    for name, t in ts.items():
        print("  %-30s %9.1f ms   (%s)" % (name, 1e3 * statistics.median(t), ", ".join("%.1f" % (1e3 * x) for x in t)), flush=True)
    print("  updated = %d in all three" % updated)
    L.refx_scmdb_destroy(scm)
    L.refx_srdb_destroy(db)
    hip.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else synth.CONFIG1S["n_reads"])
