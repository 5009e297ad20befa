#!/usr/bin/env python3
"""Wall clock of the coverage estimates from read alignments over several handles at run_syncasm.c:295-297: the N-handle pair
(oatk_multi_scg_ra_utg_coverage + oatk_multi_scg_ra_arc_coverage + the reference's scg_refine_arc_coverage) with 1, 2 and 4 handles on one
GPU, next to two one-handle figures of the same session -- the resident pair, and the uploaded pair, which is what an N-handle caller had to
use before -- the median of 3 each, after checking that every vtx[].cov and arc[].cov equals the compiled reference's.  Like
tests/racov_time.py the state is the real one: config-3 reads (oatk_amd.synth CONFIGS) written to a FASTA file (oatk_multi reads files: 15 kB
per read in the temporary directory, 30 GB at 2 M reads), scan, count, EC and assembly graph on the device(s), the reference's tail with the
alignments on the device(s), stopped at :295.  On one GPU the handles share the card: the figure of interest is the cost of the chain, the
N-handle time minus the one-handle resident time, and how it moves with N and with the EM's pass count (printed).
Needs oracle/_ref (built where the reference sources exist).  Development aid.
usage: python tests/racov_sharded_time.py [n_reads ...]      (default: 200000 2000000)"""
import ctypes as C
import os
import shutil
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
H = _lib.load_host()
H.oatk_sr_read_files.argtypes = [vp, vp, C.POINTER(C.c_char_p), C.c_int]
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


def em_passes(db, v, g):
    """the EM's pass count of this state, from the reference's own line (verbose 3)"""
    import re
    snap = covs(g)
    r, w = os.pipe()
    sys.stderr.flush()
    old = os.dup(2)
    os.dup2(w, 2)
    try:
        L.scg_ra_utg_coverage(g, db, v, 3)
    finally:
        os.dup2(old, 2)
        os.close(old), os.close(w)
    text = b""
    while True:
        chunk = os.read(r, 1 << 16)
        if not chunk:
            break
        text += chunk
    os.close(r)
    restore(g, snap)
    m = re.search(rb"ended at iteration (\d+)", text)
    return min(int(m.group(1)) + 1, 1000) if m else None


def measure(pairs, db, v, g):
    """pairs: [(name, fn)]; the reference first.  Every fn leaves vtx[].cov / arc[].cov; all must agree"""
    a = C.cast(g, C.POINTER(Scg)).contents.utg_asmg.contents
    snap = covs(g)
    out = {}

    def ref():
        L.scg_ra_utg_coverage(g, db, v, 0)
        L.scg_ra_arc_coverage(g, db, v, 1, 0)

    want = None
    for name, fn in [("reference", ref)] + pairs:
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
        print("  %-22s %9.1f ms   (%s)" % (name, 1e3 * out[name], ", ".join("%.1f" % (1e3 * t) for t in ts)), flush=True)
    restore(g, snap)
    out["passes"] = em_passes(db, v, g)
    print("  %d unitigs, %d arcs, %d alignment records, %s EM passes (the covs of all are identical)"
          % (a.n_vtx, a.n_arc, C.cast(v, C.POINTER(C.c_size_t))[0], out["passes"]), flush=True)
    return out


def tail_to_295(db, scm, asmg, cov, align, at_295):
    state = {"no_unzip": 0, "res": None}

    def aligner(db_, v, g, n_threads, for_unzip):
        align(db_, v, g, for_unzip)
        if for_unzip == 0:
            state["no_unzip"] += 1
            if state["no_unzip"] == 2:                     # :295, after the unzip rounds and the demultiplexing (:259)
                state["res"] = at_295(db_, v, g)

    cb = C.CFUNCTYPE(None, vp, vp, vp, C.c_int, C.c_int)(aligner)
    L.refx_set_aligner(cb)
    out = os.path.join(tempfile.mkdtemp(), "dev")
    assert L.refx_syncasm_tail_graph(db, scm, asmg, K, 100000, 10000, cov, 0.35, 0.3, 3, T, out.encode()) == 0
    L.refx_set_aligner(None)
    shutil.rmtree(os.path.dirname(out), ignore_errors=True)
    assert state["res"] is not None, "the tail never reached run_syncasm.c:295"
    return state["res"]


def one_handle(files, cov):
    hip = HipSyncasm(0)
    db = H.oatk_sr_db_new(K, S)
    assert H.oatk_sr_read_files(hip.h, db, files, 1) == 0, hip.L.oatk_hip_last_error(hip.h)
    rc = C.c_int(0)
    scm = H.oatk_collect_syncmer_from_reads(hip.h, db, C.byref(rc))
    st = np.zeros(12, np.uint64)
    assert H.oatk_read_error_correction(hip.h, db, scm, None, 0.02, cov, 10 * cov, cov, 0.35, st.ctypes.data) == 0
    asmg = H.oatk_make_syncmer_asmg(hip.h, scm, cov, 0.35, C.byref(rc))
    assert asmg and rc.value == 0

    def align(db_, v, g, for_unzip):
        nsk = C.c_uint64(0)
        assert H.oatk_scg_read_alignment(hip.h, db_, v, g, for_unzip, C.byref(nsk), None) == 0 and nsk.value == 0

    def dev(flags_u, flags_a, db_, v, g):
        def run():
            assert H.oatk_scg_ra_utg_coverage(hip.h, db_, v, g, flags_u, 0) == 0, hip.L.oatk_hip_last_error(hip.h)
            assert H.oatk_scg_ra_arc_coverage(hip.h, db_, v, g, flags_a, 0) == 0, hip.L.oatk_hip_last_error(hip.h)
            L.scg_refine_arc_coverage(g, 0)
        return run

    print(" one handle", flush=True)
    res = tail_to_295(db, scm, asmg, cov, align,
                      lambda db_, v, g: measure([("one handle, resident", dev(3, 2, db_, v, g)), ("one handle, uploaded", dev(0, 0, db_, v, g))], db_, v, g))
    L.refx_scmdb_destroy(scm)
    L.refx_srdb_destroy(db)
    hip.close()
    return res


def n_handles(files, cov, n):
    m = H.oatk_multi_create((C.c_int * n)(*([0] * n)), n)
    assert m
    err = lambda: H.oatk_multi_last_error(m)
    db = H.oatk_sr_db_new(K, S)
    assert H.oatk_multi_sr_read_files(m, db, files, 1) == 0, err()
    rc = C.c_int(0)
    scm = H.oatk_multi_collect_syncmer_from_reads(m, db, C.byref(rc))
    assert scm and rc.value == 0, err()
    st = np.zeros(12, np.uint64)
    assert H.oatk_multi_read_error_correction(m, db, scm, 0.02, cov, 10 * cov, cov, 0.35, st.ctypes.data) == 0, err()
    asmg = H.oatk_multi_make_syncmer_asmg(m, scm, cov, 0.35, C.byref(rc))
    assert asmg and rc.value == 0, err()

    def align(db_, v, g, for_unzip):
        nsk = C.c_uint64(0)
        assert H.oatk_multi_scg_read_alignment(m, db_, v, g, for_unzip, C.byref(nsk)) == 0 and nsk.value == 0, err()

    def pair(db_, v, g):
        def run():
            assert H.oatk_multi_scg_ra_utg_coverage(m, db_, v, g, 0) == 0, err()
            assert H.oatk_multi_scg_ra_arc_coverage(m, db_, v, g, 0) == 0, err()
            L.scg_refine_arc_coverage(g, 0)
        return run

    print(" %d handle%s on one GPU (%s)" % (n, "" if n == 1 else "s", "the in-process communicator group"), flush=True)
    name = "%d handle%s, resident" % (n, "" if n == 1 else "s")
    res = tail_to_295(db, scm, asmg, cov, align, lambda db_, v, g: measure([(name, pair(db_, v, g))], db_, v, g))
    L.refx_scmdb_destroy(scm)
    L.refx_srdb_destroy(db)
    H.oatk_multi_destroy(m)
    return res[name], res["passes"]


def run(n):
    cfg = CONFIGS["config3"]
    cov = cfg["min_k_cov"]
    rs = ReadSet(cfg["genome_len"], n, cfg["mean_len"])
    tmp = tempfile.mkdtemp()
    fa = os.path.join(tmp, "reads.fa")
    bases = 0
    with open(fa, "wb") as f:                              # in pieces: the text of 2 M reads is 30 GB
        step = 20000
        for first in range(0, n, step):
            cnt = min(step, n - first)
            seq, off, lens = rs.slice(first, cnt, threads=16)
            bases += int(lens.sum())
            for i in range(cnt):
                f.write(b">r%d\n" % (first + i) + seq[int(off[i]):int(off[i]) + int(lens[i])].tobytes() + b"\n")
    print("%d reads, %.2f Gbases (config-3 shape)" % (n, bases / 1e9), flush=True)
    files = (C.c_char_p * 1)(fa.encode())
    try:
        one = one_handle(files, cov)
        rows = {k: n_handles(files, cov, k) for k in (1, 2, 4)}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    base = one["one handle, resident"]
    for k, (t, passes) in rows.items():
        print("  %d handle%s: %8.1f ms = one handle resident %+8.1f ms (the chain: %d EM passes x %d steps + %d steps for the arcs); uploaded one-handle pair %8.1f ms"
              % (k, " " if k == 1 else "s", 1e3 * t, 1e3 * (t - base), passes, k, k, 1e3 * one["one handle, uploaded"]), flush=True)
        if t > one["one handle, uploaded"]:
            print("  FINDING: the %d-handle pair is slower than the uploaded one-handle pair of this session" % k, flush=True)
    return one, rows


if __name__ == "__main__":
    sizes = [int(x) for x in sys.argv[1:]] or [200000, 2000000]
    for n_ in sizes:
        run(n_)
