"""Child process of tests/test_gpu_devmem_balance.py: the smallest pipeline that touches every state struct smoke() touches (scan, count, EC graph, correction,
assembly graph, read alignment), one batch assembled from two 32-read handles (so that buffers grow and keep what they hold), and every handle closed.
With OATK_DEBUG_ALLOC_LOG=1 the library writes each hipMalloc and hipFree to stderr; the parent compares the two."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np

import align_util as AU
from oatk_amd import HipSyncasm
from oatk_amd.synth import ReadSet

K, S, C = 1001, 31, 4
rs = ReadSet(genome_len=60_000, n_reads=64, mean_len=12_000)
seq, off, lens = rs.slice(0, 64, threads=4)
hip = HipSyncasm(0)
hip.scan_host(seq, off, lens, K, S)
hip.count()
hip.ec_graph()
hip.ec(0.02, C, 0.35)
nv2, na2 = hip.asm_graph(C, 0.35)
ag = hip.fetch_asm_graph()
nv = len(ag["scm_del"])
su_off = np.zeros(nv + 1, np.uint64)
su_off[1:] = np.cumsum(ag["scm_del"] == 0)
graph = {"n_scm": nv, "su_off": su_off, "su_uid": np.arange(nv2, dtype=np.uint64) << np.uint64(1), "su_pos": np.zeros(nv2, np.uint32),
         "utg_n": np.ones(nv2, np.uint32), "idx_p": ag["idx_p"], "idx_n": ag["idx_n"].astype(np.uint64), "arc_w": ag["arc_w"],
         "arc_ln": np.zeros(na2, np.uint64), "arc_del": np.zeros(na2, np.uint8)}
ra = AU.device_align(hip, graph)
assert len(ra["sid"]) > 0

piece, main = HipSyncasm(0), HipSyncasm(0)
main.scan_begin(K, S)
for first in (0, 32):
    sq, of, ln = rs.slice(first, 32, threads=4)
    piece.scan_host(sq, of, ln, K, S, sid0=first)
    main.scan_append(piece)
assert main.info()["n_reads"] == 64
main.count()
for h in (piece, main, hip):
    h.close()
print("closed: %d reads, %d alignments" % (len(lens), len(ra["sid"])))
