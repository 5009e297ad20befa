#!/usr/bin/env python3
"""What reading unaligned BAM on the device costs (include/oatk_hip_ingest.h: oatk_hip_ingest_bam), for the record.  Input: config-2-sized reads
(oatk_amd.synth CONFIGS: 200 k x 15 kb) written once as an inflated BAM stream (random quality, one integer tag per record) and once as FASTA text, each resident
on the device before the clock starts.
  (a) oatk_hip_ingest_bam: the whole call, and with oatk_hip_set_timing on the phases from HIP events on the call's stream -- candidate passes, successors + doubling
      rounds, compaction + stop, record kernel + offsets scan, unpack kernel; medians of 5 after a warm-up.  The unpack kernel also as bytes read + written per second.
  (b) oatk_hip_ingest of the same reads as FASTA, same build, same process: the yardstick; median of 5 after a warm-up.
No counters are taken.  The measurement is a process of its own under a time limit.  Development aid, not a test; run it under tools/memcap.py.
usage: python tests/bam_time.py [n_reads] [output file]"""
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
THREADS = 16
PHASES = ["candidate passes", "successors + doubling", "compaction + stop", "record kernel + scan", "unpack kernel"]


def make(n_reads):
    """(inflated BAM stream, FASTA text, bases) of the same reads, by numpy: a loop over reads that only copies slices"""
    from oatk_amd import synth
    cfg = dict(synth.CONFIGS["config2"])
    cfg["n_reads"] = n_reads
    seq, off, lens = synth.ReadSet(**cfg).slice(0, n_reads, threads=THREADS)
    off, lens = off.astype(np.int64), lens.astype(np.int64)
    lut = np.zeros(256, np.uint8)
    for i, c in enumerate(b"=ACMGRSVTWYHKDBN"):
        lut[c] = i
    codes = lut[seq[:(len(seq) // 2) * 2]]
    packed = (codes[0::2] << 4) | codes[1::2]                   # every read starts on an even offset of the slab: its pairs are the slab's
    del codes
    text = b"@HD\tVN:1.6\tSO:unknown\n"
    head = b"BAM\x01" + len(text).to_bytes(4, "little") + text + (0).to_bytes(4, "little")
    name_len, tag = 11, 7                                       # "r%09d" + NUL; "npi" + i32
    nb = (lens + 1) // 2
    size = 36 + name_len + nb + lens + tag
    at = len(head) + np.concatenate([[0], np.cumsum(size)[:-1]])
    bam = np.zeros(len(head) + int(size.sum()), np.uint8)
    bam[:len(head)] = np.frombuffer(head, np.uint8)
    fixed = np.zeros(n_reads, np.dtype([("bs", "<i4"), ("ref", "<i4"), ("pos", "<i4"), ("lrn", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("ncig", "<u2"), ("flag", "<u2"),
                                        ("lseq", "<u4"), ("nref", "<i4"), ("npos", "<i4"), ("tlen", "<i4")]))
    fixed["bs"], fixed["ref"], fixed["pos"], fixed["lrn"], fixed["mapq"], fixed["bin"], fixed["flag"], fixed["lseq"] = size - 4, -1, -1, name_len, 255, 4680, 4, lens
    fixed["nref"], fixed["npos"] = -1, -1
    fixed = fixed.view(np.uint8).reshape(n_reads, 36)
    rng = np.random.default_rng(1)
    qual = rng.integers(0, 94, 1 << 26, dtype=np.uint8)
    fa_at = np.concatenate([[0], np.cumsum(lens + name_len + 2)[:-1]])
    fa = np.full(int((lens + name_len + 2).sum()), 10, np.uint8)
    for i in range(n_reads):
        a, ln, o = int(at[i]), int(lens[i]), int(off[i])
        nm = np.frombuffer(b"r%09d" % i, np.uint8)
        bam[a:a + 36] = fixed[i]
        bam[a + 36:a + 46] = nm
        p = a + 36 + name_len
        bam[p:p + int(nb[i])] = packed[o // 2:o // 2 + int(nb[i])]
        if ln & 1:
            bam[p + int(nb[i]) - 1] &= 0xF0
        q = int(rng.integers(0, len(qual) - ln))
        bam[p + int(nb[i]):p + int(nb[i]) + ln] = qual[q:q + ln]
        t = p + int(nb[i]) + ln
        bam[t:t + 3] = (110, 112, 105)                          # "npi"
        bam[t + 3] = 5 + i % 20
        f = int(fa_at[i])
        fa[f] = 62
        fa[f + 1:f + 11] = nm
        fa[f + 12:f + 12 + ln] = seq[o:o + ln]
    return bam, fa, int(lens.sum())


def resident(hip, data):
    d = C.c_void_p()
    hip._check(hip.L.oatk_hip_ingest_text_buffer(hip.h, data.size, C.byref(d)), "text buffer")
    hip.L.oatk_hip_h2d_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    hip._check(hip.L.oatk_hip_h2d_async(hip.h, d, data.ctypes.data, data.size), "upload")
    hip.sync()
    return d.value


def measure(n_reads):
    from oatk_amd import HipSyncasm
    t0 = time.perf_counter()
    bam, fa, bases = make(n_reads)
    print("made %d reads, %.3f Gbases: %.3f GB of BAM stream, %.3f GB of FASTA text (%.1f s)" % (n_reads, bases / 1e9, bam.size / 1e9, fa.size / 1e9, time.perf_counter() - t0))
    hip = HipSyncasm(0)
    d = resident(hip, bam)
    whole, phases = [], []
    for i in range(12):                                         # warm-up, then 5 calls as they are and 5 with the phase events
        timed = i >= 7
        hip.set_timing(timed)
        t0 = time.perf_counter()
        n, used = hip.ingest_bam_device(d, bam.size, True, True)
        dt = time.perf_counter() - t0
        assert (n, used) == (n_reads, bam.size)
        if 2 <= i < 7:
            whole.append(dt)
        if timed:
            ms = (C.c_float * 5)()
            hip._check(hip.L.oatk_hip_ingest_bam_times(hip.h, ms), "times")
            phases.append([float(x) for x in ms])
    hip.set_timing(False)
    st = hip.bam_stats()
    seq_bam = hip.fetch("INGEST_LEN")
    med = statistics.median(whole)
    print("oatk_hip_ingest_bam, resident: %d candidates for %d records; median %.4f s (%.4f .. %.4f) = %.2f Gbases/s" % (st["candidates"], st["records"], med, min(whole), max(whole), bases / 1e9 / med))
    for k, name in enumerate(PHASES):
        v = [p[k] for p in phases]
        extra = ""
        if k == 4:
            moved = float(((seq_bam.astype(np.int64) + 1) // 2).sum() + bases)
            extra = " = %.2f TB/s of bytes read + written (%.0f%% of the 6.3 TB/s the guides give as achievable)" % (moved / 1e12 / (statistics.median(v) / 1e3), 100 * moved / 1e12 / (statistics.median(v) / 1e3) / 6.3)
        print("  %-24s median %9.3f ms (%.3f .. %.3f)%s" % (name, statistics.median(v), min(v), max(v), extra))
    d = resident(hip, fa)
    ts = []
    for i in range(7):
        t0 = time.perf_counter()
        n, used = hip.ingest_device(d, fa.size, 1, True)
        ts.append(time.perf_counter() - t0)
        assert (n, used) == (n_reads, fa.size)
    ts = ts[2:]
    assert np.array_equal(hip.fetch("INGEST_LEN"), seq_bam)
    fmed = statistics.median(ts)
    print("oatk_hip_ingest (FASTA, one line per read), resident: median %.4f s (%.4f .. %.4f) = %.2f Gbases/s" % (fmed, min(ts), max(ts), bases / 1e9 / fmed))
    print("BAM / FASTA per base: %.2f" % (med / fmed))
    hip.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--measure":
        measure(int(sys.argv[2]))
        return
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    out = sys.argv[2] if len(sys.argv) > 2 else None
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure", str(n_reads)], capture_output=True, text=True, timeout=900)
    sys.stdout.write(r.stdout)
    if out:
        with open(out, "w") as f:
            f.write(r.stdout)
    if r.returncode != 0:
        sys.stdout.write(r.stderr[-2000:])
        raise SystemExit("the measurement failed with %d" % r.returncode)


if __name__ == "__main__":
    main()
