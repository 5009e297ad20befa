#!/usr/bin/env python3
"""What inflating BGZF input on the device costs and buys (include/oatk_hip_ingest.h: oatk_hip_inflate_bgzf; include/oatk_inflate.h: the reader's switch; DESIGN.md
11), for the record.  Input: config-2-sized reads (oatk_amd.synth CONFIGS: 200 k x 15 kb) written once as BGZF FASTA with synth.write_fasta, 16 host threads.
  (a) the kernel alone, compressed bytes resident: GB/s of text of oatk_hip_inflate_bgzf (inflate and CRC are one kernel), median and range of 3 after a warm-up;
  (b) oatk_sr_read_files with the structs filled, the reader's switch off and on ALTERNATED in one session, 3 runs each, median and range.  The yardstick is the
      switch-off path -- the code as it was before the switch existed.  A difference is called real only if the medians differ by more than twice the larger range
      (the rule of DESIGN.md 7); the result is printed either way.
Every sample is a process of its own under its own time limit; the first one that fails ends the script.  Development aid, not a test.
usage: python tests/inflate_time.py [n_reads] [output file]"""
import ctypes as C
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, S, THREADS = 1001, 31, 16


def step_make(path, n_reads):
    from oatk_amd import synth
    cfg = dict(synth.CONFIGS["config2"])
    cfg["n_reads"] = n_reads
    rs = synth.ReadSet(**cfg)
    seq, off, lens = rs.slice(0, n_reads, threads=THREADS)
    synth.write_fasta(path, seq, off, lens, mode=synth.FA_BGZF, threads=THREADS)
    print("made %s: %.1f MB of BGZF for %.2f Gbases" % (path, os.path.getsize(path) / 1e6, float(lens.sum()) / 1e9))


def step_kernel(path):
    from oatk_amd import HipSyncasm, bgzf_index
    data = np.fromfile(path, np.uint8)
    members, n_text, n_comp = bgzf_index(data)
    assert n_comp == data.size
    hip = HipSyncasm(0)
    L = hip.L
    d_text = C.c_void_p()
    hip._check(L.oatk_hip_ingest_text_buffer(hip.h, n_text, C.byref(d_text)), "text buffer")
    other = HipSyncasm(0)                                # (its text buffer holds the compressed bytes: resident before the clock starts)
    d_comp = C.c_void_p()
    other._check(L.oatk_hip_ingest_text_buffer(other.h, data.size, C.byref(d_comp)), "comp buffer")
    L.oatk_hip_h2d_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    other._check(L.oatk_hip_h2d_async(other.h, d_comp, data.ctypes.data, data.size), "upload")
    other.sync()
    bad, ts = C.c_uint64(), []
    for i in range(4):
        t0 = time.perf_counter()
        hip._check(L.oatk_hip_inflate_bgzf(hip.h, d_comp, data.size, members.ctypes.data, len(members), d_text, n_text, C.byref(bad), None), "inflate")
        ts.append(time.perf_counter() - t0)
        assert bad.value == 0
    ts = ts[1:]
    print("kernel: %d members, %.3f GB of text from %.3f GB: median %.4f s (%.4f .. %.4f) = %.2f GB/s of text"
          % (len(members), n_text / 1e9, data.size / 1e9, statistics.median(ts), min(ts), max(ts), n_text / 1e9 / statistics.median(ts)))


def step_read(path, on):
    from oatk_amd import HipSyncasm, _lib, inflate_counts, set_device_inflate
    H = _lib.load_host()
    H.oatk_sr_read_files.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p), C.c_int]
    H.oatk_host_set_threads.argtypes = [C.c_int]
    H.oatk_host_set_threads(THREADS)
    hip = HipSyncasm(0)
    set_device_inflate(on)
    db = H.oatk_sr_db_new(K, S)
    files = (C.c_char_p * 1)(path.encode())
    t0 = time.perf_counter()
    rc = H.oatk_sr_read_files(hip.h, db, files, 1)
    dt = time.perf_counter() - t0
    assert rc == 0, hip.L.oatk_hip_last_error(hip.h)
    print("sr_read switch=%s: %.4f s, counters %s" % ("on" if on else "off", dt, inflate_counts()))


def child(args, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit)
    sys.stdout.write(r.stdout)
    if r.returncode != 0:
        sys.stdout.write(r.stderr[-2000:])
        raise SystemExit("step %s failed with %d: stopping" % (args[0], r.returncode))
    return r.stdout


def main():
    if len(sys.argv) > 1 and sys.argv[1].startswith("--"):
        step = sys.argv[1]
        if step == "--make":
            step_make(sys.argv[2], int(sys.argv[3]))
        elif step == "--kernel":
            step_kernel(sys.argv[2])
        elif step == "--read":
            step_read(sys.argv[2], sys.argv[3] == "on")
        return
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    out = sys.argv[2] if len(sys.argv) > 2 else None
    d = tempfile.mkdtemp(prefix="oatk_inflate_time_")
    path = os.path.join(d, "reads.fa.gz")
    log = []
    try:
        log.append(child(["--make", path, str(n_reads)], 900))
        log.append(child(["--kernel", path], 300))
        t = {"off": [], "on": []}
        for _ in range(3):
            for sw in ("off", "on"):
                o = child(["--read", path, sw], 300)
                log.append(o)
                t[sw].append(float(o.split(": ")[1].split(" s")[0]))
        med = {k: statistics.median(v) for k, v in t.items()}
        rng = {k: max(v) - min(v) for k, v in t.items()}
        real = abs(med["on"] - med["off"]) > 2 * max(rng.values())
        log.append("sr_read, structs filled, %d host threads: switch off median %.4f s (range %.4f), switch on median %.4f s (range %.4f): %s\n"
                   % (THREADS, med["off"], rng["off"], med["on"], rng["on"],
                      ("the device path is %s" % ("faster" if med["on"] < med["off"] else "slower")) if real else "no difference by the rule of twice the larger range"))
        sys.stdout.write(log[-1])
    finally:
        shutil.rmtree(d, ignore_errors=True)
        if out:
            with open(out, "w") as f:
                f.write("".join(log))


if __name__ == "__main__":
    main()
