"""GPU: the streamed reader with BGZF members inflated on the device (oatk_host_set_device_inflate / OATK_DEVICE_INFLATE; host/ingest_host.c: uploader_src).
oatk_sr_read_files with the switch on leaves the sr_db_t it leaves with the switch off -- every array of every read and every name -- and both equal the compiled
reference's sr_read of the same files: a BGZF file, a BGZF file followed by a plain .gz one, a file whose first half is BGZF members and whose second half is one
plain member, BGZF FASTQ with CRLF, a file that ends without a newline; windows forced small so that members, records and windows cut each other every way; one
handle and two handles on one GPU.  So that a silent fallback cannot pass, the counters must show members inflated on the device and none inflated again on the host.
A damaged member gives the switch-off return code and message (the host path judges the file); the -D cap takes the same last read; the drop-in CLI with
OATK_DEVICE_INFLATE=1 writes the reference binary's GFA files."""
import ctypes as C
import filecmp
import gzip
import os
import re

import numpy as np
import pytest

import adversarial as A
import bgzf_util as B
import cli_util as U
import ref_lib as R
from oatk_amd import _lib, bgzf_index, inflate_counts, pack_reads, set_device_inflate, synth
from test_gpu_ingest import fasta, fastq

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")]

K, S = 301, 21
READS = A.hifi_like(90, 30000, 4000, seed=29) + [b"acgtnACGTN" * 60, b"A" * 900 + A.rand_dna(np.random.default_rng(2), 700), b"C"]


def bgzf_bytes(text, seed, lo=300, hi=9000, eof=True, eof_inside=True):
    """the text as BGZF members of lo .. hi bytes of text each (some stored, most deflated), bgzip's end marker in the middle and at the end"""
    rng = np.random.default_rng(seed)
    out, at, k = [], 0, 0
    while at < len(text):
        n = int(rng.integers(lo, hi))
        t = text[at:at + n]
        out.append(B.member(B.raw_deflate(t, (6, 1, 9, 0)[k % 4]), t))
        at, k = at + n, k + 1
        if eof_inside and k == 7:
            out.append(B.EOF_MARKER)
    if eof:
        out.append(B.EOF_MARKER)
    return b"".join(out)


def make_inputs(tmp_path, case):
    p = lambda name: str(tmp_path / name)      # noqa: E731
    a, b = READS[:50], READS[50:]
    if case == "bgzf":
        open(p("a.fa.gz"), "wb").write(bgzf_bytes(fasta(READS, 70), 1))
        return [p("a.fa.gz")]
    if case == "bgzf_then_plain_gz":
        open(p("a.fa.gz"), "wb").write(bgzf_bytes(fasta(a, 0), 2))
        gzip.open(p("b.fa.gz"), "wb").write(fasta(b, 61))
        return [p("a.fa.gz"), p("b.fa.gz")]
    if case == "half_bgzf_half_plain_member":
        t = fasta(READS, 80)
        cut = len(t) // 2 + 17
        open(p("a.fa.gz"), "wb").write(bgzf_bytes(t[:cut], 3, eof=False, eof_inside=False) + gzip.compress(t[cut:]))
        return [p("a.fa.gz")]
    if case == "bgzf_fastq_crlf":
        open(p("a.fq.gz"), "wb").write(bgzf_bytes(fastq(READS, b"\r\n"), 4))
        return [p("a.fq.gz")]
    if case == "no_last_newline":
        open(p("a.fa.gz"), "wb").write(bgzf_bytes(fasta(a, 70, last_eol=False), 5))
        open(p("b.fa.gz"), "wb").write(bgzf_bytes(fasta(b, 0, last_eol=False), 6, eof=False))
        return [p("a.fa.gz"), p("b.fa.gz")]
    raise KeyError(case)


def host():
    H = _lib.load_host()
    H.oatk_sr_read_files.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p), C.c_int]
    H.oatk_sr_read_files_capped.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.c_uint64]
    H.oatk_host_set_threads.argtypes = [C.c_int]
    return H


def read_files(hip, files, window, on, handles=1, m_data=0):
    """oatk_sr_read_files over `handles` handles -> (rc, flattened sr_db_t, names, what the inflate counters moved by)"""
    H, L = host(), R.lib()
    L.refx_srdb_name.restype = C.c_char_p
    L.refx_srdb_name.argtypes = [C.c_void_p, C.c_uint64]
    db = H.oatk_sr_db_new(K, S)
    m = H.oatk_multi_create((C.c_int * handles)(*([hip.device] * handles)), handles) if handles > 1 else None
    assert handles == 1 or m
    set_device_inflate(on)
    c0 = inflate_counts()
    H.oatk_host_debug_window(window)
    H.oatk_host_set_threads(5)
    try:
        if m:
            rc = H.oatk_multi_sr_read_files(m, db, R._files_arg(files), len(files))
        elif m_data:
            rc = H.oatk_sr_read_files_capped(hip.h, db, R._files_arg(files), len(files), m_data)
        else:
            rc = H.oatk_sr_read_files(hip.h, db, R._files_arg(files), len(files))
    finally:
        H.oatk_host_debug_window(0)
        H.oatk_host_set_threads(0)
        set_device_inflate(False)
        if m:
            H.oatk_multi_destroy(m)
    moved = tuple(b - a for a, b in zip(c0, inflate_counts()))
    w = R.SrDb.__new__(R.SrDb)
    w.K, w.S, w._h = K, S, db
    flat, names = (w.flatten(), [L.refx_srdb_name(db, i) for i in range(w.n())]) if rc == 0 else (None, None)
    if rc == 0:                                                     # (a read that failed leaves its sr_db_t to the caller as it is: not looked into here)
        w.close()
    return rc, flat, names, moved


FIELDS = ["hoco_l", "n_scm", "sid", "hoco_s", "ho_rl", "ho_l_rl", "m_pos", "s_mer", "k_mer"]


def same_db(a, b, what):
    for f in FIELDS:
        assert np.array_equal(a[f], b[f]), (what, f)


CASES = ["bgzf", "bgzf_then_plain_gz", "half_bgzf_half_plain_member", "bgzf_fastq_crlf", "no_last_newline"]


@pytest.mark.parametrize("case,window,handles", [(c, w, 1) for c in CASES for w in (5000, 40000, 333333)] + [(c, 40000, 2) for c in CASES])
def test_switch_on_equals_switch_off_equals_the_reference(hip, tmp_path, case, window, handles):
    files = make_inputs(tmp_path, case)
    ref = R.SrDb(files, K, S, 2)
    want = ref.flatten()
    L = R.lib()
    L.refx_srdb_name.restype = C.c_char_p
    L.refx_srdb_name.argtypes = [C.c_void_p, C.c_uint64]
    want_names = [L.refx_srdb_name(ref.handle, i) for i in range(ref.n())]
    assert ref.n() == len(READS)
    ref.close()
    rc0, off, names0, moved0 = read_files(hip, files, window, False, handles)
    rc1, on, names1, moved1 = read_files(hip, files, window, True, handles)
    assert rc0 == 0 and rc1 == 0
    assert moved0 == (0, 0, 0)                                      # the switch is off: nothing went the new way
    same_db(on, off, "switch on against switch off")
    same_db(on, want, "switch on against the reference's sr_read")
    assert names1 == names0 == want_names
    assert moved1[0] > 0 and moved1[1] == 0 and moved1[2] > 0, moved1      # members on the device, none again on the host


@pytest.mark.parametrize("window", [40000, 333333])
def test_every_member_goes_to_the_device_not_only_those_of_the_first_window(hip, tmp_path, window):
    """No member of this file holds more than 9000 bytes of text and no record is longer than a window, so every member with text fits a window whole: all of
    them are the device's, and every window (none holds more than `window` bytes) has text from there.  A window that ends inside a member leaves that member to
    the host; a reader that then stays on the host path for the rest of the file still shows members on the device > 0, which is why this asks for all of them."""
    files = make_inputs(tmp_path, "bgzf")
    members, n_text, n_comp = bgzf_index(open(files[0], "rb").read())
    assert n_comp == os.path.getsize(files[0])
    with_text = int(np.count_nonzero(members["out_len"]))
    assert with_text > 40
    rc, _, names, moved = read_files(hip, files, window, True)
    assert rc == 0 and len(names) == len(READS)
    assert with_text <= moved[0] <= len(members) and moved[1] == 0 and moved[2] >= n_text // window, (moved, with_text, len(members))


def test_a_damaged_member_is_judged_by_the_host_path(hip, tmp_path, capfd):
    t = fasta(READS, 70)
    good = bgzf_bytes(t, 7, eof_inside=False)
    members, _, n_comp = bgzf_index(good)
    assert n_comp == len(good) and len(members) > 20
    mid = members[len(members) // 2]
    bad = bytearray(good)
    bad[int(mid["in_off"]) + int(mid["in_len"]) // 2] ^= 0x5A     # a byte in the middle of the middle member's deflate stream
    path = str(tmp_path / "bad.fa.gz")
    open(path, "wb").write(bytes(bad))
    with pytest.raises(Exception):
        gzip.decompress(bytes(bad))
    capfd.readouterr()
    rc0, _, _, moved0 = read_files(hip, [path], 40000, False)
    msg0 = capfd.readouterr().err
    rc1, _, _, moved1 = read_files(hip, [path], 40000, True)
    msg1 = capfd.readouterr().err
    assert rc0 != 0 and rc1 == rc0
    assert "is damaged" in msg0 and [ln for ln in msg1.splitlines() if "[E::" in ln] == [ln for ln in msg0.splitlines() if "[E::" in ln]
    assert moved0 == (0, 0, 0) and moved1[1] > 0                    # the window with the bad member was inflated again on the host


def test_the_data_cap_takes_the_same_last_read(hip, tmp_path):
    files = make_inputs(tmp_path, "bgzf")
    cap = sum(len(r) for r in READS[:37]) - 5                       # the 37th read takes the total to the cap
    rc0, off, names0, _ = read_files(hip, files, 40000, False, m_data=cap)
    rc1, on, names1, moved = read_files(hip, files, 40000, True, m_data=cap)
    assert rc0 == 0 and rc1 == 0 and len(names0) == 37 and names1 == names0
    same_db(on, off, "capped")
    assert moved[0] > 0 and moved[1] == 0


@pytest.mark.skipif(not U.available(), reason="oracle/_ref CLI binaries not built")
def test_cli_with_the_environment_switch(tmp_path):
    reads = A.hifi_like(300, 50000, 5000, seed=14, err=0.0008)
    seq, off, lens = pack_reads(reads)
    fa = str(tmp_path / "reads.fa.gz")
    synth.write_fasta(fa, seq, off, lens, mode=synth.FA_BGZF)
    ref, dev = str(tmp_path / "ref"), str(tmp_path / "dev")
    U.run_cli(U.CLI_REF, fa, ref, 301, 6, 4, extra=["-s", "21"])
    _, err = U.run_cli(U.CLI_DROPIN, fa, dev, 301, 6, 4, env={"OATK_DROPIN_LOG": "1", "OATK_DEVICE_INFLATE": "1", "OATK_DEBUG_WINDOW": "400000"}, extra=["-s", "21"])
    for suffix in (".utg.gfa", ".utg.final.gfa"):
        assert os.path.getsize(ref + suffix) > 100 and filecmp.cmp(ref + suffix, dev + suffix, shallow=False), suffix
    tab = U.served_table(err)
    assert tab["sr_read"][0] == 1 and tab["sr_read"][2] == 0, tab["sr_read"]
    m = re.search(r"oatk_sr_read_files\].*inflated on the device so far: (\d+) members, (\d+) redone on the host, (\d+) windows", err)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) == 0 and int(m.group(3)) > 0, err[-1500:]
