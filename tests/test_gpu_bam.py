"""GPU: unaligned BAM read on the device (oatk_hip_ingest_bam: include/oatk_hip_ingest.h, oatk_amd/csrc/bam.hpp).  Two yardsticks: the plain-Python reading of the
same stream (tests/bam_util.py: offsets, names, letters), and the project's own FASTA path -- the same reads as FASTA text through ingest_host must leave the same
INGEST_OFF / INGEST_LEN and the same letters.  Every stream given to the device here has been through oatk_amd/csrc/bam_core.hpp on the CPU under ASan + UBSan first
(tests/test_host_bam_core.py)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import adversarial as A
import bam_util as U
from oatk_amd import OatkHipError, _lib

pytestmark = pytest.mark.gpu

E_ARG, E_STATE, E_SPLIT = 2, 3, 5


def resident(hip):
    seq, off, lens = hip.fetch("INGEST_SEQ"), hip.fetch("INGEST_OFF"), hip.fetch("INGEST_LEN")
    assert np.all(off % 64 == 0)
    return [seq[int(o):int(o) + int(l)].tobytes() for o, l in zip(off, lens)], off, lens


def check_against_both(hip, b, scan=None):
    """ingest the stream b whole; reads, names, header offsets against the oracle, OFF / LEN / letters against the FASTA path"""
    names, reads, recs = U.parse(b)
    n, used = hip.ingest_bam_host(b)
    assert (n, used) == (len(reads), len(b))
    got, off, lens = resident(hip)
    assert got == reads
    assert hip.fetch("INGEST_HDR").tolist() == recs
    assert hip.ingest_names(*hip.bam_text) == names
    st = hip.bam_stats()
    assert st["records"] == len(recs) and st["header_bytes"] == U.header_walk(b)[1] and st["candidates"] == len(U.candidates(b, st["header_bytes"]))
    bam_scan = None
    if scan:
        hip.scan_ingested(*scan)
        bam_scan = hip.fetch_scan(off)
    text = U.fasta(names, reads)
    assert hip.ingest_host(text, 1, True) == (len(reads), len(text))
    fa, fa_off, fa_lens = resident(hip)
    assert np.array_equal(fa_off, off) and np.array_equal(fa_lens, lens) and fa == got
    assert hip.fetch("INGEST_SEQ").size == sum((len(r) + 63) // 64 * 64 for r in reads)
    if scan:
        hip.scan_ingested(*scan)
        fa_scan = hip.fetch_scan(fa_off)
        assert sorted(fa_scan) == sorted(bam_scan)
        for k in fa_scan:
            assert fa_scan[k].dtype == bam_scan[k].dtype and fa_scan[k].tobytes() == bam_scan[k].tobytes(), k
    return st


@pytest.mark.parametrize("tags", [False, True], ids=["no_tags", "tags"])
@pytest.mark.parametrize("n_cigar", [0, 3])
def test_length_and_alignment_sweep(hip, tags, n_cigar):
    """every l_seq around the 16-letter group, the 64-byte padding and the 1024-base trip, with names of 1 .. 16 bytes so that the packed bases start at every offset
    modulo 16; quality bytes 0xFF; all sixteen codes at even and at odd positions"""
    rd = U.sweep_reads(tags, n_cigar)
    assert {len(r["seq"]) for r in rd} == set(U.SWEEP_LENS) and {len(r["name"]) for r in rd} == set(range(1, 17))
    for parity in (0, 1):
        assert {chr(c) for r in rd for c in r["seq"][parity::2]} == set(U.CODES)
    b = U.stream(rd)
    _, _, recs = U.parse(b)
    at = {(o + 36 + b[o + 12] + 4 * n_cigar) % 16 for o in recs}
    assert at == set(range(16))
    check_against_both(hip, b)


def test_hifi_like_reads_and_the_scan_behind_them(hip):
    reads = A.hifi_like(40, 20000, 3000, seed=11)
    rng = np.random.default_rng(2)
    b = U.stream([dict(name=b"m84/%d/ccs" % i, seq=r, qual=rng.integers(0, 94, len(r), dtype=np.uint8).tobytes(), tags=U.tag_int(b"np", i)) for i, r in enumerate(reads)],
                 refs=((b"chr1", 1000), (b"x", 5)))
    check_against_both(hip, b, scan=(1001, 31))


def test_false_candidates_from_integer_tags(hip):
    """zero bytes of integer tags in front of record starts look like records that begin a byte early: the candidate list is longer than the chain"""
    b = U.stream(U.short_reads_with_int_tags(300, 1))
    st = check_against_both(hip, b)
    assert st["candidates"] > st["records"] == 300


def test_fake_records_inside_tags(hip):
    """complete records inside B-type tags: two whose chain ends with the enclosing record and so rejoins the true chain, one in front of the first record's successor"""
    b = U.stream(U.nested_fake_records())
    st = check_against_both(hip, b)
    assert st["records"] == 4 and st["candidates"] >= 8


def test_chunked_stream_gives_the_same_reads(hip):
    rd = U.short_reads_with_int_tags(60, 6)
    b = U.stream(rd, text=b"@HD\tVN:1.6\tSO:unknown\n@PG\tID:ccs\tVN:6.4\n")
    names, reads, recs = U.parse(b)
    s0 = recs[0]

    def seq_at(j):
        return recs[j] + 36 + b[recs[j] + 12]
    rng = np.random.default_rng(8)
    cuts = set(rng.integers(1, len(b) - 1, 12).tolist())
    cuts |= {20, recs[5] + 2, recs[11] + 20, recs[17] + 36 + 3, seq_at(23) + 5, seq_at(29) + (len(reads[29]) + 1) // 2 + 9, recs[35]}
    cuts = sorted(cuts) + [len(b)]
    assert cuts[0] < s0                                             # the first chunk ends inside the header
    bounds = set(recs) | {len(b)}
    got, got_names, pos, carry, taken = [], [], 0, b"", 0          # taken: bytes of the stream the calls so far have consumed
    for c in cuts:
        chunk = carry + b[pos:c]
        final = c == len(b)
        n, used = hip.ingest_bam_host(chunk, header=taken == 0, final=final)
        if taken == 0 and len(chunk) < s0:
            assert (n, used) == (0, 0)                              # half a header: come back with more
        else:
            assert taken + used in bounds
        r, _, _ = resident(hip)
        assert len(r) == n
        got += r
        got_names += hip.ingest_names(*hip.bam_text)
        taken += used
        carry, pos = chunk[used:], c
    assert taken == len(b) and got == reads and got_names == names


def test_device_only_route_and_the_host_helper(hip, tmp_path):
    """compressed .bam bytes -> inflate_bgzf -> ingest_bam_device on the inflated bytes -> names and reads, no text on the host; the same file through
    oatk_ingest_files; two BAM files in one call are refused"""
    b = U.stream(U.short_reads_with_int_tags(500, 12))
    names, reads, recs = U.parse(b)
    data = U.bgzf(b, member_text=65536)
    assert len(b) > 2 * 65536 and all(o % 65536 for o in recs[1:])  # several members, and records span them
    text = hip.inflate_bgzf(data)
    assert text.tobytes() == b
    d_text, n_text = hip.inflated
    assert hip.ingest_bam_device(d_text, n_text, True, True) == (len(reads), len(b))
    assert resident(hip)[0] == reads and hip.ingest_names(d_text, n_text) == names
    H = _lib.load_host()
    H.oatk_ingest_files.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_uint64)]
    p1, p2 = str(tmp_path / "a.hifi_reads.bam"), str(tmp_path / "b.hifi_reads.bam")
    open(p1, "wb").write(data)
    open(p2, "wb").write(U.bgzf(U.stream(U.sweep_reads(True, 0)[:50])))
    n = C.c_uint64()
    assert H.oatk_ingest_files(hip.h, (C.c_char_p * 1)(p1.encode()), 1, C.byref(n)) == 0 and n.value == len(reads)
    assert resident(hip)[0] == reads
    assert H.oatk_ingest_files(hip.h, (C.c_char_p * 2)(p1.encode(), p2.encode()), 2, C.byref(n)) == E_ARG
    fa = str(tmp_path / "c.fa")
    open(fa, "wb").write(U.fasta(names[:9], reads[:9]))
    assert H.oatk_ingest_files(hip.h, (C.c_char_p * 2)(fa.encode(), p2.encode()), 2, C.byref(n)) == E_ARG
    assert H.oatk_ingest_files(hip.h, (C.c_char_p * 1)(fa.encode()), 1, C.byref(n)) == 0 and n.value == 9      # other input goes the way it went


@pytest.mark.parametrize("case", sorted(U.damage_cases()))
def test_refusals_and_damage(hip, case):
    b, want = U.damage_cases()[case]
    with pytest.raises(OatkHipError) as e:
        hip.ingest_bam_host(b)
    code = int(re.search(r"code (\d+)", str(e.value)).group(1))
    assert code == (E_ARG if want == "arg" else E_SPLIT), str(e.value)
    with pytest.raises(OatkHipError, match="code %d" % E_STATE):
        hip.fetch("INGEST_SEQ")
    good = U.stream(U.sweep_reads(True, 0)[100:140])
    assert hip.ingest_bam_host(good)[0] == 40 and resident(hip)[0] == U.parse(good)[1]


def test_a_cut_record_is_left_for_the_next_chunk_and_truncate_keeps_the_first_reads(hip):
    b = U.stream(U.sweep_reads(False, 0)[200:260])
    names, reads, recs = U.parse(b)
    n, used = hip.ingest_bam_host(b[:recs[41] + 3], final=False)
    assert (n, used) == (41, recs[41])
    hip.L.oatk_hip_ingest_truncate.argtypes = [C.c_void_p, C.c_uint64]      # (no argtypes in _lib: without them the handle would go as a C int)
    hip._check(hip.L.oatk_hip_ingest_truncate(hip.h, 17), "oatk_hip_ingest_truncate")
    assert resident(hip)[0] == reads[:17] and hip.ingest_names(*hip.bam_text) == names[:17]


def test_fasta_after_bam_on_the_same_context(hip):
    """the text formats are untouched: after a BAM ingest, FASTA text and its names come out as before"""
    names = [b"read%d" % i for i in range(30)]
    reads = A.hifi_like(30, 8000, 700, seed=3)
    text = b"".join(b">" + n + b" some comment\n" + r[:300] + b"\n" + r[300:] + b"\n" for n, r in zip(names, reads))
    hip.ingest_bam_host(U.stream(U.nested_fake_records()))
    assert hip.ingest_host(text, 0, True) == (30, len(text))
    assert resident(hip)[0] == reads
    d = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:%d" % hip.device)
    torch.cuda.synchronize()
    assert hip.ingest_device(d.data_ptr(), len(text), 1, True)[0] == 30
    assert hip.ingest_names(d.data_ptr(), len(text)) == names
