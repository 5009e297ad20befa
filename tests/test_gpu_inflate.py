"""GPU: BGZF members inflated on the device (oatk_hip_inflate_bgzf, csrc/inflate.hpp) against Python's zlib.  Members are built here from raw deflate streams plus
bgzip's header and trailer (tests/bgzf_util.py, tests/gpu_inflate_cases.py), so every shape is exact: the end marker, stored members, ISIZE 65536, fixed-Huffman
members with overlapping copies, distance 32768, several blocks in a member, no distance codes, repeat codes across the literal/distance boundary; 1 to 300 members
in a call; a FASTA file written as BGZF, inflated and parsed where it lies; and a fixed list of damaged members, each among good ones, with the text buffer filled
with a sentinel beforehand: the bad member gets its status, the good ones their text, and nothing outside the members' own ranges changes.
(tests/test_host_inflate_core_fuzz.py has put the same streams, and a few thousand damaged ones, to the decoder on the CPU under ASan first.)
The shapes here are hand-picked: their overlapped copies have distances up to 8 and none of them mixes a stored run with Huffman blocks.  What the kernel alone
does -- copies at every distance and length, the edges of the 64-token batch, stored runs among tokens, the 16-byte phases, the CRC's pieces, many bad members in
one call -- is swept in tests/test_gpu_inflate_sweeps.py."""
import gzip
import zlib

import numpy as np
import pytest
import torch

import adversarial as A
import bgzf_util as B
import gpu_inflate_cases as G
from oatk_amd import OatkHipError, bgzf_index, pack_reads, synth

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 4096, 0xA5


def inflate_into_sentinel(hip, data, rows, shift=0):
    """the members inflated into the middle of a buffer of sentinel bytes; returns (n_bad, status, text region, True if both guards are untouched)"""
    cap = int(rows["out_off"][-1]) + int(rows["out_len"][-1]) if len(rows) else 0
    buf = torch.full((GUARD + shift + cap + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda:%d" % hip.device)
    torch.cuda.synchronize()
    n_bad, st = hip.inflate_members(data, rows, buf.data_ptr() + GUARD + shift, cap)
    h = buf.cpu().numpy()
    lo, hi = h[:GUARD + shift], h[GUARD + shift + cap:]
    return n_bad, st, h[GUARD + shift:GUARD + shift + cap], bool(np.all(lo == SENTINEL) and np.all(hi == SENTINEL) and len(hi) == GUARD)


@pytest.mark.parametrize("name", [s[0] for s in G.member_shapes()])
def test_member_shapes(hip, name):
    _, stream, text = next(s for s in G.member_shapes() if s[0] == name)
    data = B.member(stream, text)
    members, n_text, n_comp = bgzf_index(data)
    assert len(members) == 1 and n_text == len(text) and n_comp == len(data)
    assert hip.inflate_bgzf(data).tobytes() == text == zlib.decompressobj(-15).decompress(stream)
    n_bad, st, got, guards = inflate_into_sentinel(hip, data, members, shift=7)
    assert n_bad == 0 and list(st) == [0] and got.tobytes() == text and guards
    assert hip.L.oatk_hip_inflate_last_byte(hip.h) == (text[-1] if text else 0)


@pytest.mark.parametrize("n,eof_at", [(1, None), (63, 0), (64, 31), (65, 64), (300, 150), (300, 299)])
def test_many_members_in_one_call(hip, n, eof_at):
    rng = np.random.default_rng(n)
    texts = [b"" if i == eof_at else (G.acgt(int(rng.integers(1, 3000)), 1000 + i) if i % 3 else G.fasta_like(int(rng.integers(1, 9000)), 1000 + i)) for i in range(n)]
    ms = [B.EOF_MARKER if i == eof_at else B.member(B.raw_deflate(t, (1, 6, 9, 0)[i % 4]), t) for i, t in enumerate(texts)]
    data = b"".join(ms)
    want = b"".join(texts)
    assert gzip.decompress(data) == want
    members, n_text, n_comp = bgzf_index(data)
    assert len(members) == n and n_text == len(want) and n_comp == len(data)
    got, st = hip.inflate_bgzf(data, status=True)
    assert not st.any() and got.tobytes() == want
    last = [t for t in texts if t][-1]
    assert hip.L.oatk_hip_inflate_last_byte(hip.h) == last[-1]


def test_bgzf_fasta_inflated_and_parsed_on_the_device(hip, tmp_path):
    reads = A.hifi_like(40, 20000, 3000, seed=11)
    seq, off, lens = pack_reads(reads)
    path = str(tmp_path / "reads.fa.gz")
    synth.write_fasta(path, seq, off, lens, mode=synth.FA_BGZF)
    data = open(path, "rb").read()
    want = gzip.decompress(data)
    members, _, n_comp = bgzf_index(data)
    assert n_comp == len(data) and len(members) >= 3              # two members of text and bgzip's end marker, at the least
    text = hip.inflate_bgzf(data)
    assert text.tobytes() == want
    d_text, n_text = hip.inflated
    n, used = hip.ingest_device(d_text, n_text, 0, True)
    assert n == len(reads) and used == n_text
    dseq, doff, dlen = hip.fetch("INGEST_SEQ"), hip.fetch("INGEST_OFF"), hip.fetch("INGEST_LEN")
    got = [dseq[int(o):int(o) + int(l)].tobytes() for o, l in zip(doff, dlen)]
    hip.ingest_host(want, 0, True)
    hseq, hoff, hlen = hip.fetch("INGEST_SEQ"), hip.fetch("INGEST_OFF"), hip.fetch("INGEST_LEN")
    assert got == [hseq[int(o):int(o) + int(l)].tobytes() for o, l in zip(hoff, hlen)] == reads


@pytest.mark.parametrize("name", [c[0] for c in G.damage_cases()])
def test_damaged_member_among_good_ones(hip, name):
    _, bad, edit, expect = next(c for c in G.damage_cases() if c[0] == name)
    ms = [G.good_member(0), G.good_member(1), bad, G.good_member(2), B.EOF_MARKER]
    data, rows = B.table(ms)
    if edit:
        edit(rows[2:3])
    n_bad, st, got, guards = inflate_into_sentinel(hip, data, rows, shift=3)
    assert n_bad == 1 and list(st) == [0, 0, expect, 0, 0]
    assert guards
    for i, k in ((0, 0), (1, 1), (3, 2)):
        o = int(rows["out_off"][i])
        assert got[o:o + len(G.GOOD[k])].tobytes() == G.GOOD[k], i
    o, ln = int(rows["out_off"][2]), int(rows["out_len"][2])
    if expect != 3:                                     # a member that is no stream, or of another length, leaves its range as it was
        assert np.all(got[o:o + ln] == SENTINEL)
    if not edit:                                        # (a cut in_len has no file form)
        with pytest.raises(OatkHipError, match="member 2 "):
            hip.inflate_bgzf(data)


def test_a_table_that_does_not_fit_is_refused_before_launch(hip):
    data, rows = B.table([G.good_member(0), G.good_member(2)])
    cap = int(rows["out_off"][-1] + rows["out_len"][-1])
    buf = torch.full((cap + 64,), SENTINEL, dtype=torch.uint8, device="cuda:%d" % hip.device)
    torch.cuda.synchronize()

    def refused(edit, cap=cap, comp=data):
        r = rows.copy()
        edit(r)
        with pytest.raises(OatkHipError, match="code 2"):
            hip.inflate_members(comp, r, buf.data_ptr(), cap)
    refused(lambda r: r["in_len"].__setitem__(1, r["in_len"][1] + 9))                   # one byte past the compressed bytes (the last member's trailer is 8)
    refused(lambda r: r["in_len"].__setitem__(1, r["in_len"][1] + 1), comp=data[:-8])   # the same with the compressed bytes ending where the stream ends
    refused(lambda r: r["out_off"].__setitem__(1, r["out_off"][1] - 1))                 # overlaps the member before it
    refused(lambda r: r["out_len"].__setitem__(1, 65537))                               # larger than a BGZF member
    refused(lambda r: None, cap=cap - 1)                                                # past the text buffer
    refused(lambda r: r["in_off"].__setitem__(0, 1 << 63))
    assert np.all(buf.cpu().numpy() == SENTINEL)


@pytest.mark.parametrize("case", ["fasta", "fasta_crlf", "fastq", "fastq_crlf", "header_ends_the_text"])
def test_names_cut_on_the_device(hip, case):
    """oatk_hip_ingest_names against the names kseq_like (tests/test_gpu_ingest.py) cuts: comments behind a space or a tab, CRLF, an empty name, a name that runs
    to the end of the text"""
    from test_gpu_ingest import kseq_like
    eol = b"\r\n" if case.endswith("crlf") else b"\n"
    if case.startswith("fastq"):
        t = b"".join(b"@" + nm + eol + s + eol + b"+" + eol + b"I" * len(s) + eol
                     for nm, s in [(b"m84/1/ccs np=3", b"ACGT"), (b"q2\tcomment after a tab", b"GG"), (b"", b"ACG"), (b"a|b:c;d", b"T"), (b"last", b"ACGTACGT")])
    else:
        t = b"".join(b">" + nm + eol + s + eol for nm, s in [(b"r0 some comment", b"ACGT"), (b"r1\ttab comment", b"GGCC"), (b"", b"AC"), (b"x" * 300, b"T"), (b"r4", b"ACGT" * 50)])
        if case == "header_ends_the_text":
            t += b">the_very_end"
    want = [nm for nm, _ in kseq_like(t)]
    assert b"" in want and len(want) >= 5
    d = torch.frombuffer(bytearray(t), dtype=torch.uint8).to("cuda:%d" % hip.device)
    torch.cuda.synchronize()
    n, used = hip.ingest_device(d.data_ptr(), len(t), 0, True)
    assert n == len(want) and used == len(t)
    assert hip.ingest_names(d.data_ptr(), len(t)) == want
