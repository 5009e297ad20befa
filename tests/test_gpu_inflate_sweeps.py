"""GPU: what only the kernel of csrc/inflate.hpp does -- batches of 64 tokens executed wave-wide, overlapped copies from[j % a], stored runs copied from the staged
input, the 16-byte phases of staging and write-out, the CRC in 64 pieces of 1 KiB, the count of bad members and the last byte -- swept instead of sampled.  The
members are written token by token (tests/gpu_inflate_cases.py), every expected text is zlib's inflate of the stream AND a byte-by-byte LZ77 model of the tokens
(the two agree before anything is launched; tests/test_host_inflate_core_fuzz.py has put every stream to the decoder core on the CPU), and everything is compared
byte for byte.  tests/test_inflate_case_lists.py asserts what the lists cover: every distance 1..520 with every length 3..258, a match and a stored run at every
place of the batch, a stored header at every bit offset.  Each test is one launch, or a handful."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import bgzf_util as B
import gpu_inflate_cases as G
from oatk_amd import _lib, bgzf_index
from test_gpu_inflate import GUARD, SENTINEL, inflate_into_sentinel

pytestmark = pytest.mark.gpu


def where_it_went_wrong(name, got, text):
    """the first differing offset of a member and the token it falls in, from the member's token list"""
    got, want = np.frombuffer(got, np.uint8), np.frombuffer(text, np.uint8)
    at = int(np.flatnonzero(got != want)[0])
    msg = "member %s: first wrong byte at offset %d of %d (0x%02x, expected 0x%02x)" % (name, at, len(text), got[at], want[at])
    for i, kind, o, ln, d in B.walk_blocks(G.BLOCKS.get(name, [])):
        if o <= at < o + ln:
            msg += "; it is byte %d of token %d (place %d of its batch), a " % (at - o, i, i % 64)
            msg += {"lit": "literal", "stored": "stored run of %d bytes" % ln, "match": "match of length %d at distance %d" % (ln, d)}[kind]
    return msg


def members_in_one_call(hip, entries, shift):
    """every entry as one member of ONE call, into a buffer of sentinel bytes: no bad member, every text right, both guards untouched"""
    data, rows = B.table([B.member(s, t) for _, s, t in entries])
    n_bad, st, got, guards = inflate_into_sentinel(hip, data, rows, shift=shift)
    for (name, _, text), o, status in zip(entries, rows["out_off"], st):      # the texts first: a member whose CRC is not its trailer's is written out all the same
        mine = got[int(o):int(o) + len(text)].tobytes()
        assert mine == text, where_it_went_wrong(name, mine, text) + "; status %d" % status
    assert n_bad == 0 and not st.any(), [(entries[i][0], int(st[i])) for i in np.flatnonzero(st)]
    assert guards
    return data, rows


def as_a_file(hip, entries):
    """the same members as a BGZF file with bgzip's end marker: the index finds the table tests/bgzf_util.py computes, the text is whole, and the last byte is the
    last text byte of the file -- and of a few files that end with another member"""
    ms = [B.member(s, t) for _, s, t in entries]
    data, rows = B.table(ms + [B.EOF_MARKER])
    found, n_text, n_comp = bgzf_index(data)
    assert n_comp == len(data) and n_text == sum(len(t) for _, _, t in entries) and len(found) == len(rows)
    for f in ("in_off", "in_len", "out_len", "out_off", "crc"):
        assert np.array_equal(found[f], rows[f]), f
    want = b"".join(t for _, _, t in entries)
    text, st = hip.inflate_bgzf(data, status=True)
    assert not st.any() and text.tobytes() == want
    assert hip.L.oatk_hip_inflate_last_byte(hip.h) == want[-1]
    for i in range(0, len(entries), max(1, len(entries) // 12)):              # at most thirteen more launches, each of two members
        if entries[i][2]:
            assert hip.inflate_bgzf(ms[i] + B.EOF_MARKER).tobytes() == entries[i][2]
            assert hip.L.oatk_hip_inflate_last_byte(hip.h) == entries[i][2][-1], entries[i][0]


def test_overlapped_copies_at_every_distance(hip):
    """527 members, 17,829,021 bytes of text: a match of every length 3..258 at every distance 1..520 (and at 1023, 1024, 1025, 4096, 16384, 32767, 32768 as far as
    a member holds them), each reading what the matches before it wrote"""
    members_in_one_call(hip, G.copy_sweep(), shift=5)


def test_batch_edges(hip):
    """24 members, 8,298 bytes: the first match at place 60..68 and 124..132 of the token stream, a literal, a run of one byte, a match from the member's first
    byte; members of exactly 63, 64, 65, 127, 128, 129 literals"""
    members_in_one_call(hip, G.batch_edges(), shift=11)
    as_a_file(hip, G.batch_edges())


def test_stored_runs_among_tokens(hip):
    """113 members, 96,232 bytes: a stored run of 0, 1, 63, 64, 65, 1000 bytes and of the longest a member allows between fixed blocks, its header at every bit
    offset, read by matches (inside it, into it, overlapped out of it) and followed by a second stored run; a stored run at every place of the batch"""
    members_in_one_call(hip, G.mixed_blocks(), shift=13)
    as_a_file(hip, G.mixed_blocks())


def test_every_input_and_output_phase(hip):
    """2,560 members in one call, 49,664 bytes of text: each member of phase_grid() with its text at every address modulo 16 and its stream at every address modulo
    16, sentinel between the texts and 0xFF between the streams; afterwards the buffer is the texts and, everywhere else, the sentinel"""
    grid = G.phase_grid()
    comp, rows, o_end, label = bytearray(), [], 0, []
    for p in range(16):
        for q in range(16):
            for name, stream, text in grid:
                comp += b"\xff" * (1 + (q - (len(comp) + 1)) % 16)
                o = o_end + 1 + (p - (o_end + 1)) % 16          # at least one byte of sentinel in front of every text
                assert len(comp) % 16 == q and o % 16 == p
                rows.append((len(comp), len(stream), len(text), o, zlib.crc32(text), 0))
                label.append((p, q, name))
                comp += stream
                o_end = o + len(text)
    comp += b"\xff" * 16
    rows = np.array(rows, dtype=_lib.BGZF_MEMBER)
    assert len(rows) == 2560 and np.all(np.diff(rows["out_off"].astype(np.int64)) > 0)
    cap = o_end + 16
    buf = torch.full((GUARD + cap + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda:%d" % hip.device)
    torch.cuda.synchronize()
    assert buf.data_ptr() % 16 == 0 and GUARD % 16 == 0          # the output phases are what they claim to be (the compressed bytes go to a fresh allocation)
    n_bad, st = hip.inflate_members(bytes(comp), rows, buf.data_ptr() + GUARD, cap)
    got = buf.cpu().numpy()
    want = np.full(len(got), SENTINEL, np.uint8)
    for r, (_, _, text) in zip(rows, grid * 256):
        want[GUARD + int(r["out_off"]):GUARD + int(r["out_off"]) + len(text)] = np.frombuffer(text, np.uint8)
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0]) - GUARD
        i = int(np.searchsorted(rows["out_off"].astype(np.int64), at, side="right")) - 1
        raise AssertionError("byte %d of the text buffer is 0x%02x, not 0x%02x: member %d (output phase, input phase, kind) = %s begins at %d and is %d long"
                             % (at, got[at + GUARD], want[at + GUARD], i, label[max(i, 0)], int(rows["out_off"][max(i, 0)]), int(rows["out_len"][max(i, 0)])))
    assert n_bad == 0 and not st.any(), [(label[i], int(st[i])) for i in np.flatnonzero(st)[:8]]


def test_crc_piece_boundaries(hip):
    """15 members, 432,128 bytes of compressible text that ends on, before and behind a 1 KiB piece; then 36 damaged copies of the largest stored member (65,505
    bytes), each between good members: every bit of the trailer's CRC flipped in turn, and a payload bit flipped in the first piece's first and last byte, the
    second piece's first and the last piece's last"""
    members_in_one_call(hip, G.crc_lengths(), shift=9)
    t = bytes(np.random.default_rng(41).integers(0, 256, 65505, dtype=np.uint8).tolist())
    stream, _ = B.write_blocks([("stored", t)])
    assert len(stream) + 26 == 65536 and G.zlib_text(stream) == t
    crc, bad = zlib.crc32(t), []
    for bit in range(32):
        bad.append(B.member(stream, crc=crc ^ (1 << bit), isize=len(t)))
    for k, (at, bit) in enumerate([(0, 0), (1023, 7), (1024, 0), (65504, 7)]):
        s = bytearray(stream)
        s[5 + at] ^= 1 << bit
        assert zlib.crc32(G.zlib_text(bytes(s))) != crc
        bad.append(B.member(bytes(s), t))
    ms = [G.good_member(0)]
    for i, m in enumerate(bad):
        ms += [m, G.good_member(1 + i % 2)]
    data, rows = B.table(ms)
    n_bad, st, got, guards = inflate_into_sentinel(hip, data, rows, shift=1)
    assert n_bad == 36 and list(st) == [0] + [3, 0] * 36
    assert guards                                                # (the members lie end to end: the guards and the good texts are everything outside a bad one's range)
    for i in range(0, len(ms), 2):
        text = G.GOOD[0 if i == 0 else 1 + (i // 2 - 1) % 2]
        o = int(rows["out_off"][i])
        assert int(rows["out_len"][i]) == len(text) and got[o:o + len(text)].tobytes() == text, i


def test_many_bad_members_are_counted(hip):
    """300 members of which every third is bad, the statuses 1, 2, 3 in turn: the count is 100, with and without a status vector"""
    by = {1: [], 2: [], 3: []}
    for c in G.damage_cases():
        by[c[3]].append(c)
    ms, texts, edits, expect = [], [], [], []
    for i in range(300):
        if i % 3 == 2:
            j = i // 3
            _, m, edit, status = by[j % 3 + 1][(j // 3) % len(by[j % 3 + 1])]
            ms.append(m), texts.append(None), edits.append(edit), expect.append(status)
        else:
            t = G.acgt(1 + 37 * i % 2500, 2000 + i) if i % 2 else G.fasta_like(1 + 53 * i % 4000, 2000 + i)
            ms.append(B.member(B.raw_deflate(t, (1, 6, 9, 0)[i % 4]), t)), texts.append(t), edits.append(None), expect.append(0)
    data, rows = B.table(ms)
    for i, edit in enumerate(edits):
        if edit:
            edit(rows[i:i + 1])
    n_bad, st, got, guards = inflate_into_sentinel(hip, data, rows, shift=6)
    assert n_bad == 100 and expect.count(1) == 34 and expect.count(2) == 33 and expect.count(3) == 33
    assert list(st) == expect and guards

    def check(got):
        for i, t in enumerate(texts):
            o, ln = int(rows["out_off"][i]), int(rows["out_len"][i])
            if t is not None:
                assert got[o:o + ln].tobytes() == t, i
            elif expect[i] != 3:                                # a member that is no stream, or of another length, leaves its range as it was
                assert np.all(got[o:o + ln] == SENTINEL), i
    check(got)
    # the same call without a status vector, through the C ABI
    cap = int(rows["out_off"][-1]) + int(rows["out_len"][-1])
    buf = torch.full((GUARD + cap + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda:%d" % hip.device)
    torch.cuda.synchronize()
    c, m, bad = np.frombuffer(data, np.uint8), np.ascontiguousarray(rows, dtype=_lib.BGZF_MEMBER), C.c_uint64()
    rc = hip.L.oatk_hip_inflate_bgzf_host(hip.h, c.ctypes.data, c.size, m.ctypes.data, len(m), buf.data_ptr() + GUARD, cap, C.byref(bad), None)
    assert rc == _lib.OK and bad.value == 100
    h = buf.cpu().numpy()
    assert np.all(h[:GUARD] == SENTINEL) and np.all(h[GUARD + cap:] == SENTINEL)
    check(h[GUARD:GUARD + cap])
