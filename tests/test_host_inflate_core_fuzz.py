"""CPU: oatk_amd/csrc/inflate_core.hpp -- the DEFLATE decoder the device kernel runs (csrc/inflate.hpp) -- built with g++ under AddressSanitizer + UBSan as a
stand-alone program (tests/c/inflate_core_fuzz.cpp) and run against zlib: members made with every level and strategy (Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE among them),
stored members, flushes inside a member, texts of runs, short periods and random ACGT come out as zlib's text; damaged copies (bits flipped, bytes dropped, tails cut,
wrong lengths) come out as an error or as zlib's bytes, never accepted with other bytes; input and output sit in heap blocks of exactly their sizes, so an access one
byte outside them is a sanitizer report; every run ends within its bound.  The streams the GPU tests feed the kernel (tests/bgzf_util.py, tests/gpu_inflate_cases.py) are
put to the core here first, the hand-made ones and the sweeps of tests/test_gpu_inflate_sweeps.py included."""
import os
import shutil
import subprocess
import zlib

import pytest

import bgzf_util as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oatk_amd", "csrc")


@pytest.fixture(scope="module")
def fuzzer(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("inffuzz") / "inflate_core_fuzz")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I" + CSRC, "-o", exe,
           os.path.join(ROOT, "tests", "c", "inflate_core_fuzz.cpp"), "-lz"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")


@pytest.mark.parametrize("seed", [1, 2])
def test_core_equals_zlib_on_made_and_damaged_members(fuzzer, seed):
    r = subprocess.run([fuzzer, "16", str(seed)], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "members equal to zlib's text" in r.stdout and "no member accepted with other bytes" in r.stdout


def ask(fuzzer, tmp_path, cases):
    """[(stream, out_len)] -> [(status, n_cross, crc)] from the core"""
    p = tmp_path / "members.txt"
    p.write_text("".join("%s %d\n" % (s.hex() or "-", n) for s, n in cases))
    r = subprocess.run([fuzzer, "members", str(p)], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(cases)
    return [(int(a), int(b), int(c, 16)) for a, b, c in rows]


def test_hand_made_streams(fuzzer, tmp_path):
    """what zlib's deflate never writes: each error is the stream error it should be, and the repeat codes that run across the literal/distance boundary are read
    as zlib's inflate reads them (the core's own counter says the stream does what it was made for)"""
    stream, text = B.repeat_across_the_boundary()
    got = ask(fuzzer, tmp_path, [(stream, len(text)), (B.first_token_is_a_match(), 3), (B.distance_one_beyond(), 5), (B.oversubscribed(), 0), (B.block_type_3(), 0),
                                 (B.stored_len_mismatch(), 5), (b"", 0), (b"\x03\x00", 0), (b"\x03\x00\x00", 0), (b"\x03\x00", 1), (B.stored(b"x"), 1)])
    assert got[0] == (0, 1, zlib.crc32(text))
    assert [g[0] for g in got[1:7]] == [1, 1, 1, 1, 1, 1]
    assert got[7] == (0, 0, 0)                          # bgzip's end marker: a fixed block that holds nothing
    assert got[8][0] == 1 and got[9][0] == 2            # a byte behind the final block; a text shorter than its trailer says
    assert got[10] == (0, 0, zlib.crc32(b"x"))
    for bad in (B.first_token_is_a_match(), B.distance_one_beyond(), B.oversubscribed(), B.block_type_3(), B.stored_len_mismatch()):
        with pytest.raises(zlib.error):                 # zlib refuses them too
            zlib.decompressobj(-15).decompress(bad)


def test_members_of_the_gpu_tests_decode_without_a_rejection(fuzzer, tmp_path):
    """every valid member tests/test_gpu_inflate.py and tests/test_gpu_inflate_sweeps.py build is one the core takes, with zlib's CRC over what its tokens make:
    a rejection or a wrong byte there would be the decoder's, not the kernel's.  (All of them: the 527 members of the copy sweep too, 18 MB of text.)"""
    import gpu_inflate_cases as G
    members = list(G.member_shapes()) + [e for f in G.SWEEP_LISTS for e in f()]
    got = ask(fuzzer, tmp_path, [(s, len(t)) for _, s, t in members])
    for (name, s, t), g in zip(members, got):
        assert g[0] == 0 and g[2] == zlib.crc32(t), (name, g)
        assert zlib.decompressobj(-15).decompress(s) == t, name
