"""CPU: oatk_amd/csrc/bam_core.hpp -- the header walk, the record predicates and the letter tables the BAM kernels run (csrc/bam.hpp) -- built with g++ under
AddressSanitizer + UBSan as a stand-alone program (tests/c/bam_core_check.cpp) and run over the streams tests/test_gpu_bam.py gives the device: the made ones, every
damage case, cut streams and some hundreds of single-byte mutations of a small one.  Verdicts, candidate lists, the chain, where it stops and as what, names and
letters equal the plain-Python reading of tests/bam_util.py; the chain built by successors and pointer doubling equals the serial walk; every stream sits in a heap
block of exactly its size and the sanitizers report nothing."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import adversarial as A
import bam_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oatk_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
HDR_VERDICT = {"ok": 0, "more": 1, "bad": 2}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("bamcore") / "bam_core_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I" + CSRC, "-o", exe,
           os.path.join(ROOT, "tests", "c", "bam_core_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def ask(checker, tmp_path, cases):
    """[(stream, header?, letters?)] -> per case a dict of what the core made of it"""
    p = tmp_path / "cases.bin"
    with open(p, "wb") as f:
        for b, hdr, letters in cases:
            f.write(struct.pack("<QBB", len(b), 1 if hdr else 0, 1 if letters else 0) + b)
    r = subprocess.run([checker, str(p)], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    out = []
    for ln in r.stdout.splitlines():
        w = ln.split(" ")
        if w[0] == "H":
            out.append({"hdr": (int(w[1]), int(w[2]), int(w[3])), "reads": []})
        elif w[0] == "C":
            out[-1]["cand"] = [int(x) for x in w[2:]]
            assert len(out[-1]["cand"]) == int(w[1])
        elif w[0] == "R":
            out[-1]["chain"] = ([int(x) for x in w[4:]], int(w[2]), int(w[3]))
            assert len(out[-1]["chain"][0]) == int(w[1])
        elif w[0] == "D":
            out[-1]["doubling"] = int(w[1])
        elif w[0] == "S":
            out[-1]["reads"].append((bytes.fromhex(w[1][:-1]), w[2].encode() if len(w) > 2 else b""))
    assert len(out) == len(cases)
    return out


def check(got, b, hdr, letters=False):
    """one case against the oracle"""
    v, x = U.header_walk(b) if hdr else ("ok", 0)
    assert got["hdr"][0] == HDR_VERDICT[v]
    if v == "more":
        assert got["hdr"][2] == x
    if v != "ok":
        return
    assert got["hdr"][1] == x
    assert got["cand"] == U.candidates(b, x)
    recs, t, why = U.chain(b, x)
    assert got["chain"] == (recs, t, why)
    assert got["doubling"] == 1
    if letters:
        assert got["reads"] == [U.read_at(b, o)[:2] for o in recs]


def made_streams():
    hifi = A.hifi_like(40, 20000, 3000, seed=11)
    rng = np.random.default_rng(2)
    return {
        "sweep tags cigar0": U.stream(U.sweep_reads(True, 0)),
        "sweep plain cigar3": U.stream(U.sweep_reads(False, 3)),
        "hifi": U.stream([dict(name=b"m84/%d/ccs" % i, seq=r, qual=rng.integers(0, 94, len(r), dtype=np.uint8).tobytes(), tags=U.tag_int(b"np", i))
                          for i, r in enumerate(hifi)], refs=((b"chr1", 1000), (b"x", 5))),
        "short with int tags": U.stream(U.short_reads_with_int_tags(300, 1)),
        "nested fakes": U.stream(U.nested_fake_records()),
        "header only": U.header(),
    }


def test_made_streams_read_as_the_oracle_reads_them(checker, tmp_path):
    s = made_streams()
    got = ask(checker, tmp_path, [(b, True, True) for b in s.values()])
    for (name, b), g in zip(s.items(), got):
        check(g, b, True, letters=True)
        assert g["chain"][2] == U.CLEAN, name
    names, reads, _ = U.parse(s["sweep tags cigar0"])
    want = U.sweep_reads(True, 0)
    assert names == [w["name"] for w in want] and reads == [w["seq"] for w in want]      # the oracle itself reads back what the writer was given
    # the streams are what they are for: false candidates exist, and the fake records are among them without joining the chain
    g = got[list(s).index("short with int tags")]
    assert len(g["cand"]) > len(g["chain"][0])
    g = got[list(s).index("nested fakes")]
    assert len(g["cand"]) >= len(g["chain"][0]) + 4 and len(g["chain"][0]) == 4


def test_damage_cases_get_their_verdict(checker, tmp_path):
    cases = U.damage_cases()
    got = ask(checker, tmp_path, [(b, True, False) for b, _ in cases.values()])
    for (name, (b, want)), g in zip(cases.items(), got):
        check(g, b, True)
        if want == "arg":
            assert g["hdr"][0] == 2 or g["chain"][2] in (U.CUT, U.BAD), name
        else:                                                   # the chain is clean: the refusal is the record kernel's, by the flag
            assert g["chain"][2] == U.CLEAN, name
            assert any(U.read_at(b, o)[2] & 0x910 for o in g["chain"][0]), name


def test_cut_streams_and_header_prefixes(checker, tmp_path):
    b = U.stream(U.sweep_reads(True, 3)[:40], text=b"@HD\tVN:1.6\n@PG\tID:x\n", refs=((b"ref", 9),))
    _, s0 = U.header_walk(b)
    cuts = list(range(0, s0 + 80)) + [len(b) - k for k in range(0, 60)]
    got = ask(checker, tmp_path, [(b[:c], True, False) for c in cuts] + [(b[s0 + 7:], False, False), (b[s0:s0 + 500], False, True)])
    for c, g in zip(cuts, got):
        check(g, b[:c], True)
    check(got[-2], b[s0 + 7:], False)
    check(got[-1], b[s0:s0 + 500], False, letters=True)
    assert got[0]["hdr"][0] == 1 and got[s0 - 1]["hdr"][0] == 1 and got[s0]["hdr"] == (0, s0, 0)


def test_single_byte_mutations(checker, tmp_path):
    base = U.stream(U.short_reads_with_int_tags(6, 4) + U.nested_fake_records())
    rng = np.random.default_rng(9)
    cases = []
    for _ in range(400):
        b = bytearray(base)
        p = int(rng.integers(0, len(b)))
        b[p] = int(rng.integers(0, 256)) if rng.integers(0, 2) else b[p] ^ (1 << int(rng.integers(0, 8)))
        cases.append(bytes(b))
    got = ask(checker, tmp_path, [(b, True, False) for b in cases])
    for b, g in zip(cases, got):
        check(g, b, True)
