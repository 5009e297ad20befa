"""CPU: oatk_amd/csrc/cons_str_core.hpp -- what decides whether a piece of a consensus sequence is prepared, how long it is and which character stands at any offset
of it (the device kernels of csrc/cons_str.hpp run the same functions) -- built with g++ under AddressSanitizer + UBSan as a stand-alone program
(tests/c/cons_str_core_check.cpp) and run over small hand-made tables: k = 5, 64, 65 and 1101, both orientations, beg in {0, 1, k - 1, -4}, hoco and base space, run
lengths of 0, 254 and 700, a syncmer without a first occurrence, one with no occurrence counted, one that is not prepared, and k-mers that start at each of the four
2-bit phases of their read's packed string.  Length and every character equal a restatement that appends one character at a time; the text assembled tile by tile
with the bisection the fill kernel uses is the same; the sanitizers report nothing.  The N branches are reached here only: real reads give no live syncmer whose every
occurrence was corrected away."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oatk_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("consstrcore") / "cons_str_core_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I" + CSRC, "-o", exe,
           os.path.join(ROOT, "tests", "c", "cons_str_core_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.mark.parametrize("k", [5, 64, 65, 1101])
@pytest.mark.parametrize("seed", [1, 2])
def test_core_equals_the_char_by_char_restatement(checker, k, seed):
    r = subprocess.run([checker, str(k), str(seed)], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    w = r.stdout.split()
    assert w[0] == "OK", r.stdout
    got = {x.split("=")[0]: int(x.split("=")[1]) for x in w[1:]}
    # 16 syncmers (one unprepared) and one id past the table, x 2 orientations x 4 beg x 2 spaces
    assert got["pieces"] == 15 * 16 and got["unprepared"] == 2 * 16
    assert got["n_first"] == 16 and got["m0"] == 16
    assert got["phases"] & 15 == 15 and got["phases"] >> 4 == 15        # every phase, read forward and read complemented
    assert got["rl0"] > 0 and got["rl254"] > 0 and got["rl700"] > 0
    assert got["chars"] > 15 * 16 * 1                                    # (k = 5, beg = k - 1: one position and what it expands to)
