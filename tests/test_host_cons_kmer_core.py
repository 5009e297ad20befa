"""CPU: the k-mer rows of oatk_amd/csrc/cons_str_core.hpp -- kmer_word, which cstr_kmer_kernel (csrc/cons_str.hpp) stores once per consensus when the reads are
sharded over several handles, and open() with Tables::kmer set, which the string kernels read then -- built with g++ under AddressSanitizer + UBSan as a stand-alone
program (tests/c/cons_kmer_core_check.cpp).  For k = 5, 16, 17, 64, 65 and 1101, every source phase p & 3 and both strands: every word of a row equals a code-by-code
restatement, the codes behind k - 1 are zero, code_at on the stored row (p = 0, rev 0 and 1) equals code_at on the read, and over a small table the text of every
piece (syncmer x rev x beg in {0, 9, k - 1, -4} x space) from the k-mer-backed tables equals the read-backed text.  The source strings are allocated to the byte, so a
load outside [p >> 2, (p + k - 1) >> 2] is a sanitizer report; the k-mer-backed tables carry no reads at all."""
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
    exe = str(tmp_path_factory.mktemp("conskmercore") / "cons_kmer_core_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I" + CSRC, "-o", exe,
           os.path.join(ROOT, "tests", "c", "cons_kmer_core_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.mark.parametrize("k", [5, 16, 17, 64, 65, 1101])
@pytest.mark.parametrize("seed", [1, 2])
def test_kmer_rows_equal_the_code_by_code_restatement(checker, k, seed):
    r = subprocess.run([checker, str(k), str(seed)], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    w = r.stdout.split()
    assert w[0] == "OK", r.stdout
    got = {x.split("=")[0]: int(x.split("=")[1]) for x in w[1:]}
    row_words = 2 * ((k + 31) // 32)                                     # the table's stride: 8 * ceil(k / 32) bytes
    n_kmers = 4 * 2 * 4                                                  # phases x strands x (p below 4, and three further positions)
    assert got["words"] == n_kmers * row_words
    assert got["codes"] == n_kmers * k and got["tail"] == n_kmers * (16 * row_words - k)
    assert got["phases"] == 255                                          # every phase on either strand
    # 16 syncmers, one of them unprepared, x 2 orientations x 4 beg x 2 spaces; syncmer 12 has no first occurrence
    assert got["pieces"] == 15 * 16 and got["nofirst"] == 16
    assert got["chars"] > got["pieces"]
