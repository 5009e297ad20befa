"""CPU: oatk_amd/csrc/count_onepass_core.hpp -- which sorted records the count's one-pass check compares (every record that is no group head with its
predecessor), which k-mers a strip of eight loads for it, and where a difference is reported (the group's head, found by walking back) -- the functions
gather_verify_kernel of csrc/count.hpp runs.  Built with AddressSanitizer + UBSan as a stand-alone program (tests/c/count_onepass_check.cpp) that restates
the kernel's tile and strip walk over heap arrays of exactly n records and compares it with the plain statement, at every tile and strip edge and on seeded
random batches; the sanitizers report nothing."""
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
    exe = str(tmp_path_factory.mktemp("onepasscore") / "count_onepass_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I" + CSRC, "-o", exe,
           os.path.join(ROOT, "tests", "c", "count_onepass_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_walk_compares_every_follower_with_its_predecessor_and_reports_at_the_head(checker, seed):
    r = subprocess.run([checker, str(seed)], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    w = r.stdout.split()
    assert w[0] == "OK", r.stdout
    got = {x.split("=")[0]: int(x.split("=")[1]) for x in w[1:]}
    # the batches reach clean and mixed groups, tiles that need the record in front of them, and strips that share it: fewer loads than two per comparison
    assert got["batches"] >= 600 and got["bad"] >= 1000 and got["pred"] >= 100
    assert got["compared"] < got["loads"] < 2 * got["compared"]
