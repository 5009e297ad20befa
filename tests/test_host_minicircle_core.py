"""CPU: oatk_amd/csrc/minicircle_core.hpp -- the rule that decides whether an alignment record walks round the anchor periodically, and the canonical path
element (the device kernels of csrc/minicircle.hpp run the same functions) -- and oatk_mc_path_stats of csrc/host/minicircle_host.c, built with AddressSanitizer +
UBSan as a stand-alone program (tests/c/minicircle_core_check.cpp) and run over the hand-derived table of tests/minicircle_util.py, records whose hits lie past
position 1024, and 20 000 seeded random records per seed.  A lane's walk, the 64-fragment chunks of a wave and a restatement in the reference's loop order agree on
every record; the statistics equal hand-computed values on a three-unitig graph, a path over a missing arc is refused; the sanitizers report nothing."""
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
    exe = str(tmp_path_factory.mktemp("minicirclecore") / "minicircle_core_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off", "-I" + CSRC,
           "-I" + os.path.join(ROOT, "include"), "-o", exe, "-x", "c", os.path.join(CSRC, "host", "minicircle_host.c"),
           "-x", "c++", os.path.join(ROOT, "tests", "c", "minicircle_core_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_core_equals_the_restatement_and_the_statistics_are_the_hand_computed_ones(checker, seed):
    r = subprocess.run([checker, str(seed)], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    w = r.stdout.split()
    assert w[0] == "OK", r.stdout
    got = {x.split("=")[0]: int(x.split("=")[1]) for x in w[1:]}
    assert got["records"] == 15 + 3 + 20000
    # the random records reach both verdicts, both length classes and units that begin behind the first chunk, with many different paths
    assert 1000 <= got["valid"] <= got["records"] - 1000 and got["long"] >= 1000 and got["chunk_first"] >= 1 and got["distinct"] >= 100
