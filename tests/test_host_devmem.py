"""CPU: oatk_amd/csrc/devmem.hpp -- ChunkPool and DevBuf, under every device array the library owns -- built with g++ as a stand-alone program
(tests/c/devmem_test.cpp) that defines the hip* entry points the header calls over a ledger in host memory, so every path runs without a GPU, the failures a
test could reach on a real one only by exhausting it included.  One build under AddressSanitizer + UBSan with leak detection (a hipMalloc'ed block is a heap
block of exactly its size); the threaded case once more under ThreadSanitizer.

  caps     cap after ensure / grow_keep / reserve of 1, the threshold - 1, the threshold, 64 MB - 1, 64 MB, 64 MB + 1 and 200 MB, with and without a pool,
           against the numbers of the code before it had one growth routine
  keep     grow_keep copies exactly `used` bytes and frees the old block after the wait; ensure frees first; pieces grow where they are; an outgrown range
           gets the same pieces in the same order and no copy; reserve in pieces maps nothing
  zero     pieces another buffer gave back are cleared (exactly the new span) and waited for; pieces fresh from the driver are not
  fail     the k-th hipMalloc / hipMemCreate / hipMemAddressReserve / hipMemcpyAsync / hipMemMap / hipMemSetAccess of each scenario fails, each k in turn: the call
           returns true with cap >= bytes, or false with the buffer empty or exactly as before; the three rules of devmem.hpp's failure paths by name; and
           after every one of them nothing is left with the driver but idle pieces and ranges
  own      a struct of buffers that is deleted gives everything back; a DevBuf can be neither copied nor moved (static_assert)
  threads  eight threads create, grow and drop 100 buffers each over one pool while it warms"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oatk_amd", "csrc")
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def build(tmp_path_factory, sanitizer):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("devmem") / "devmem_test")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=" + sanitizer, "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE, "-I" + CSRC,
           "-o", exe, os.path.join(ROOT, "tests", "c", "devmem_test.cpp"), "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and any(s in r.stderr for s in ("-fsanitize", "cannot find -lasan", "cannot find -lubsan", "cannot find -ltsan", "san_preinit.o")):
        pytest.skip("this g++ has no %s sanitizer runtime" % sanitizer)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def asan(tmp_path_factory):
    return build(tmp_path_factory, "address,undefined")


@pytest.fixture(scope="module")
def tsan(tmp_path_factory):
    return build(tmp_path_factory, "thread")


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1", TSAN_OPTIONS="halt_on_error=1 exitcode=66")


def run(exe, case):
    r = subprocess.run([exe, case], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0 and "FAILED" not in r.stdout and ("ok: " + case) in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr, r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("case", ["caps", "keep", "zero", "own", "threads"])
def test_devmem(asan, case):
    run(asan, case)


def test_devmem_every_failure(asan):
    out = run(asan, "fail")
    # each scenario made the calls it is there for: the failures were injected, not skipped
    n = {ln.split(":")[0]: int(ln.split(":")[1].split()[0]) for ln in out.splitlines() if "failures injected" in ln}
    assert len(n) == 10 and all(v >= 1 for v in n.values()), n
    assert n["fresh ensure"] >= 10 and n["grow_keep from a small block to pieces"] >= 11 and n["grow_keep of a buffer in pieces"] >= 7, n


def test_devmem_threads_under_tsan(tsan):
    run(tsan, "threads")
