"""The per-read chain walk of the error correction (ec.hpp: ec_blocks_wave, behind ec_stage_blocks_wave_kernel) keeps its state in scalar
registers: every value the loop branches on is the same in all lanes of the wave.  What
the compiler makes of it for gfx950 says whether it still knows -- a broadcast through LDS (ds_bpermute_b32) or a bit scan in a vector
register (v_ffbl_b32) inside the serial loop is what this file keeps out.  No GPU needed: the kernels are compiled, not run."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc") or None

pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not found")

KERNELS = ["ec_stage_blocks_wave_kernel"]


def compile_isa(d, name, text):
    src = d / (name + ".hip")
    src.write_text(text)
    out = d / (name + ".s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "oatk_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), str(src), "-o", str(out)], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    text = out.read_text()
    funcs = {}
    # a kernel's code runs from its label to .Lfunc_end<N>; the resource summary (ScratchSize ...) follows in comments up to the next label
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:(.*?)(?=^_Z\w+:|\Z)", text, re.S | re.M):
        funcs[m.group(1)] = (m.group(2), m.group(3))
    return funcs


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    return compile_isa(tmp_path_factory.mktemp("isa"), "walks", '#include "ec.hpp"\n')


@pytest.mark.parametrize("kernel", KERNELS)
def test_walk_is_scalar(isa, kernel):
    names = [n for n in isa if kernel in n]
    assert len(names) == 1, (kernel, sorted(isa))
    body, summary = isa[names[0]]
    assert body.count("ds_bpermute_b32") == 0
    assert body.count("v_ffbl_b32") == 0
    assert body.count("s_ff1_i32_b64") >= 1
    m = re.search(r"ScratchSize:\s*(\d+)", summary)
    assert m is not None and int(m.group(1)) == 0


def test_kmer_hash_kernel_keeps_eight_waves_and_no_scratch(tmp_path):
    """kmer_hash_kernel's rate is records in flight: it is built for eight waves per SIMD (__launch_bounds__(64, 8), 64 VGPRs), and a register more than that
    becomes scratch traffic without a word from the compiler.  It also places the records now, so it carries their words across the gathers and the barrier."""
    funcs = compile_isa(tmp_path, "kmh", '#include "kmer_hash.hpp"\n')
    names = [n for n in funcs if "kmer_hash_kernel" in n]
    assert len(names) == 1, sorted(funcs)
    summary = funcs[names[0]][1]
    scratch, vgprs = re.search(r"ScratchSize:\s*(\d+)", summary), re.search(r"NumVgprs:\s*(\d+)", summary)
    assert scratch is not None and int(scratch.group(1)) == 0
    assert vgprs is not None and int(vgprs.group(1)) <= 64
