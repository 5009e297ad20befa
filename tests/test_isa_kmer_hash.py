"""kmer_hash_kernel (kmer_hash.hpp) as the compiler makes it for gfx950.  A workgroup of four waves prepares 64 records, then its first wave runs the
Murmur chains of all of them, one lane per record.  Two things the source cannot promise by itself: that the kernel still fits eight waves per SIMD
with nothing in scratch now that a workgroup is four waves, and that the chain loop runs under a FULL exec mask -- a wave64 instruction under a
partial mask costs the same issue slot, which is why the chain moved to full waves.  No GPU needed: the kernel is compiled, not run."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc") or None

pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not found")

SAVEEXEC = re.compile(r"\bs_(and|andn2|or|xor|andn1|orn2)_saveexec_b64\b")
RESTORE = re.compile(r"\bs_(or|mov)_b64\s+exec\b")
BRANCH = re.compile(r"\bs_cbranch_\w+\s+(\.LBB\d+_\d+)")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")


@pytest.fixture(scope="module")
def kernel(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_kmh")
    src, out = d / "kmh.hip", d / "kmh.s"
    src.write_text('#include "kmer_hash.hpp"\n')
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "oatk_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), str(src), "-o", str(out)], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    text = out.read_text()
    # the kernel's code runs from its label to .Lfunc_end<N>; the resource summary and the kernel descriptor follow up to the next function
    found = re.findall(r"^(_Z\w*kmer_hash_kernel\w*):[^\n]*\n(.*?)^\.Lfunc_end\d+:(.*?)(?=^_Z\w+:|\Z)", text, re.S | re.M)
    assert len(found) == 1, [f[0] for f in found]
    return found[0][1], found[0][2]


def test_four_wave_workgroup_keeps_eight_waves_per_simd_and_no_scratch(kernel):
    _, summary = kernel
    scratch, vgprs, occ = (re.search(r"%s:\s*(\d+)" % k, summary) for k in ("ScratchSize", "NumVgprs", "Occupancy"))
    assert scratch is not None and int(scratch.group(1)) == 0
    assert vgprs is not None and int(vgprs.group(1)) <= 64
    assert occ is not None and int(occ.group(1)) == 8
    # no LDS of its own besides the dynamic block the launch sizes (kmh_lds_bytes): residency is what the launch computes
    lds = re.search(r"LDSByteSize:\s*(\d+)", summary)
    assert lds is not None and int(lds.group(1)) == 0


def test_chain_loop_runs_under_a_full_exec_mask(kernel):
    """Behind the kernel's one barrier come the chain's loops (the eight-step unrolled one and its remainder): ds_read of the pre-mixed blocks and the
    64-bit multiply.  None may sit inside, or contain, a saveexec region: lanes past the shard's last record run the chain on a duplicate and are
    masked only at the stores."""
    body, _ = kernel
    lines = body.split("\n")
    bar = [i for i, l in enumerate(lines) if re.search(r"\bs_barrier\b", l)]
    assert len(bar) == 1, "one barrier between the preparation and the chain"
    seen, masked_at, masked = {}, [], False
    tail = lines[bar[0]:]
    for i, l in enumerate(tail):
        m = LABEL.match(l)
        if m:
            seen[m.group(1)] = i
        if SAVEEXEC.search(l):
            masked = True
        elif RESTORE.search(l):
            masked = False
        masked_at.append(masked)
    loops = []
    for i, l in enumerate(tail):
        m = BRANCH.search(l)
        if m and m.group(1) in seen and seen[m.group(1)] < i:
            loops.append((seen[m.group(1)], i))
    chains = [(a, b) for a, b in loops if any("v_mad_u64_u32" in x for x in tail[a:b]) and any("ds_read" in x for x in tail[a:b])]
    assert chains, "no chain loop found behind the barrier"
    for a, b in chains:
        assert not any(masked_at[a:b + 1]), "chain loop under a partial exec mask:\n" + "\n".join(tail[max(a - 12, 0):a + 4])
    # the stores, and only they, are masked by lane < nrec: the first saveexec behind the barrier comes after the last chain loop
    first_mask = next((i for i, l in enumerate(tail) if SAVEEXEC.search(l)), None)
    assert first_mask is not None and first_mask > max(b for _, b in chains)
    assert not any("global_store" in x for x in tail[:first_mask])
