#!/usr/bin/env python3
"""VALU instructions of kernel B along ONE path through its tile loop, priced by issue class (the classes of tools/isa_mix.py).  CPU only (hipcc -S).

tools/isa_mix.py counts the whole loop body, rare paths included; this walks the listing from the loop header the way a wave does and counts what it issues.
The path is given as one letter per conditional branch met on the way: T taken, N not taken.  Run it without --path first: it walks with N everywhere and
prints every conditional branch it meets with its line in the listing, which is how a path is found (read the listing around each).  Instructions skipped
under a cleared exec mask behind `s_cbranch_execz` are NOT issued when the branch is taken; instructions between `s_and_saveexec` and `s_or_b64 exec` with no
branch round them are issued and counted.  Blocks of the loop that the compiler has placed behind the loop's last line are followed there and back.

    python tools/isa_tile_path.py --form 2048,true,128,6 --path TNNT... [--header path/to/scan_syncmer_fast.hpp] [--marks]

--marks prints the running VALU count and weighted cycles at every label, barrier and branch on the path: the stretches of DESIGN 5's table are differences
of those.  The ordinary tile (inside wave, no repeat mode, a pending tile without syncmers, no candidate) is what DESIGN 5 tabulates."""
import argparse, collections, os, re, subprocess, sys, tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_mix import RATES, ROOT


def price(op):
    for pat, c, name in RATES:
        if re.search(pat, op):
            return c, name
    return 4.0, "other (4.0)"


def listing(header, form):
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "kb.hip"), "w") as f:
        f.write('#include <hip/hip_runtime.h>\n#include "%s"\ntemplate __global__ void oatk::syncmer_fast_kernel<%s>(oatk::SynArgs);\n' % (header, form))
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", "kb.s", "kb.hip"],
                       cwd=d, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    res = ", ".join(m.group(1).strip() for m in re.finditer(r"remark:\s+((?:TotalSGPRs|VGPRs|ScratchSize|Occupancy|LDS Size).*?) \[-Rpass", r.stdout))
    return open(os.path.join(d, "kb.s")).read(), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", default="2048,true,128,6", help="template arguments R,S31,NT,SH")
    ap.add_argument("--header", default=os.path.join(ROOT, "oatk_amd/csrc/scan_syncmer_fast.hpp"))
    ap.add_argument("--path", default="")
    ap.add_argument("--marks", action="store_true")
    a = ap.parse_args()
    asm, res = listing(os.path.abspath(a.header), a.form)
    m = re.search(r"^(_ZN4oatk19syncmer_fast_kernel\w*):(.*?)\.Lfunc_end", asm, re.S | re.M)
    ins, labels, loops = [], {}, []
    for no, raw in enumerate(m.group(2).splitlines()):
        ln = raw.split(";")[0].strip()
        if ln.endswith(":") and "Loop Header: Depth=1" in raw:
            loops.append(ln[:-1])
        if not ln or ln.startswith(("//", ".")) and not ln.endswith(":"):
            continue
        if ln.endswith(":"):
            labels[ln[:-1]] = len(ins)
            continue
        ins.append((no + 1, ln))
    # the tile loop: the outermost loop with the longest body (the listing marks loop headers)
    best = (0, 0, 0)
    for i, (_, ln) in enumerate(ins):
        mm = re.match(r"s_c?branch\w*\s+(\S+)", ln)
        if mm and mm.group(1) in loops and labels[mm.group(1)] < i and i - labels[mm.group(1)] > best[0]:
            best = (i - labels[mm.group(1)], labels[mm.group(1)], i)
    head, back = best[1], best[2]
    at = {v: k for k, v in labels.items()}
    ops, by, n, cyc, dec, pc, steps = collections.Counter(), collections.Counter(), 0, 0.0, 0, head, 0
    print("kernel %s\nresources: %s\nloop: listing lines %d .. %d" % (m.group(1), res, ins[head][0], ins[back][0]))
    while True:
        steps += 1
        assert steps < 100000, "the path does not come back to the loop header"
        no, ln = ins[pc]
        op = ln.split()[0]
        if a.marks and pc in at:
            print("  %-12s line %5d   VALU %4d   cycles %7.1f" % (at[pc], no, n, cyc))
        if op.startswith("v_"):
            c, name = price(op)
            n, cyc = n + 1, cyc + c
            ops[op] += 1
            by[name] += 1
        if a.marks and op == "s_barrier":
            print("  %-12s line %5d   VALU %4d   cycles %7.1f" % ("s_barrier", no, n, cyc))
        mm = re.match(r"(s_cbranch\w*|s_branch)\s+(\S+)", ln)
        if mm:
            tgt = labels[mm.group(2)]
            if mm.group(1) == "s_branch":
                taken = True
            else:
                taken = dec < len(a.path) and a.path[dec] == "T"
                print("  branch %2d  line %5d  %-36s %s   VALU %4d   cycles %7.1f" % (dec, no, ln, "T" if taken else "N", n, cyc))
                dec += 1
            if taken:
                if tgt == head:
                    break
                # (a block of the loop may stand BEHIND the loop's last line: the compiler moves blocks it holds to be cold there, and they come back with an
                #  s_branch.  Such a block is followed like any other; a path that has left the loop for good runs into s_endpgm or the step limit.)
                pc = tgt
                continue
        assert pc != back, "the path falls out of the loop at listing line %d (the loop's last branch is not taken)" % no
        assert op != "s_endpgm", "the path leaves the loop and ends the kernel at listing line %d" % no
        pc += 1
    print("path: %d VALU, %.1f weighted issue cycles (%.2f per instruction)" % (n, cyc, cyc / n))
    for name, k in by.most_common():
        print("  %-28s %4d" % (name, k))
    print("opcodes:")
    for o, k in sorted(ops.items(), key=lambda t: (-t[1], t[0])):
        print("  %-28s %4d" % (o, k))


if __name__ == "__main__":
    main()
