#!/bin/bash
# SQ counters of kmer_hash_kernel over one bench.py step at config 3, in a counter pass of its own (no tracing beside it): bash tools/pmc_kmer_hash.sh <out.csv>
# VALU per wave = SQ_INSTS_VALU / SQ_WAVES; a workgroup of four waves owns 64 records (profiles/r12a_pmc_kmer_hash*.csv)
OUT=${1:-pmc_kmer_hash.csv}
R=$(cd "$(dirname "$0")/.." && pwd); D=$(mktemp -d)
( cd "$D" && timeout -k 10 500 rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES SQ_ACTIVE_INST_VALU SQ_INSTS_LDS SQ_INSTS_SALU SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_INST_ANY --output-format csv -d "$D/pmc" -o p -- \
    python "$R/bench.py" --steps 1 --warmup 1 --no-cpu-baseline --no-extras > "$D/bench.log" 2>&1 ) || { tail -5 "$D/bench.log"; exit 1; }
python - "$D/pmc" "$OUT" <<'PY'
import collections, csv, glob, sys
agg = collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob(sys.argv[1] + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if "kmer_hash_kernel" in r["Kernel_Name"]:
            agg[(r["Kernel_Name"].split("(")[0], r.get("Grid_Size", ""), r.get("Workgroup_Size", ""))][r["Counter_Name"]].append(float(r["Counter_Value"]))
with open(sys.argv[2], "w") as o:
    o.write("kernel,grid_size,workgroup_size,counter,dispatches,mean_per_dispatch\n")
    for k, v in sorted(agg.items()):
        for c, vals in sorted(v.items()):
            o.write('"%s",%s,%s,%s,%d,%.0f\n' % (k[0], k[1], k[2], c, len(vals), sum(vals) / len(vals)))
print(open(sys.argv[2]).read())
PY
rm -rf "$D"
