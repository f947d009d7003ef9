#!/bin/bash
# HBM write bytes of stage A by store form:  bash tools/pmc_compat_writes.sh   (one rocprofv3 --pmc WRITE_SIZE pass per variant — FETCH_SIZE needs a pass of its own —, kernel-trace only)
set -u
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$R/gpurun_out/pmcw
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
i=0
for V in "" "--debug compat_rows=32" "--debug compat_store_mode=4" "--debug compat_store_mode=1" "--no-dense-s" "--debug compat_one_phase=1"; do
  i=$((i+1))
  timeout -k 10 90 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d "$OUT/v$i" -- \
    python3 "$R/bench.py" --config C2 --steps 3 --warmup 1 --full --headline-only $V > "$OUT/v$i.log" 2>&1 || { echo "variant $V failed"; tail -5 "$OUT/v$i.log"; exit 1; }
  python3 - "$OUT/v$i" "$V" <<'PY'
import csv, glob, sys, collections
acc = collections.defaultdict(list); dur = []
for f in glob.glob(sys.argv[1] + "/**/*counter_collection.csv", recursive=True):
    for row in csv.DictReader(open(f)):
        if "compat_tiles_kernel" in row["Kernel_Name"]:
            acc[row["Counter_Name"]].append(float(row["Counter_Value"]))
for f in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
    for row in csv.DictReader(open(f)):
        if "compat_tiles_kernel" in row["Kernel_Name"]:
            dur.append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1000)
a = {k: sum(v) / len(v) for k, v in acc.items()}
print(f"variant [{sys.argv[2]:28s}] us {sum(dur)/max(1,len(dur)):6.1f}  WRITE {a.get('WRITE_SIZE',0)*1024/1e6:7.1f} MB")
PY
done
