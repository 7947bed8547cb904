#!/bin/bash
# kernel trace of the worst-case legs (literal pages, adversarial stripes) after the headline steps:
#   tools/dbg/adv_trace.sh <output dir, relative to the repository root>
OUT=${1:?usage: tools/dbg/adv_trace.sh <output dir>}
cd "$(dirname "$0")/../.." && mkdir -p "$OUT" && export TMPDIR=/tmp
rocprofv3 --kernel-trace --output-format csv -d "$OUT/t" -- python3 bench.py --full --steps 2 --warmup 1 --end-to-end 0 --traffic 0 --cpu-seconds 0 --check-pages 0 > "$OUT/bench.json" 2> "$OUT/bench.err"
python3 - "$OUT" <<'PY'
import csv,glob,os,sys
f=glob.glob(os.path.join(sys.argv[1],'t','**','*kernel_trace.csv'),recursive=True)[0]
rows=list(csv.DictReader(open(f)))
rows.sort(key=lambda r:int(r['Start_Timestamp']))
t0=int(rows[0]['Start_Timestamp'])
out=open(os.path.join(sys.argv[1],'last_kernels.txt'),'w')
for r in rows[-60:]:
    out.write(f"{(int(r['Start_Timestamp'])-t0)/1e3:12.1f} us  {(int(r['End_Timestamp'])-int(r['Start_Timestamp']))/1e3:9.1f} us  grid {r['Grid_Size_X']:>9} wg {r['Workgroup_Size_X']:>5}  {r['Kernel_Name'][:90]}\n")
PY
tail -45 "$OUT/last_kernels.txt"
