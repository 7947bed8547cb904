#!/bin/bash
# Which roof bounds the adaptive-threshold kernels (adaptive.hip): instruction, LDS and memory counters around
# tools/bench_adaptive.py (T1 MEAN_C block 19, T2 GAUSSIAN_C block 19, N1 the composed default call: bit-plane output and
# k_adaptive_expand), one rocprofv3 --pmc run per counter set, no tracing beside it.  Memory is judged from the algorithmic
# bytes over kernel time (tools/bench_adaptive.py).
#   tools/pmc_adaptive.sh OUT_DIR      -> OUT_DIR/summary.txt
cd "$(dirname "$0")/.."
OUT=$(realpath -m "${1:?usage: tools/pmc_adaptive.sh OUT_DIR}"); rm -rf "$OUT"; mkdir -p "$OUT"; export TMPDIR=/tmp
for set in "SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAVES GRBM_GUI_ACTIVE" \
           "SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES GRBM_GUI_ACTIVE"; do
  tag=$(echo $set | cut -d' ' -f1)
  timeout -k 10 300 rocprofv3 --pmc $set --output-format csv -d "$OUT/$tag" -- \
      python3 tools/bench_adaptive.py --only T1,T2,N1 --steps 2 --warmup 1 --no-check > "$OUT/$tag.log" 2>&1 || exit $?
done
python3 - "$OUT" > "$OUT/summary.txt" <<'PY'
import csv, glob, os, re, sys
from collections import defaultdict
acc = defaultdict(lambda: defaultdict(list))
for f in glob.glob(os.path.join(sys.argv[1], "**", "*counter_collection.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        k = r.get("Kernel_Name", "")
        if "k_adaptive" not in k:
            continue
        m = re.search(r"k_adaptive(_\w+|<[^>]*>)?", k)
        name = m.group(0) if m else "k_adaptive"
        acc[name][r["Counter_Name"]].append(float(r["Counter_Value"]))
print("# per launch, summed over the chip (8 XCDs, 1024 SIMDs, 256 CUs); gui = GRBM_GUI_ACTIVE / 8 = the kernel's cycles")
print("# valu_util = SQ_INSTS_VALU x 2 cycles (one wave64 VALU instruction per SIMD-32 every 2 cycles at best) / (1024 x gui)")
print("# lds_util = SQ_LDS_IDX_ACTIVE / (256 x gui); valu_active = SQ_ACTIVE_INST_VALU / SQ_WAVE_CYCLES (share of wave time issuing VALU)")
for name, c in sorted(acc.items()):
    g = lambda n: (sum(c[n]) / len(c[n])) if c.get(n) else float("nan")
    gui = g("GRBM_GUI_ACTIVE") / 8
    print(f"{name:44s} launches={len(c['SQ_INSTS_VALU']):2d} gui_cycles={gui:10.4g} waves={g('SQ_WAVES'):9.3g} "
          f"valu={g('SQ_INSTS_VALU'):10.4g} lds_inst={g('SQ_INSTS_LDS'):10.4g} vmem_rd={g('SQ_INSTS_VMEM_RD'):9.3g} "
          f"vmem_wr={g('SQ_INSTS_VMEM_WR'):9.3g} valu_util={g('SQ_INSTS_VALU') * 2 / (1024 * gui):5.2f} "
          f"valu_active={g('SQ_ACTIVE_INST_VALU') / g('SQ_WAVE_CYCLES'):5.2f} lds_util={g('SQ_LDS_IDX_ACTIVE') / (256 * gui):5.2f} "
          f"bank_conflict={g('SQ_LDS_BANK_CONFLICT') / max(1.0, g('SQ_LDS_IDX_ACTIVE')):5.2f}")
PY
find "$OUT" -name "*.csv" -size +1M -delete
cat "$OUT/summary.txt"
