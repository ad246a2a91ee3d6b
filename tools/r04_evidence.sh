#!/bin/bash
# Round-4 evidence on ONE box, final build: the driver's own command three times (once under rocprofv3 --kernel-trace --stats),
# the paced real-time run under the kernel trace, the counter passes of the chain kernels (cfg5 / cfg3 / cfg2) and of config 4 on
# the default (two-part f16) sweep.  Everything lands under gpurun_out/r04ev/; summaries are copied into profiles/ (names r04_*).
set -u
ROOT=/root/repo
export DSPFX_ROUND=r04
OUT=$ROOT/gpurun_out/r04ev; rm -rf $OUT; mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
python3 $ROOT/bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/bench_run1.json 2>$OUT/bench_run1.err
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o drv -- python3 $ROOT/bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/bench_under_rocprof.json 2>$OUT/rocprof.err
python3 $ROOT/bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/bench_run2.json 2>$OUT/bench_run2.err
T=$(find $OUT/trace -name "*kernel_trace.csv" | head -1)
python3 $ROOT/tools/trace_phases.py $T $OUT/bench_under_rocprof.json $OUT/timed_regions.json > $OUT/timed_regions.txt 2>&1
cp $(find $OUT/trace -name "*kernel_stats.csv" | head -1) $OUT/kernel_stats.csv
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/paced_trace -o paced -- python3 $ROOT/bench.py --gpus 1 --steps 20 --warmup 5 --paced > $OUT/bench_paced_under_rocprof.json 2>$OUT/paced_rocprof.err
python3 - <<PY > $OUT/paced_kernel.txt 2>&1
import csv, glob, statistics
f = glob.glob("$OUT/paced_trace/**/*kernel_trace.csv", recursive=True)[0]
rows = [r for r in csv.DictReader(open(f)) if "chain_kernel" in r["Kernel_Name"]]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
d, last_end = [], None
for r in rows:                      # the paced launches are the ones whose predecessor ended more than 1 ms earlier
    s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    if last_end is not None and s - last_end > 1_000_000:
        d.append((e - s) / 1e3)
    last_end = e
d.sort()
print("paced launches (gap before > 1 ms): %d  kernel us: min %.1f  p50 %.1f  p99 %.1f  max %.1f  mean %.1f" % (
    len(d), d[0], d[len(d) // 2], d[int(len(d) * 0.99)], d[-1], statistics.mean(d)))
PY
rm -rf $OUT/trace/*/*.db $OUT/paced_trace/*/*.db 2>/dev/null
rm -rf $OUT/paced_trace
find $OUT/trace -name "*kernel_trace.csv" -size +20M -delete
cd $ROOT
bash tools/pmc_chain.sh > $OUT/pmc.txt 2>&1
tail -3 $OUT/timed_regions.txt; cat $OUT/paced_kernel.txt; tail -4 $OUT/pmc.txt
bash tools/fir_pmc.sh r04half > $OUT/firpmc_half.txt 2>&1
python3 tools/fir_pmc_report.py gpurun_out/firpmc_r04half r04 --kernel fir_half_kernel > $OUT/r04_fir_half_pmc.json 2>$OUT/firpmc_half_report.err
find gpurun_out/firpmc_r04half -name "*kernel_trace.csv" -size +8M -delete 2>/dev/null
find gpurun_out/firpmc_r04half gpurun_out/pmc_chain -name "*.db" -delete 2>/dev/null
head -12 $OUT/r04_fir_half_pmc.json
python3 - <<PY
import json
for f in ("bench_run1", "bench_under_rocprof", "bench_run2"):
    try:
        d = json.loads(open("$OUT/%s.json" % f).read().strip().splitlines()[-1])
        oc = d.get("other_configs", {})
        print(f, "ms/step %.4f frac %.3f by_step %.3f |" % (d["ms_per_step"], d["roofline"]["frac"], d["roofline"].get("frac_by_step", 0)),
              " ".join("%s %.4f/%.4f" % (k, v.get("ms_per_step", 0), v.get("kernel_ms_avg", 0)) for k, v in oc.items()),
              "| paced", d.get("paced", {}).get("latency_ms"))
    except Exception as ex:
        print(f, "unreadable:", ex)
PY
