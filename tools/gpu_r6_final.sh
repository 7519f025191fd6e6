#!/bin/bash
# Final visit of round 6: default bench line, one-rank dry runs of the distributed drivers, kernel summaries and timelines of the
# workloads that changed at the end of the round.   gpurun --timeout 1500 -- 'bash tools/gpu_r6_final.sh'
export TMPDIR=/tmp
out=${OUT_DIR:-results}  # where the outputs go
mkdir -p $out
timeout 900 python bench.py --full > $out/r06f_bench.json 2> $out/r06f_bench.err; echo "bench rc=$?"
BENCH_FORCE_DIST=1 timeout 400 python bench.py --full --no-cpu > $out/r06f_dist_lu.json 2> $out/r06f_dist_lu.err; echo "dist lu rc=$?"
BENCH_FORCE_DIST=1 timeout 400 python bench.py --full --workload llt --no-cpu > $out/r06f_dist_llt.json 2> $out/r06f_dist_llt.err; echo "dist llt rc=$?"
for f in r06f_bench r06f_dist_lu r06f_dist_llt; do python - $out/$f.json <<PY
import json,sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
o=d.get("others",{})
print(sys.argv[1], d["config"]["workload"], d["ms_per_step"], d.get("speedup_vs_1gpu_same_run"), {k:(v.get("ms") if isinstance(v,dict) else v) for k,v in o.items()})
PY
done
bash tools/gpu_visit.sh r06f prof:llt prof:fplu qrprof > $out/r06f_prof.log 2>&1; grep -E "rc=|ms_per_step" $out/r06f_prof.log
f=$(find $out/prof_r06f_llt -name "*kernel_trace.csv" | head -1); python tools/trace_timeline.py $f > $out/r06f_llt_timeline.txt 2>&1
f=$(find $out/prof_r06f_qr -name "*kernel_trace.csv" | head -1); python tools/qr_tail_timeline.py $f > $out/r06f_qr_timeline.txt 2>&1; tail -1 $out/r06f_qr_timeline.txt
bash tools/gpu_dllt_trace.sh 512 40000 46000 rccl > $out/r06f_dllt_trace.log 2>&1; cp $out/dllt_timeline.txt $out/r06f_dist_llt_timeline.txt; head -3 $out/dllt_timeline.txt
