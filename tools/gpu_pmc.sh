#!/bin/bash
export TMPDIR=/tmp
out=${OUT_DIR:-results}  # where the outputs go
mkdir -p $out
for ctr in FETCH_SIZE WRITE_SIZE; do
  rm -rf $out/pmc_$ctr
  timeout 300 rocprofv3 --pmc $ctr --kernel-trace --output-format csv -d $out/pmc_$ctr -o p -- python tools/pmc_workload.py > $out/pmc_$ctr.log 2>&1; echo "$ctr rc=$?"
done
ls $out/pmc_FETCH_SIZE $out/pmc_WRITE_SIZE
timeout 400 python bench.py --full > $out/bench_default.json 2> $out/bench_default.err; echo "bench rc=$?"
cat $out/bench_default.json
timeout 300 python -m pytest tests/test_gpu_factor.py -m gpu -q -x -k dist 2>&1 | tail -3
