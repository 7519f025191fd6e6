#!/bin/bash
# One visit to a GPU box: parity tests, the bench line, kernel-trace profiles (csv summaries) of every workload.
#   gpurun --timeout 1500 -- 'bash tools/gpu_round.sh r01_final'
tag=${1:-run}
export TMPDIR=/tmp
out=${OUT_DIR:-results}  # where the outputs go
mkdir -p $out
timeout 1500 python -m pytest tests -m gpu -q > $out/pytest_gpu.log 2>&1; echo "pytest rc=$?"
tail -3 $out/pytest_gpu.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -1
timeout 300 python tools/gpu_fuzz.py 300 7 2>&1 | tail -1
timeout 600 python bench.py --full > $out/${tag}_bench.json 2> $out/${tag}_bench.err; echo "bench rc=$?"
cat $out/${tag}_bench.json
for wl in ${PROF_WORKLOADS:-gemm llt lu qr tridiag}; do
  rm -rf $out/prof_${tag}_$wl
  timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_${tag}_$wl -o $wl -- python bench.py --full --workload $wl --steps 10 --warmup 2 --no-extras --no-cpu > $out/prof_${tag}_$wl.log 2>&1; echo "prof $wl rc=$?"
  grep -o '"ms_per_step": [0-9.]*' $out/prof_${tag}_$wl.log
done
