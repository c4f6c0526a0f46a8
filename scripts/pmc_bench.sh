#!/bin/bash
# HBM traffic of the bench kernels: FETCH_SIZE and WRITE_SIZE in separate PMC passes over a short bench run.  Output lands in $STORM_OUT (default: bench_out/).
TAG=${1:-pmcb}
OUT=${STORM_OUT:-bench_out}
export TMPDIR=/tmp
mkdir -p $OUT/$TAG
for c in FETCH_SIZE WRITE_SIZE; do
  timeout 900 rocprofv3 --kernel-trace --pmc $c --output-format csv -d $OUT/$TAG/$c -o p -- python bench.py --full --steps 1 --warmup 0 --N 2 --no-cpu-baseline --no-roofline > $OUT/$TAG/$c.log 2>&1
done
f=$(find $OUT/$TAG/FETCH_SIZE -name "*counter_collection.csv" | head -1); w=$(find $OUT/$TAG/WRITE_SIZE -name "*counter_collection.csv" | head -1)
python tools/pmc_traffic.py $f $w $OUT/$TAG/conv_traffic.json
find $OUT/$TAG -name "*kernel_trace.csv" -delete
