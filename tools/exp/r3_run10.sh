#!/bin/bash
export TMPDIR=/tmp
OUT=${1:?usage: tools/exp/r3_run10.sh <output dir>}
mkdir -p $OUT
python -m pytest tests/test_parity_gpu.py -x -q -m gpu -k "draws or captured_product or cpp_autograd" 2>&1 | tail -15 > $OUT/tests.txt
python tools/exp/profile_eager.py > $OUT/profile_eager.txt 2>&1
python tools/host_overhead.py > $OUT/host_overhead.txt 2>&1
python bench.py --full --steps 200 --warmup 20 --no-cpu-baseline > $OUT/bench.json 2> $OUT/bench.err
python bench.py --full --steps 800 --warmup 20 --no-cpu-baseline > $OUT/bench800.json 2>> $OUT/bench.err
