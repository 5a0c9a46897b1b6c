#!/bin/bash
# physics parity tests, then bench.py --full at each V2P_ENVS_PER_BLOCK (debug builds): value and physics kernel ms -> $OUT_DIR/sweep.log
cd "$(dirname "$0")/.."; O=${OUT_DIR:-out}; mkdir -p $O; rm -f $O/sweep.log
timeout 600 python -m pytest tests/test_gpu_physics.py -m gpu -q -x 2>&1 | tail -15 > $O/pytest_phys.log
tail -5 $O/pytest_phys.log
for L in 8 4 16 32; do
  echo "envs_per_block=$L" >> $O/sweep.log
  V2P_DEBUG=1 V2P_ENVS_PER_BLOCK=$L timeout 300 python bench.py --full --steps 96 --warmup 32 --no-cpu-baseline 2>&1 | tail -1 | python -c "import sys,json; d=json.loads(sys.stdin.read()); print(d['value'], d['roofline']['kernel_ms'])" >> $O/sweep.log
done
cat $O/sweep.log
