#!/bin/bash
# Per-particle-map mode (SLAM.java's own shape) on the GPU box: bench.py --particle-maps at the two operating points, optionally
# under alternative settings.  usage: OUT=<dir> tools/pm_bench.sh <tag> [ENV=VALUE ...]   -> $OUT/<tag>_{500,500b180,4096}.json
tag=$1; shift
OUT=${OUT:?set OUT to the output directory}
mkdir -p "$OUT"
for spec in "500,6,90:500:50" "500,6,180:500b180:50" "4096,12.8,180:4096:20"; do
  IFS=: read cfg name steps <<< "$spec"
  env "$@" python bench.py --full --particle-maps $cfg --steps $steps --no-cpu-baseline --report "$OUT/${tag}_${name}_report.json" > "$OUT/${tag}_${name}.json" 2> "$OUT/${tag}_${name}.err" || tail -n 5 "$OUT/${tag}_${name}.err"
done
