#!/bin/bash
# A/B of the update kernel's two bodies at the metric's size and at configs[4]; the bench lines go to $OUT (default: a new temporary directory)
out=${OUT:-$(mktemp -d)}; mkdir -p "$out"
for n in 100000 250000; do
 for m in bound lwbound; do
  timeout -k 10 400 python3 bench.py --full --no-cpu-baseline --steps 2 --warmup 1 --total-images $n --ward-dist $m > $out/ab_${n}_$m.json 2> $out/ab.err || { tail -c 800 $out/ab.err; exit 1; }
  python3 -c "
import json; j=json.load(open('$out/ab_${n}_$m.json')); print($n, '$m', j['value'], j['ms_per_step'], j['stages_ms_last_step'], j['roofline']['avg_launch_us'])"
 done
done
