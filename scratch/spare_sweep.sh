#!/bin/bash
# build-variant sweep at the metric's size: shared objects in scratch/so/lib_<tag>.so; the bench lines go to $OUT (default: a new temporary directory)
out=${OUT:-$(mktemp -d)}; mkdir -p "$out"
cp imageclust_amd/libimageclust_hip.so /tmp/lib_keep.so
for v in "$@"; do
  cp scratch/so/lib_$v.so imageclust_amd/libimageclust_hip.so
  timeout -k 10 300 python3 bench.py --steps 2 --warmup 1 --full --no-cpu-baseline > $out/ss.json 2> $out/ss.err || { tail -c 800 $out/ss.err; break; }
  python3 -c "
import json; j=json.load(open('$out/ss.json')); print('$v', j['value'], j['ms_per_step'], j['stages_ms_last_step'], j['roofline']['avg_launch_us'])"
done
cp /tmp/lib_keep.so imageclust_amd/libimageclust_hip.so
