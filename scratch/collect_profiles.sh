#!/bin/bash
# Profiles behind bench.py's roofline object, taken THROUGH bench.py itself (the launch path of the timed region: hipGraph
# replay of the merge loop, two embed streams): one --kernel-trace --stats run and two separate --pmc passes
# (FETCH_SIZE / WRITE_SIZE cannot share a pass: MI355X_MICROARCH.md "rocprofv3 PMC slots").  Usage (on the GPU box):
#   bash scratch/collect_profiles.sh <tag> [bench args...]      outputs -> $OUT/<tag>/ (default: profile_out/<tag>/)
# bench.py runs with --full: the untimed profiling passes behind its roofline objects are part of every profiled run.
tag=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
out=${OUT:-$R/profile_out}/$tag; mkdir -p $out; cd /tmp; export TMPDIR=/tmp
step() { # name, rocprof flags...
  name=$1; shift
  timeout -k 10 420 rocprofv3 "$@" --output-format csv -d $out/$name -- python3 $R/bench.py --full --no-cpu-baseline "${BENCH_ARGS[@]}" > $out/$name.json 2> $out/$name.err
  rc=$?; echo "$name rc=$rc" | tee -a $out/steps.log
  [ $rc -eq 124 -o $rc -eq 137 ] && { echo "killed: stopping" | tee -a $out/steps.log; exit 1; }
  return 0
}
BENCH_ARGS=("$@")
step stats --kernel-trace --stats
step pmc_fetch --kernel-trace --pmc FETCH_SIZE
step pmc_write --kernel-trace --pmc WRITE_SIZE
python3 $R/scratch/pmc_summary.py $out > $out/pmc_summary.json
# keep the summaries, drop the per-dispatch traces (tens of MB each)
cp $out/stats/*/*_kernel_stats.csv $out/kernel_stats.csv 2>/dev/null
rm -rf $out/stats $out/pmc_fetch $out/pmc_write
cat $out/steps.log
