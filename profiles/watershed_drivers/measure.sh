#!/bin/bash
# Measuring against the parent commit, the method of profiles/merge_paths/measure.sh: from the repository root, with the
# parent's library built into ab/parent (build.build(out_dir="ab/parent") on a checkout of the parent) and this tree's
# library built in place.
#   measure.sh bench OUT_DIR      eight alternating bench.py runs (c p p c c p p c)
#   measure.sh trace OUT_DIR      one kernel trace of trace_driver.py per library (a session of its own: no other tracing, no counters)
#   measure.sh launches OUT_DIR   one kernel trace of launch_driver.py per library, kept whole for launches.py
# Every step has a time limit of its own and a failed step ends the session.  summarise.py OUT_DIR OUT_DIR writes speed.md.
set -o pipefail
M=${1:?bench, trace or launches}
O=${2:?output directory}
mkdir -p $O
P=$PWD/ab/parent/libpcseg.so
D=profiles/watershed_drivers
bench() {  # name, lib ("" = branch)
  if [ -n "$2" ]; then PCSEG_LIB=$2 timeout -k 10 200 python bench.py --gpus 1 --steps 20 --warmup 4 --no-cpu-baseline 2>$O/$1.err | tail -1 > $O/$1.json
  else timeout -k 10 200 python bench.py --gpus 1 --steps 20 --warmup 4 --no-cpu-baseline 2>$O/$1.err | tail -1 > $O/$1.json; fi
}
trace() {  # driver, name, lib ("" = branch)
  if [ -n "$3" ]; then PCSEG_LIB=$3 timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $O/$2 -- python $D/$1 > $O/$2.log 2>&1
  else timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $O/$2 -- python $D/$1 > $O/$2.log 2>&1; fi
}
if [ $M = bench ]; then
  bench bench_child_1 "" && echo c1 && bench bench_parent_1 $P && echo p1 && bench bench_parent_2 $P && echo p2 && bench bench_child_2 "" && echo c2 &&
  bench bench_child_3 "" && echo c3 && bench bench_parent_3 $P && echo p3 && bench bench_parent_4 $P && echo p4 && bench bench_child_4 "" && echo c4
  rc=$?
  grep -h ms_per_step $O/bench_*.json | sed 's/.*"ms_per_step": \([0-9.]*\).*/\1/' | paste -sd' '
elif [ $M = trace ]; then
  trace trace_driver.py trace_parent $P && echo trace parent && trace trace_driver.py trace_branch "" && echo trace branch
  rc=$?
  find $O -name "*kernel_trace.csv" -delete; find $O -name "*.db" -delete
else
  trace launch_driver.py launches_parent $P && echo launches parent && trace launch_driver.py launches_branch "" && echo launches branch
  rc=$?
  find $O -name "*.db" -delete
fi
exit $rc
