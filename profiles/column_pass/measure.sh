#!/bin/bash
# Measuring against the parent commit, the method of profiles/merge_paths/measure.sh: from the repository root, with the
# parent's library built into ab/parent (build.build(out_dir="ab/parent") on a checkout of the parent) and this tree's
# library built in place.
#   measure.sh bench OUT_DIR     eight alternating bench.py runs (c p p c c p p c)
#   measure.sh kernels OUT_DIR   time_transforms.py twice per library, alternating (c p p c)
# Every step has a time limit of its own and a failed step ends the session.  summarise.py OUT_DIR writes speed.md.
set -o pipefail
M=${1:?bench or kernels}
O=${2:?output directory}
mkdir -p $O
P=$PWD/ab/parent/libpcseg.so
bench() {  # name, lib ("" = branch)
  if [ -n "$2" ]; then PCSEG_LIB=$2 timeout -k 10 200 python bench.py --gpus 1 --steps 20 --warmup 4 --no-cpu-baseline 2>$O/$1.err | tail -1 > $O/$1.json
  else timeout -k 10 200 python bench.py --gpus 1 --steps 20 --warmup 4 --no-cpu-baseline 2>$O/$1.err | tail -1 > $O/$1.json; fi
}
kernels() {  # name, lib ("" = branch)
  if [ -n "$2" ]; then PCSEG_LIB=$2 timeout -k 10 120 python profiles/column_pass/time_transforms.py $O/$1.json > $O/$1.log 2>&1
  else timeout -k 10 120 python profiles/column_pass/time_transforms.py $O/$1.json > $O/$1.log 2>&1; fi
}
if [ $M = bench ]; then
  bench bench_child_1 "" && echo c1 && bench bench_parent_1 $P && echo p1 && bench bench_parent_2 $P && echo p2 && bench bench_child_2 "" && echo c2 &&
  bench bench_child_3 "" && echo c3 && bench bench_parent_3 $P && echo p3 && bench bench_parent_4 $P && echo p4 && bench bench_child_4 "" && echo c4
  rc=$?
  grep -h ms_per_step $O/bench_*.json | sed 's/.*"ms_per_step": \([0-9.]*\).*/\1/' | paste -sd' '
else
  kernels kernels_child_1 "" && echo c1 && kernels kernels_parent_1 $P && echo p1 && kernels kernels_parent_2 $P && echo p2 &&
  kernels kernels_child_2 "" && echo c2
  rc=$?
  cat $O/kernels_*.json
fi
exit $rc
