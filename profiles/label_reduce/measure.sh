#!/bin/bash
# One measuring session against the parent commit: measure.sh OUT_DIR, from the repository root, with the parent's library
# built into ab/parent (build.build(out_dir="ab/parent") on a checkout of the parent) and this tree's library built in place.
# Eight alternating bench.py runs, six alternating runs of the changed path, one kernel trace per library; every step has
# a time limit of its own and a failed step ends the session.  summarise.py OUT_DIR then writes speed.md and kernels.md.
set -o pipefail
O=${1:?output directory}
mkdir -p $O
P=$PWD/ab/parent/libpcseg.so
bench() {  # name, lib ("" = branch)
  if [ -n "$2" ]; then PCSEG_LIB=$2 timeout -k 10 200 python bench.py --gpus 1 --steps 20 --warmup 4 --no-cpu-baseline 2>$O/$1.err | tail -1 > $O/$1.json
  else timeout -k 10 200 python bench.py --gpus 1 --steps 20 --warmup 4 --no-cpu-baseline 2>$O/$1.err | tail -1 > $O/$1.json; fi
}
unal() {
  if [ -n "$2" ]; then PCSEG_LIB=$2 timeout -k 10 90 python profiles/label_reduce/time_unaligned.py > $O/$1.json 2>$O/$1.err
  else timeout -k 10 90 python profiles/label_reduce/time_unaligned.py > $O/$1.json 2>$O/$1.err; fi
}
bench bench_child_1 "" && echo c1 && bench bench_parent_1 $P && echo p1 && bench bench_parent_2 $P && echo p2 && bench bench_child_2 "" && echo c2 &&
bench bench_child_3 "" && echo c3 && bench bench_parent_3 $P && echo p3 && bench bench_parent_4 $P && echo p4 && bench bench_child_4 "" && echo c4 &&
unal unaligned_child_1 "" && unal unaligned_parent_1 $P && unal unaligned_parent_2 $P && unal unaligned_child_2 "" &&
unal unaligned_child_3 "" && unal unaligned_parent_3 $P && echo unaligned done &&
PCSEG_LIB=$P timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_parent -- python profiles/label_reduce/trace_driver.py > $O/trace_parent.log 2>&1 && echo trace parent &&
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_branch -- python profiles/label_reduce/trace_driver.py > $O/trace_branch.log 2>&1 && echo trace branch
rc=$?
find $O -name "*kernel_trace.csv" -delete; find $O -name "*.db" -delete
grep -h ms_per_step $O/bench_*.json | sed 's/.*"ms_per_step": \([0-9.]*\).*/\1/' | paste -sd' '
cat $O/unaligned_*.json
exit $rc
