#!/bin/bash
# measure.sh bench|ragged|one OUT_DIR, from the repository root: the parent's library (ab/parent/libpcseg.so, from
# build.build(out_dir="ab/parent") on a checkout of the parent) and this tree's alternating p b p b p b in one session;
# every run has a time limit of its own and a failed run ends the session
set -o pipefail
M=${1:?bench, ragged or one}
O=${2:?output directory}; mkdir -p $O
P=$PWD/ab/parent/libpcseg.so
run() {  # name, lib ("" = branch)
  if [ $M = bench ]; then C="python bench.py --gpus 1 --steps 20 --warmup 4 --no-cpu-baseline"
  else C="python profiles/plane_sums/time_routes.py --route $M"; fi
  if [ -n "$2" ]; then PCSEG_LIB=$2 PYTHONPATH=$PWD timeout -k 10 200 $C 2>$O/$1.err | tail -1 > $O/$1.json
  else PYTHONPATH=$PWD timeout -k 10 200 $C 2>$O/$1.err | tail -1 > $O/$1.json; fi
}
run ${M}_parent_1 $P && echo p1 && run ${M}_branch_1 "" && echo b1 && run ${M}_parent_2 $P && echo p2 && run ${M}_branch_2 "" && echo b2 &&
run ${M}_parent_3 $P && echo p3 && run ${M}_branch_3 "" && echo b3
rc=$?
for f in $O/${M}_*.json; do echo $f; cut -c1-400 $f; done
echo "job exit $rc"; exit $rc
