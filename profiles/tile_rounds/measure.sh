#!/bin/bash
# measure.sh bench|rec OUT_DIR, from the repository root: parent (ab/parent/libpcseg.so) and branch alternating, three runs each, in one session
set -o pipefail
M=${1:?bench or rec}
O=${2:?output directory}; mkdir -p $O
P=$PWD/ab/parent/libpcseg.so
run() {  # name, lib ("" = branch)
  if [ $M = bench ]; then C="python bench.py --gpus 1 --steps 20 --warmup 4 --no-cpu-baseline"
  else C="python profiles/reconstruct/step_time.py --marker-h 1.0 --tag $1"; fi
  if [ -n "$2" ]; then PCSEG_LIB=$2 PYTHONPATH=$PWD timeout -k 10 200 $C 2>$O/$1.err | tail -1 > $O/$1.json
  else PYTHONPATH=$PWD timeout -k 10 200 $C 2>$O/$1.err | tail -1 > $O/$1.json; fi
}
run parent_1 $P && echo p1 && run branch_1 "" && echo b1 && run parent_2 $P && echo p2 && run branch_2 "" && echo b2 &&
run parent_3 $P && echo p3 && run branch_3 "" && echo b3
rc=$?
for f in $O/*.json; do echo $f; cut -c1-400 $f; done
echo "job exit $rc"; exit $rc
