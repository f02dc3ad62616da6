#!/bin/bash
# twelfth GPU call of round 4: GPU tests on the tree (EDT row with clamped bases, EDT reach as in round 3, label pass at three
# quads), then ABLATION builds timed stage by stage (profiles/r04/time_ops.py): the watershed's union-find tile pass without its
# vertical unions (1), without its final finds (2), without both (3); the front end without its median (1), without its tile
# unions (2), without both (3); then the default bench three times
O=$GRAFT_REPO_ROOT/gpurun_out/r4l; mkdir -p $O; cd $GRAFT_REPO_ROOT
step() {
  local name=$1 t=$2; shift 2
  echo "=== $name"; timeout -k 10 $t "$@" > $O/$name.log 2> $O/$name.err; local rc=$?
  echo "=== $name rc=$rc"; tail -3 $O/$name.log
  if [ $rc -ge 124 ]; then echo "killed: stopping"; exit $rc; fi
}
step pytest 600 python -m pytest tests -m gpu -x -q
lib() { [ "$1" = main ] && echo "" || echo "$GRAFT_REPO_ROOT/ab/$1/libpcseg.so"; }
for V in main uft1 uft2 uft3 main; do
  PCSEG_LIB=$(lib $V) step refine_$V 200 python profiles/r04/time_ops.py refine 4
  echo "== refine $V"; grep -E "ws_uf_tile|ws_uf_border|ws_uf_label4|ws_relax_kernel" $O/refine_$V.log
done
for V in main fe1 fe2 fe3 main; do
  PCSEG_LIB=$(lib $V) step classmap_$V 200 python profiles/r04/time_ops.py classmap 6
  echo "== classmap $V"; grep -E "classmap_median|ccl_border|relabel" $O/classmap_$V.log
done
Q="--no-shape-legs --no-cpu-baseline --secondary-batch 0 --batch64-frames 0 --graph-leg-steps 0 --no-end-to-end"
step serial 200 python bench.py $Q --full --serial --steps 6 --kernel-table
head -45 $O/serial.err
for rep in 1 2 3; do
  step bench_$rep 200 python bench.py $Q
  python3 -c "import json;d=json.load(open('$O/bench_$rep.log'));print('== overlapped main', d['ms_per_step'], d['value'])"
done
