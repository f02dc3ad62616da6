"""Turn the files of measure.sh into speed.md.  Usage: summarise.py BENCH_DIR TRACE_DIR > speed.md"""
import csv
import glob
import json
import os
import re
import sys

# (parent's name, branch's name) of the five hot kernels of the merge stage
HOT = (("set_bits4_multi_kernel", "set_bits_kernel<true>"), ("dilate_bits_disk2_kernel",) * 2, ("bitrun_tile_kernel",) * 2,
       ("bitrun_border_kernel",) * 2, ("merge_fused_kernel", "merge_groups_kernel<pcseg::RunRoots, true>"))


def med(v):
    v = sorted(v)
    return (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2


def runs(d, pattern):
    return [json.load(open(p))["ms_per_step"] for p in sorted(glob.glob(os.path.join(d, pattern)))]


def kernel_stats(d):
    out = {}
    for p in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(p)):
            name = re.sub(r"\(.*$", "", row["Name"]).replace("void ", "")
            name = name[len("pcseg::"):] if name.startswith("pcseg::") else name
            out[name] = dict(calls=int(row["Calls"]), mean=float(row["AverageNs"]) / 1e3, lo=float(row["MinNs"]) / 1e3,
                             hi=float(row["MaxNs"]) / 1e3, sd=float(row["StdDev"]) / 1e3)
    return out


def main(bench_dir, trace_dir):
    ok = True
    parent, child = runs(bench_dir, "bench_parent_*.json"), runs(bench_dir, "bench_child_*.json")
    good = med(child) <= max(parent)
    ok = ok and good
    print("# Speed against the parent commit 118c8f9 (one machine; bench and traces in sessions of their own)\n")
    print("## Headline: `bench.py --gpus 1 --steps 20 --warmup 4 --no-cpu-baseline`, order c p p c c p p c\n")
    print("| | runs (ms/step) | median |\n|---|---|---|")
    print("| parent | %s | %.4g |" % (", ".join("%.4g" % x for x in parent), med(parent)))
    print("| branch | %s | %.4g |" % (", ".join("%.4g" % x for x in child), med(child)))
    print("\nCondition `median(branch) <= max(parent)` (%.4g <= %.4g): **%s**.\n" % (med(child), max(parent), "holds" if good else "FAILS"))
    a, b = kernel_stats(os.path.join(trace_dir, "trace_parent")), kernel_stats(os.path.join(trace_dir, "trace_branch"))
    print("## The five hot kernels, per launch (`rocprofv3 --kernel-trace --stats`, trace_driver.py)\n")
    print("| kernel (branch's name) | calls | parent mean (us) | parent min .. max | branch mean (us) | rise | allowed (parent max - min) | |")
    print("|---|---|---|---|---|---|---|---|")
    for old, new in HOT:
        x, y = a[old], b[new]
        good = y["mean"] - x["mean"] <= x["hi"] - x["lo"]
        ok = ok and good
        print("| `%s` | %d | %.1f | %.1f .. %.1f | %.1f | %+.1f | %.1f | %s |"
              % (new.replace("pcseg::", ""), y["calls"], x["mean"], x["lo"], x["hi"], y["mean"], y["mean"] - x["mean"], x["hi"] - x["lo"],
                 "holds" if good else "**FAILS**"))
    up, uc = (json.load(open(os.path.join(bench_dir, "unfused_%s.json" % k))) for k in ("parent", "child"))
    print("\n## Entry points off the benchmark path: test_merge_groups' calls (time_unfused.py, median of 50, us; no condition)\n")
    print("Lists of %s entries, %s groups.\n\n| call | parent | branch |\n|---|---|---|" % (uc["list"], uc["groups"]))
    for k in uc:
        if k.endswith("_us"):
            print("| `%s` | %.1f | %.1f |" % (k[:-3], up[k], uc[k]))
    assert up["groups"] == uc["groups"]
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
