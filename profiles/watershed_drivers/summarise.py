"""Turn the files of measure.sh into speed.md.  Usage: summarise.py BENCH_DIR TRACE_DIR > speed.md"""
import csv
import glob
import json
import os
import re
import sys

# the relaxation's and the label assignment's kernels (the parent's names carry <64> on the first three)
HOT = ("ws_relax_kernel", "ws_relax_list_kernel", "ws_relax_tail_kernel", "ws_k2_relax_kernel", "ws_k2_relax_tail_kernel",
       "ws_uf_tile_kernel", "ws_uf_label4_kernel")


def med(v):
    v = sorted(v)
    return (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2


def runs(d, pattern):
    return [json.load(open(p))["ms_per_step"] for p in sorted(glob.glob(os.path.join(d, pattern)))]


def kernel_stats(d):
    """name (the parent's <64> dropped, other template arguments kept) -> calls, mean, min, max in us"""
    out = {}
    for p in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(p)):
            name = re.sub(r"\(.*$", "", row["Name"]).replace("void ", "").replace("pcseg::", "").replace("<64>", "")
            out[name] = dict(calls=int(row["Calls"]), mean=float(row["AverageNs"]) / 1e3, lo=float(row["MinNs"]) / 1e3,
                             hi=float(row["MaxNs"]) / 1e3)
    return out


def main(bench_dir, trace_dir):
    parent, child = runs(bench_dir, "bench_parent_*.json"), runs(bench_dir, "bench_child_*.json")
    ok = med(child) <= max(parent)
    print("# Speed against the parent commit 0c66b24 (one machine; bench and traces in sessions of their own)\n")
    print("## Headline: `bench.py --gpus 1 --steps 20 --warmup 4 --no-cpu-baseline`, order c p p c c p p c\n")
    print("| | runs (ms/step) | median |\n|---|---|---|")
    print("| parent | %s | %.4g |" % (", ".join("%.4g" % x for x in parent), med(parent)))
    print("| branch | %s | %.4g |" % (", ".join("%.4g" % x for x in child), med(child)))
    print("\nCondition `median(branch) <= max(parent)` (%.4g <= %.4g): **%s**.\n" % (med(child), max(parent), "holds" if ok else "FAILS"))
    a, b = kernel_stats(os.path.join(trace_dir, "trace_parent")), kernel_stats(os.path.join(trace_dir, "trace_branch"))
    print("## The watershed's hot kernels, per launch (`rocprofv3 --kernel-trace --stats`, trace_driver.py)\n")
    print("Every instantiation on a row of its own.  Condition: branch mean - parent mean <= parent max - min.\n")
    print("| kernel | calls | parent mean (us) | parent min .. max | branch mean (us) | rise | allowed (parent max - min) | |")
    print("|---|---|---|---|---|---|---|---|")
    for k in sorted(n for n in a if n in HOT or n.split("<")[0] in HOT):
        x, y = a[k], b[k]
        good = y["mean"] - x["mean"] <= x["hi"] - x["lo"] and x["calls"] == y["calls"]
        ok = ok and good
        print("| `%s` | %d | %.1f | %.1f .. %.1f | %.1f | %+.1f | %.1f | %s |"
              % (k, y["calls"], x["mean"], x["lo"], x["hi"], y["mean"], y["mean"] - x["mean"], x["hi"] - x["lo"], "holds" if good else "**FAILS**"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
