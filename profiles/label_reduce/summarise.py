"""Turn one measuring session's files into speed.md and kernels.md.

Usage: summarise.py DIR   (DIR holds bench_{child,parent}_{1..4}.json, unaligned_{child,parent}_*.json and
trace_{parent,branch}/**/*kernel_stats.csv as rocprofv3 --kernel-trace --stats wrote them)."""
import csv
import glob
import json
import os
import re
import sys

KERNELS = ("region_stats_col_kernel", "region_reduce_col_kernel", "region_sums2_col_kernel", "lp_count_kernel", "shape_moments_kernel",
           "shape_perimeter_kernel", "region_reduce_kernel")


def med(v):
    v = sorted(v)
    return (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2


def runs(d, pattern, key):
    return [json.load(open(p))[key] for p in sorted(glob.glob(os.path.join(d, pattern)))]


def compare(name, parent, child, unit):
    spread = max(parent) - min(parent)
    ok = med(child) <= med(parent) + spread
    lines = ["## %s\n" % name,
             "| | runs (%s) | median |" % unit, "|---|---|---|",
             "| parent | %s | %.4g |" % (", ".join("%.4g" % x for x in parent), med(parent)),
             "| branch | %s | %.4g |" % (", ".join("%.4g" % x for x in child), med(child)),
             "", "Parent's spread (max - min): %.4g %s.  Condition `median(branch) <= median(parent) + spread`: **%s**.\n"
             % (spread, unit, "holds" if ok else "FAILS")]
    return "\n".join(lines), spread / med(parent), ok


def kernel_means(d):
    out = {}
    for p in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(p)):
            name = re.sub(r"\(.*$", "", row["Name"]).replace("void ", "").replace("pcseg::", "")
            out[name] = (int(row["Calls"]), float(row["AverageNs"]) / 1e3)
    return out


def main(d):
    head, rel, ok1 = compare("Headline: `bench.py --gpus 1 --steps 20 --warmup 4 --no-cpu-baseline`, order c p p c c p p c",
                             runs(d, "bench_parent_*.json", "ms_per_step"), runs(d, "bench_child_*.json", "ms_per_step"), "ms/step")
    path, _, ok2 = compare("The changed path: plane-free `ops.region_reduce` on 16 frames of 1022 x 1022, alternating fresh processes",
                           runs(d, "unaligned_parent_*.json", "median_ms"), runs(d, "unaligned_child_*.json", "median_ms"), "ms")
    sums = set(runs(d, "unaligned_*.json", "checksum"))
    with open(os.path.join(d, "speed.md"), "w") as f:
        f.write("# Speed against the parent commit 83c9388 (one machine, one session)\n\n%s\n%s\nChecksum of the area column, every run: %s.\n"
                % (head, path, sorted(sums)))
    a, b = kernel_means(os.path.join(d, "trace_parent")), kernel_means(os.path.join(d, "trace_branch"))
    with open(os.path.join(d, "kernels.md"), "w") as f:
        f.write("# Mean kernel times, parent beside branch (`rocprofv3 --kernel-trace --stats`, trace_driver.py)\n\n")
        f.write("The headline's relative spread is %.2f %%; kernels that rose by more are marked.\n\n" % (100 * rel))
        f.write("| kernel | calls | parent (us) | branch (us) | change |\n|---|---|---|---|---|\n")
        for k in sorted(set(a) | set(b)):
            if not k.startswith(KERNELS):
                continue
            x, y = a.get(k), b.get(k)
            if x and y:
                ch = y[1] / x[1] - 1
                f.write("| `%s` | %d | %.1f | %.1f | %+.1f %%%s |\n" % (k, y[0], x[1], y[1], 100 * ch, " **above the spread**" if ch > rel else ""))
            else:
                f.write("| `%s` | %s | %s | %s | one side only |\n" % (k, (x or y)[0], "%.1f" % x[1] if x else "-", "%.1f" % y[1] if y else "-"))
    print(open(os.path.join(d, "speed.md")).read())
    print(open(os.path.join(d, "kernels.md")).read())
    return 0 if ok1 and ok2 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
