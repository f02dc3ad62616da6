"""Turn the files of measure.sh into speed.md.  Usage: summarise.py OUT_DIR PARENT_REV > speed.md
The claim is "no slower": the branch's median may exceed the parent's median by at most the parent's own range (max - min of
its runs) -- a difference smaller than the scatter of what it is compared with cannot be told."""
import glob
import json
import os
import sys


def med(v):
    v = sorted(v)
    return (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2


def verdict(parent, child):
    return med(child) - med(parent) <= max(parent) - min(parent)


def main(d, rev):
    ok = True
    runs = lambda pat, key: [key(json.load(open(p))) for p in sorted(glob.glob(os.path.join(d, pat)))]
    parent, child = runs("bench_parent_*.json", lambda j: j["ms_per_step"]), runs("bench_child_*.json", lambda j: j["ms_per_step"])
    print("# Speed against the parent commit %s (one machine, one session per table)\n" % rev)
    print("Rule for every row: median(branch) - median(parent) <= max(parent) - min(parent).\n")
    print("## Headline: `bench.py --gpus 1 --steps 20 --warmup 4 --no-cpu-baseline`, order c p p c c p p c\n")
    print("| | runs (ms/step) | median | range |\n|---|---|---|---|")
    print("| parent | %s | %.4f | %.4f |" % (", ".join("%.4f" % x for x in parent), med(parent), max(parent) - min(parent)))
    print("| branch | %s | %.4f | %.4f |" % (", ".join("%.4f" % x for x in child), med(child), max(child) - min(child)))
    good = verdict(parent, child)
    ok = ok and good
    print("\nbranch - parent = %+.4f ms/step, allowed %.4f: **%s**.\n" % (med(child) - med(parent), max(parent) - min(parent),
                                                                       "holds" if good else "FAILS"))
    print("## The two transforms on the benchmark batch (`time_transforms.py`: 64 x 1024 x 1024, the `cells` sites, device events,")
    print("median of 20 after 2 warm-ups; each library twice, order c p p c)\n")
    print("| call | parent medians (ms) | branch medians (ms) | branch - parent | allowed | |\n|---|---|---|---|---|---|")
    for call in ("nearest_label", "edt_sq"):
        p, c = (runs("kernels_%s_*.json" % k, lambda j: j[call]["median_ms"]) for k in ("parent", "child"))
        good = verdict(p, c)
        ok = ok and good
        print("| `%s` | %s | %s | %+.4f | %.4f | %s |" % (call, ", ".join("%.4f" % x for x in p), ", ".join("%.4f" % x for x in c),
                                                         med(c) - med(p), max(p) - min(p), "holds" if good else "**FAILS**"))
    sums = {tuple(s) for s in runs("kernels_*.json", lambda j: j["checksum"])}
    print("\nSums of `d2` and `near` over the batch, all four runs: %s.\n" % ("equal" if len(sums) == 1 else "**DIFFERENT** %s" % sorted(sums)))
    return 0 if ok and len(sums) == 1 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
