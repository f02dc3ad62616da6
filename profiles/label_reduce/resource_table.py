"""Kernel resource usage of some files of csrc/, parent beside branch, as a markdown table.

Usage: resource_table.py [--parent REV] [--renamed OLD=NEW ...] PARENT_DIR BRANCH_DIR [FILE ...] > resource_usage.md
Each directory holds FILE.txt for every FILE (default: reduce shape refined): the stderr of
    hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -Rpass-analysis=kernel-resource-usage -c <file>.hip
(the flags of build.py plus the remark) on that tree.  --renamed puts the parent's kernel OLD on the row of the branch's
kernel NEW (names as the table prints them).  Exit status 1 if a branch kernel breaks a condition: scratch where the
parent had none, a lower occupancy, other LDS bytes."""
import argparse
import re
import subprocess
import sys

FIELDS = (("VGPRs", "VGPRs"), ("TotalSGPRs", "SGPRs"), ("LDS Size [bytes/block]", "LDS"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occupancy"))


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    short = []
    for n in out[:len(names)]:
        n = n.replace("pcseg::", "").replace("void ", "")
        short.append(re.sub(r"\(.*$", "", n))  # the argument list away, template arguments stay
    return short


def parse(path):
    kernels, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([^:]+): (\S+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    names = list(kernels)
    return dict(zip(demangle(names), (kernels[n] for n in names)))


def main(parent_dir, branch_dir, files, parent_rev, renamed):
    bad = []
    print("# Kernel resource usage, parent (%s) beside branch\n" % parent_rev)
    print("gfx950, the flags of build.py plus `-Rpass-analysis=kernel-resource-usage`; every kernel of the files below.")
    print("Each cell: parent -> branch (one number where they agree).  Kernels that exist on one side only are listed with `-`.")
    for old, new in renamed.items():
        print("The parent's `%s` is listed as `%s`." % (old, new))
    print()
    for f in files:
        a, b = parse("%s/%s.txt" % (parent_dir, f)), parse("%s/%s.txt" % (branch_dir, f))
        a = {renamed.get(k, k): v for k, v in a.items()}
        print("## %s.hip\n" % f)
        print("| Kernel | " + " | ".join(h for _, h in FIELDS) + " |")
        print("| --- |" + " --- |" * len(FIELDS))
        for k in sorted(set(a) | set(b)):
            cells = []
            for key, head in FIELDS:
                x, y = a.get(k, {}).get(key, "-"), b.get(k, {}).get(key, "-")
                cells.append(x if x == y else "%s -> %s" % (x, y))
                if "-" in (x, y):
                    continue
                if (head == "scratch" and x == "0" and y != "0") or (head == "occupancy" and int(y) < int(x)) or (head == "LDS" and x != y):
                    bad.append((k, head, x, y))
            print("| `%s` | %s |" % (k, " | ".join(cells)))
        print()
    print("Conditions broken: %s" % (", ".join("%s %s %s -> %s" % t for t in bad) if bad else "none"))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="83c9388")
    ap.add_argument("--renamed", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("parent_dir")
    ap.add_argument("branch_dir")
    ap.add_argument("files", nargs="*", default=["reduce", "shape", "refined"])
    args = ap.parse_args()
    sys.exit(main(args.parent_dir, args.branch_dir, args.files, args.parent, dict(r.split("=", 1) for r in args.renamed)))
