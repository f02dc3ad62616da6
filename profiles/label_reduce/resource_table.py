"""Kernel resource usage of reduce.hip, shape.hip and refined.hip, parent beside branch, as a markdown table.

Usage: resource_table.py PARENT_DIR BRANCH_DIR > resource_usage.md
Each directory holds reduce.txt, shape.txt, refined.txt: the stderr of
    hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -Rpass-analysis=kernel-resource-usage -c <file>.hip
(the flags of build.py plus the remark) on that tree.  Exit status 1 if a branch kernel breaks a condition: scratch where
the parent had none, a lower occupancy, other LDS bytes."""
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


def main(parent_dir, branch_dir):
    bad = []
    print("# Kernel resource usage, parent (83c9388) beside branch\n")
    print("gfx950, the flags of build.py plus `-Rpass-analysis=kernel-resource-usage`; every kernel of the three files.")
    print("Each cell: parent -> branch (one number where they agree).  Kernels that exist on one side only are listed with `-`.\n")
    for f in ("reduce", "shape", "refined"):
        a, b = parse("%s/%s.txt" % (parent_dir, f)), parse("%s/%s.txt" % (branch_dir, f))
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
    sys.exit(main(sys.argv[1], sys.argv[2]))
