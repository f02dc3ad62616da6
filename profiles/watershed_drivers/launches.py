"""The launch sequences of launch_driver.py under the parent's library and the branch's, side by side.
Usage: launches.py PARENT_TRACE_DIR BRANCH_TRACE_DIR > launches.md   (the directories rocprofv3 wrote, with *kernel_trace.csv)
Exit status 1 unless the ordered lists of (kernel name without <64>, grid, workgroup size, LDS bytes) of the ws_ kernels
are identical."""
import csv
import glob
import os
import re
import sys


def launches(d):
    rows = []
    for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(p)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = []
    for r in rows:
        name = re.sub(r"\(.*$", "", r["Kernel_Name"]).replace("void ", "").replace("pcseg::", "").replace("<64>", "")
        if not name.startswith("ws_"):
            continue
        lds = r.get("LDS_Block_Size", r.get("Group_Segment_Size", "?"))
        out.append((name, "x".join(r["Grid_Size_" + a] for a in "XYZ"), "x".join(r["Workgroup_Size_" + a] for a in "XYZ"), lds))
    return out


def main(parent_dir, branch_dir):
    a, b = launches(parent_dir), launches(branch_dir)
    same = a == b and len(a) > 0
    print("# Launch sequence of the watershed, parent 0c66b24 beside branch\n")
    print("`launch_driver.py` (4 frames of 256 x 256, modes 0, 2 and 6) under `rocprofv3 --kernel-trace --stats`, one run per")
    print("library.  Every `ws_` kernel in start order: name (the parent's `<64>` dropped), grid in work-items, workgroup, LDS bytes.\n")
    print("%d launches under the parent, %d under the branch: **%s**.\n" % (len(a), len(b), "identical" if same else "DIFFERENT"))
    print("| # | kernel | grid | workgroup | LDS | branch (where it differs) |\n|---|---|---|---|---|---|")
    for i in range(max(len(a), len(b))):
        x = a[i] if i < len(a) else ("-",) * 4
        y = b[i] if i < len(b) else ("-",) * 4
        print("| %d | `%s` | %s | %s | %s | %s |" % (i, x[0], x[1], x[2], x[3], "" if x == y else "`%s` %s %s %s" % y))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
