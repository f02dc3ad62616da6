"""Parent against branch: ``tables_device`` on the benchmark's batch, fresh child processes (time_tables.py) in turn, parent
first.  ``python profiles/table_switches/ab_tables.py PARENT_ROOT OUT.json [ROUNDS]`` from the repository root: PARENT_ROOT
holds the parent commit's package (``git archive PARENT particle_col_image_segmentation_amd | tar -x -C PARENT_ROOT``); both
sides load this tree's libpcseg.so (PCSEG_LIB), which the change leaves as it is.  The spread of the parent's own figures
(max - min over its rounds) is the margin the branch's median is held against.  Stops at the first child that fails."""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
CHILD_LIMIT_S = 240


def main(parent_root, path, rounds=5):
    env = dict(os.environ, PCSEG_LIB=os.path.join(ROOT, "particle_col_image_segmentation_amd", "libpcseg.so"))
    runs = {"parent": [], "branch": []}
    for k in range(rounds):
        for side, root in (("parent", os.path.abspath(parent_root)), ("branch", ROOT)):
            p = subprocess.run([sys.executable, os.path.join(HERE, "time_tables.py"), root], env=env, stdout=subprocess.PIPE,
                               timeout=CHILD_LIMIT_S, text=True)
            if p.returncode != 0:
                raise SystemExit("%s child of round %d failed (exit code %r): nothing more is started" % (side, k, p.returncode))
            runs[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(side, k, p.stdout.strip().splitlines()[-1], flush=True)
    out = {"rounds": rounds, "runs": runs}
    for name in ("none", "every"):
        ms = {side: [r[name]["ms_per_call"] for r in runs[side]] for side in runs}
        spread = max(ms["parent"]) - min(ms["parent"])
        med = {side: statistics.median(v) for side, v in ms.items()}
        out[name] = {"parent_median_ms": med["parent"], "branch_median_ms": med["branch"], "parent_spread_ms": round(spread, 4),
                     "branch_within_parent_spread": abs(med["branch"] - med["parent"]) <= spread or med["branch"] <= med["parent"]}
        print(name, json.dumps(out[name]), flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], *[int(v) for v in sys.argv[3:4]])
