"""Parent against branch: the pair tables on the benchmark's batch, fresh child processes (time_pair_tables.py) in turn, parent
first.  ``python profiles/pair_tables/ab_pair_tables.py PARENT_ROOT PARENT_LIB OUT.json [ROUNDS]`` from the repository root:
PARENT_ROOT holds the parent commit's tree (``git archive PARENT | tar -x -C PARENT_ROOT``), PARENT_LIB its library
(``build.build(out_dir=...)`` run in that tree); the branch's children use this tree and its libpcseg.so.  The spread of the
parent's own figures (max - min over its rounds) is the margin the branch's median is held against.  Stops at the first child
that fails."""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
CHILD_LIMIT_S = 240


def main(parent_root, parent_lib, path, rounds=5):
    sides = (("parent", os.path.abspath(parent_root), os.path.abspath(parent_lib)),
             ("branch", ROOT, os.path.join(ROOT, "particle_col_image_segmentation_amd", "libpcseg.so")))
    runs = {"parent": [], "branch": []}
    for k in range(rounds):
        for side, root, lib in sides:
            p = subprocess.run([sys.executable, os.path.join(HERE, "time_pair_tables.py"), root], env=dict(os.environ, PCSEG_LIB=lib),
                               stdout=subprocess.PIPE, timeout=CHILD_LIMIT_S, text=True)
            if p.returncode != 0:
                raise SystemExit("%s child of round %d failed (exit code %r): nothing more is started" % (side, k, p.returncode))
            runs[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(side, k, p.stdout.strip().splitlines()[-1], flush=True)
    out = {"rounds": rounds, "runs": runs, "figures": {}}
    first = runs["parent"][0]
    figures = [("kernels_ms", t, s) for t in first["kernels_ms"] for s in ("fill", "count", "scan", "write")]
    figures += [("wall_ms", t, None) for t in first["wall_ms"]]
    for kind, table, stg in figures:
        get = lambda r: r[kind][table] if stg is None else r[kind][table][stg]
        ms = {side: [get(r) for r in runs[side]] for side in runs}
        spread = max(ms["parent"]) - min(ms["parent"])
        med = {side: statistics.median(v) for side, v in ms.items()}
        name = "%s %s" % (table, stg or "call wall")
        out["figures"][name] = {"parent_median_ms": med["parent"], "branch_median_ms": med["branch"], "parent_spread_ms": round(spread, 4),
                                "branch_within_parent_spread": abs(med["branch"] - med["parent"]) <= spread}
        print(name, json.dumps(out["figures"][name]), flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3], *[int(v) for v in sys.argv[4:5]])
