"""Parent against branch: the host cost of a call and the benchmark, fresh child processes in turn, parent first.
``python profiles/ops_call/ab_ops_call.py PARENT_ROOT OUT_PREFIX [ROUNDS]`` from the repository root: PARENT_ROOT holds the
parent commit's tree (``git archive PARENT | tar -x -C PARENT_ROOT``); both sides load this tree's libpcseg.so (the change
touches no C source).  Per round and side one ``time_calls.py`` child and one default ``bench.py --gpus 1`` run of that tree,
from which ``ms_per_step`` and ``config.launch_probe_ms_per_step.eager_8_host_threads`` are taken.  Writes
``OUT_PREFIX_calls.json`` and ``OUT_PREFIX_bench.json``: the runs, and per figure the two means, the parent's spread (largest
minus smallest of its rounds) and whether the branch's mean lies within that of the parent's mean or is faster.  Stops at
the first child that fails."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
LIB = os.path.join(ROOT, "particle_col_image_segmentation_amd", "libpcseg.so")
CHILD_LIMIT_S = 120


def child(side, k, argv):
    p = subprocess.run([sys.executable] + argv, env=dict(os.environ, PCSEG_LIB=LIB), stdout=subprocess.PIPE, timeout=CHILD_LIMIT_S,
                       text=True)
    if p.returncode != 0:
        raise SystemExit("%s child of round %d failed (exit code %r): nothing more is started" % (side, k, p.returncode))
    line = p.stdout.strip().splitlines()[-1]
    print(side, k, line[:300], flush=True)
    return json.loads(line)


def figures(runs):
    out = {}
    for name in runs["parent"][0]:
        v = {side: [r[name] for r in runs[side]] for side in runs}
        mean = {side: sum(x) / len(x) for side, x in v.items()}
        spread = max(v["parent"]) - min(v["parent"])
        out[name] = {"parent_mean": round(mean["parent"], 4), "branch_mean": round(mean["branch"], 4), "parent_spread": round(spread, 4),
                     "branch_within_parent_spread_or_faster": mean["branch"] <= mean["parent"] + spread}
        print(name, json.dumps(out[name]), flush=True)
    return out


def main(parent_root, prefix, rounds=5):
    sides = (("parent", os.path.abspath(parent_root)), ("branch", ROOT))
    calls = {"parent": [], "branch": []}
    bench = {"parent": [], "branch": []}
    for k in range(rounds):
        for side, root in sides:
            calls[side].append(child(side, k, [os.path.join(HERE, "time_calls.py"), root]))
            b = child(side, k, [os.path.join(root, "bench.py"), "--gpus", "1"])
            bench[side].append({"ms_per_step": b["ms_per_step"], "launch": b["config"]["launch"],
                                "eager_8_host_threads": b["config"]["launch_probe_ms_per_step"]["eager_8_host_threads"]})
    for path, runs, unit in ((prefix + "_calls.json", calls, "us per call"), (prefix + "_bench.json", bench, "ms per step")):
        numeric = {side: [{k: v for k, v in r.items() if not isinstance(v, str)} for r in runs[side]] for side in runs}
        with open(path, "w") as f:
            json.dump({"rounds": rounds, "unit": unit, "runs": runs, "figures": figures(numeric)}, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], *[int(v) for v in sys.argv[3:4]])
