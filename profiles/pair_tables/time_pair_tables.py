"""One child of ab_pair_tables.py: the three pair tables on the benchmark's batch (64 x 1024 x 1024, seed 10 000).
``python time_pair_tables.py PACKAGE_ROOT`` (PCSEG_LIB: the library) prints one JSON line: per table the library's per-launch
times (ms per call, mean of 5 calls after 2 warm-ups: ``kernel_times`` of profiles/agreement/measure_agreement.py) of its fill
kernel, ``pair_count``, ``pair_scan`` and its row writer -- whatever the tree calls it --, and the wall time of the calls
``territory_pairs`` (``slot_of`` given, ``pair_cap = 8 cap``), ``_contingency_rows``, ``label_borders`` (conn 8) and
``merge_by_border`` (mean), each followed by a synchronise (mean of 10 calls after 2 warm-ups)."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "agreement"))
sys.path.insert(0, sys.argv[1])

import torch  # noqa: E402

from particle_col_image_segmentation_amd import ops, synth  # noqa: E402
from particle_col_image_segmentation_amd.pipeline import FramePipeline  # noqa: E402
from measure_agreement import kernel_times  # noqa: E402


def stage(name):
    return "write" if "write" in name else "count" if "pair_count" in name else "scan" if "pair_scan" in name else "fill"


def wall_ms(fn, n=10, warm=2):
    for _ in range(warm):
        fn()
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
        torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3 / n, 4)


def main():
    dev = torch.device("cuda")
    pipe = FramePipeline(dict(synth.CELL_TYPES_5))
    stack = synth.gen_batch_torch(10_000, 64, 1024, 1024, dev)
    res = pipe.run(stack)
    res.synchronize()
    T, S, V, counts = res["labels"], res["ws_labels"], stack[:, pipe.boundary_plane], res["n_markers"]
    cap, cap_t, cap_s = res["stats"].shape[1], int(res["counts"].max().item()), int(counts.max().item())
    rows = ops.class_rows(res)
    d2, near, _ = ops.nearest_label(rows.labels, rows.live.view(torch.uint8), cap)
    calls = {"territory_pairs": lambda: ops.territory_pairs(near, d2, -1, 8 * cap, slot_of=rows.slot_of, n_types=2),
             "contingency_rows": lambda: ops._contingency_rows(T, S, cap_t, cap_s, None),
             "label_borders": lambda: ops.label_borders(S, V, conn=8, cap=cap_s),
             "merge_by_border": lambda: ops.merge_by_border(S, V, 0.3, by="mean", counts=counts, cap=cap_s)}
    out = {"kernels_ms": {}, "wall_ms": {}, "names": {}}
    for name in ("territory_pairs", "contingency_rows", "label_borders"):
        kt = {k: v for k, v in kernel_times(calls[name]).items() if "pair" in k or "ag_" in k or "border_" in k}
        assert sorted(stage(k) for k in kt) == ["count", "fill", "scan", "write"], sorted(kt)
        out["kernels_ms"][name] = {stage(k): v[1] for k, v in kt.items()}
        out["names"][name] = {stage(k): k for k in kt}
    for name, fn in calls.items():
        out["wall_ms"][name] = wall_ms(fn)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
