"""Figures of the border stage on the benchmark batch (64 x 1024 x 1024, seed 10 000): the borders of the refined ROIs
(``ws_labels``) weighed by the boundary plane -- pairs per frame, table fill at the default ``pair_cap``, the library's
per-launch times of the fill, the merge and the relabelling, the whole ``merge_by_border`` call -- beside ``ag_count_kernel``
on two label images of the same size in the same session (the same bytes and the same kind of walk).  Per-launch times are the
mean over 5 calls after 2 warm-ups (pcseg_timing_enable).  Frame 0 is checked against torch on the way.
``PYTHONPATH=. python profiles/borders/measure_borders.py OUT.json`` from the repository root."""
import json
import sys
import time

import torch

from particle_col_image_segmentation_amd import ops, synth
from particle_col_image_segmentation_amd.pipeline import FramePipeline

sys.path.insert(0, __file__.rsplit("/", 2)[0] + "/agreement")
from measure_agreement import kernel_times  # noqa: E402

BELOW = 0.3


def wall_ms(fn, n=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3 / n, 4)


def main(path):
    dev = torch.device("cuda")
    B, H, W = 64, 1024, 1024
    pipe = FramePipeline(dict(synth.CELL_TYPES_5))
    stack = synth.gen_batch_torch(10_000, B, H, W, dev)
    res = pipe.run(stack)
    res.synchronize()
    L, V, counts = res["ws_labels"], stack[:, pipe.boundary_plane], res["n_markers"]
    cap = int(counts.max().item())
    out = {"batch": [B, H, W], "cap": cap, "below": BELOW}
    for conn in (8, 4):
        bd = ops.label_borders(L, V, conn=conn, cap=cap)
        assert bd["n_overflow"] == 0 and not bd["overflow"].any()
        per_frame = torch.bincount(bd["frame"], minlength=B)
        out["conn%d" % conn] = {
            "pair_cap": bd["pair_cap"],
            "pairs_per_frame": {"min": int(per_frame.min()), "median": float(per_frame.float().median()), "max": int(per_frame.max())},
            "fill_max": round(int(per_frame.max()) / bd["pair_cap"], 4),
            "links_per_pair_median": float(bd["links"].float().median())}
        if conn == 4:  # frame 0's right and down links against torch
            l0, v0 = L[0].to(torch.int64), V[0]
            keys, vals = [], []
            for p, q, vp, vq in ((l0[:, :-1], l0[:, 1:], v0[:, :-1], v0[:, 1:]), (l0[:-1], l0[1:], v0[:-1], v0[1:])):
                on = (p >= 1) & (q >= 1) & (p != q)
                keys.append((torch.minimum(p, q)[on] << 32) | torch.maximum(p, q)[on])
                vals.append(torch.round(torch.maximum(vp, vq)[on].to(torch.float64) * 4294967296.0).to(torch.int64))
            uniq, inv = torch.unique(torch.cat(keys), return_inverse=True)
            total = torch.zeros_like(uniq).index_add_(0, inv, torch.cat(vals))
            sel = bd["frame"] == 0
            assert torch.equal((bd["a"][sel] << 32) | bd["b"][sel], uniq) and torch.equal(bd["sum"][sel], total)
        kt = kernel_times(lambda: ops.label_borders(L, V, conn=conn, cap=cap))
        out["conn%d" % conn]["kernels"] = {k: v for k, v in kt.items() if "border_" in k or "pair_" in k}
    cap_t = int(res["counts"].max().item())
    kt = kernel_times(lambda: ops._contingency_rows(res["labels"], L, cap_t, cap, None))
    out["contingency_kernels"] = {k: v for k, v in kt.items() if "ag_count" in k}
    for by in ("mean", "saddle"):
        call = lambda: ops.merge_by_border(L, V, BELOW, by=by, counts=counts, cap=cap)
        merged, n_merged, _, flags = call()
        assert not flags.any()
        kt = kernel_times(call)
        out["merge_by_" + by] = {"kernels": {k: v for k, v in kt.items() if "border_" in k or "relabel_" in k or "pair_" in k},
                                 "call_wall_ms": wall_ms(call),
                                 "rois_before_median": float(counts.float().median()), "rois_after_median": float(n_merged.float().median())}
    # the pipeline's own cap (parents in the workspace, a table of 4 x that cap)
    pcap = res["stats"].shape[1]
    call = lambda: ops.merge_by_border(L, V, BELOW, counts=counts, cap=pcap)
    kt = kernel_times(call)
    out["merge_at_pipeline_cap"] = {"cap": pcap, "kernels": {k: v for k, v in kt.items() if "border_" in k or "relabel_" in k},
                                    "call_wall_ms": wall_ms(call)}
    print(json.dumps(out, indent=1), flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
