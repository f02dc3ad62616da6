"""The routes of the plane sums that bench.py does not time, for whatever library PCSEG_LIB names; one JSON line.
  --route ragged   FramePipeline.run on 16 frames of 1022 x 1022 (W % 4 == 2: _sums_stage takes ops.region_reduce with planes
                   per label image -- the plane-free pass and the row sums kernel); three windows of 10 steps, ms per step
  --route one      ops.region_reduce(labels, planes=planes) on one 1024 x 1024 frame with 7 planes, and on 16 frames with 5
                   planes, class map and counts (the plane-free pass and the one-image column sums kernel); HIP events, the
                   median of 50 calls after 5 warm-ups, ms per call
Run in alternating fresh processes."""
import argparse
import json
import os
import time

import numpy as np
import torch

from particle_col_image_segmentation_amd import ops, synth
from particle_col_image_segmentation_amd.pipeline import FramePipeline

ap = argparse.ArgumentParser()
ap.add_argument("--route", choices=("ragged", "one"), required=True)
a = ap.parse_args()
dev = torch.device("cuda")
out = {"lib": os.environ.get("PCSEG_LIB", "branch"), "route": a.route}


def blobs(B, H, W, n):
    """labels 0 .. n - 1 in blobs of 13 x 13, the label image of profiles/label_reduce/time_unaligned.py"""
    rng = np.random.default_rng(H + W)
    cell = rng.integers(0, n, (B, (H + 12) // 13, (W + 12) // 13))
    return torch.from_numpy(np.repeat(np.repeat(cell, 13, 1), 13, 2)[:, :H, :W].astype(np.int32)).to(dev)


def median_ms(call, reps=50, warm=5):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        call()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return float(np.median(ms)), min(ms), max(ms)


if a.route == "ragged":
    stack = synth.gen_batch_torch(10_000, 16, 1022, 1022, dev)
    pipe = FramePipeline(dict(synth.CELL_TYPES_5))
    for _ in range(4):
        r = pipe.run(stack)
    pipe.synchronize()
    windows = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(10):
            r = pipe.run(stack)
        pipe.synchronize()
        windows.append(1e3 * (time.perf_counter() - t0) / 10)

    def total(table, counts):  # (rows at and beyond a frame's count are not initialised)
        live = torch.arange(table.shape[1], device=dev)[None, :] < counts[:, None]
        return table[live].sum().item()

    out.update(ms_per_step_windows=windows, ms=float(np.median(windows)), n_markers=int(r["n_markers"].sum().item()),
               area=int(total(r["ws_stats"][:, :, 0], r["n_markers"])), ws_sum=float(total(r["ws_sums"], r["n_markers"])),
               cc_sum=float(total(r["cc_sums"], r["counts"])))
else:
    g = torch.Generator(device=dev).manual_seed(7)
    lab1, planes1 = blobs(1, 1024, 1024, 4000), torch.rand((1, 7, 1024, 1024), device=dev, generator=g) * 100
    lab16, planes16 = blobs(16, 1024, 1024, 4000), torch.rand((16, 5, 1024, 1024), device=dev, generator=g) * 100
    cls16 = torch.randint(0, 6, (16, 1024, 1024), device=dev, generator=g, dtype=torch.uint8)
    counts = torch.full((16,), 4000, dtype=torch.int32, device=dev)
    res = {}

    def one():
        res["one"] = ops.region_reduce(lab1, planes=planes1, cap=4000)

    def batch():
        res["batch"] = ops.region_reduce(lab16, counts, cls16, planes16, cap=4000)

    out["one_frame_7_planes_ms"], out["one_min"], out["one_max"] = median_ms(one)
    out["batch16_5_planes_cls_ms"], out["batch_min"], out["batch_max"] = median_ms(batch)
    out.update(area=int(res["batch"][0][:, :, 0].sum().item()), sum1=float(res["one"][2].sum().item()),
               sum16=float(res["batch"][2].sum().item()))
print(json.dumps(out))
