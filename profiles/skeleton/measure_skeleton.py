"""Figures of the skeleton stage on the benchmark batch (64 x 1024 x 1024, seed 10 000): full iterations, launches, the share
of tiles on each launch's list, and the times of thin_labels, region_skeleton and the table stage with and without the
``skeleton`` switch (beside ``convex``).  Device events around the call (thin_labels waits for the device between launches:
the events span those waits too), median of 7 after 2 warm-ups, with min and max; the table stage by the wall clock around
a synchronised call.  ``PYTHONPATH=. python profiles/skeleton/measure_skeleton.py OUT.json`` from the repository root."""
import ctypes
import json
import statistics
import sys
import time

import torch

from particle_col_image_segmentation_amd import _lib, ops, synth
from particle_col_image_segmentation_amd.pipeline import FramePipeline


def timed(fn, wall=False, n=7, warm=2):
    out = []
    for k in range(warm + n):
        torch.cuda.synchronize()
        if wall:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
        else:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
        if k >= warm:
            out.append(ms)
    return {"median_ms": round(statistics.median(out), 4), "min_ms": round(min(out), 4), "max_ms": round(max(out), 4)}


def kernel_times(fn):
    """{kernel: (launches, total ms)} of one call, from the library's per-launch events"""
    lib = _lib.load()
    lib.pcseg_timing_enable(1)
    fn()
    torch.cuda.synchronize()
    nbytes = lib.pcseg_timing_report(None, 0)
    buf = ctypes.create_string_buffer(nbytes + 16)
    lib.pcseg_timing_report(buf, nbytes + 16)
    lib.pcseg_timing_enable(0)
    out = {}
    for line in buf.value.decode().splitlines():
        name, calls, ms = line.split("\t")
        out[name] = (int(calls), round(float(ms), 4))
    return out


def active_share(labels, peel):
    """the share of tiles on the list of every launch, from the peel image: the first launch lists the tiles with a pixel, a
    later one the tiles that deleted a pixel in the launch before it, and their 8 neighbours"""
    (tw, th), k = ops.THIN_TILE, ops.THIN_HALO
    B, H, W = labels.shape
    ty, tx = (H + th - 1) // th, (W + tw - 1) // tw
    pad = lambda m: torch.nn.functional.pad(m, (0, tx * tw - W, 0, ty * th - H))
    tiles = lambda m: pad(m).reshape(B, ty, th, tx, tw).any(dim=4).any(dim=2)
    gone = peel.view(torch.int16).to(torch.int32) & 0xFFFF  # (torch converts no uint16: its bit pattern)
    gone = torch.where(gone == ops.PEEL_SKELETON, torch.zeros_like(gone), gone)
    share = [float(tiles(labels > 0).float().mean().item())]
    for j in range(1, (int(gone.max().item()) + k - 1) // k + 1):
        hit = tiles((gone > k * (j - 1)) & (gone <= k * j)).float()[:, None]
        near = torch.nn.functional.max_pool2d(hit, 3, stride=1, padding=1)
        share.append(float(near.mean().item()))
    return [round(s, 4) for s in share]


def main(path):
    dev = torch.device("cuda")
    B, H, W = 64, 1024, 1024
    pipe = FramePipeline(dict(synth.CELL_TYPES_5))
    res = pipe.run(synth.gen_batch_torch(10_000, B, H, W, dev))
    res.synchronize()
    cap = res["stats"].shape[1]
    out = {"batch": [B, H, W], "cap": cap, "tile": list(ops.THIN_TILE), "halo": ops.THIN_HALO}
    for name, key, cnt in (("cells", "labels", "counts"), ("refined", "ws_labels", "n_markers")):
        labels, counts = res[key], res[cnt]
        peel, iters = ops.thin_labels(labels)
        r = {"labels": int(counts.sum().item()), "foreground_share": round(float((labels > 0).float().mean().item()), 4),
             "full_iterations_max": int(iters.max().item()), "full_iterations_median": float(iters.float().median().item())}
        kt = kernel_times(lambda: ops.thin_labels(labels))
        r["kernels"] = {k.split("(")[0]: v for k, v in kt.items() if "thin_" in k}
        r["launches"] = max([v[0] for k, v in r["kernels"].items() if "thin_tile_kernel" in k] or [0])
        r["tiles_listed_share_per_launch"] = active_share(labels, peel)
        r["thin_labels"] = timed(lambda: ops.thin_labels(labels))
        r["region_skeleton"] = timed(lambda: ops.region_skeleton(labels, peel, counts, cap=cap))
        out[name] = r
        print(name, json.dumps(r), flush=True)
    for kw in ({}, {"skeleton": True}, {"convex": True}):
        tag = "tables_device_refined" + "".join("_" + k for k in kw)
        out[tag] = timed(lambda: pipe.tables_device(res, refined=True, check=False, **kw), wall=True)
        print(tag, json.dumps(out[tag]), flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
