"""Workload of the per-kernel trace: FramePipeline on the benchmark batch with the refined, shape and convexity tables on,
so that lp_count_kernel, shape_moments_kernel and shape_perimeter_kernel sit in the trace next to region_stats_col_kernel,
region_reduce_col_kernel and region_sums2_col_kernel.  Run it under `rocprofv3 --kernel-trace --stats` (no counters, no
other tracing), once per library (PCSEG_LIB selects the parent's)."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from particle_col_image_segmentation_amd import synth  # noqa: E402
from particle_col_image_segmentation_amd.pipeline import FramePipeline  # noqa: E402

dev = torch.device("cuda:0")
stack = synth.gen_batch_torch(10000, 64, 1024, 1024, dev)
pipe = FramePipeline(dict(synth.CELL_TYPES_5))
for _ in range(6):
    res = pipe.run(stack)
    res.synchronize()
    tabs = pipe.tables_device(res, refined=True, shape=True, convex=True)
    torch.cuda.synchronize()
pipe.synchronize()
print("rows:", {k: tuple(v.shape) for k, v in tabs.items() if hasattr(v, "shape")})
