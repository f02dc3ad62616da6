"""Workload of the per-kernel trace: FramePipeline on the benchmark batch, six runs.  Run it under
`rocprofv3 --kernel-trace --stats` (no counters, no other tracing), once per library (PCSEG_LIB selects the parent's)."""
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
pipe.synchronize()
print("ws label sum:", int(res["ws_labels"].sum()))
