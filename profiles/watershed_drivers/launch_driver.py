"""Workload of the launch comparison: ops.watershed once each in modes 0, 2 and 6 on four frames of 256 x 256 -- two of plain
noise, two quantised as in tests/test_gpu_watershed_fences.py (_frames, ties=True), so that both levels and the exact pass
run.  Run it under `rocprofv3 --kernel-trace --stats` (no counters, no other tracing), once per library (PCSEG_LIB selects
the parent's); launches.py compares the two traces."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from particle_col_image_segmentation_amd import ops  # noqa: E402

B, H, W = 4, 256, 256
rng = np.random.default_rng(3)
img = rng.random((B, H, W))
q = np.floor(img[2:] * 200) / 200
img[2:] = (q + np.roll(q, 1, 1) + np.roll(q, 1, 2)) / 3
mask = np.ones((B, H, W), np.uint8)
mask[:2] = rng.random((2, H, W)) < 0.97
mk = np.zeros((B, H, W), np.int32)
for b in range(B):
    sel = rng.random((H, W)) < 0.002
    sel[H // 2, W // 2] = True
    mk[b][sel] = rng.permutation(int(sel.sum())).astype(np.int32) + 1
dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (img.astype(np.float32), mk, mask)]
for mode in (0, 2, 6):
    out, flags = ops.watershed(*dev, mode=mode)
    torch.cuda.synchronize()
    print("mode", mode, "tie_flags", flags.cpu().tolist(), "label sum", int(out.sum()))
