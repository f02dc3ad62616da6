"""The one changed path: ops.region_reduce(labels, counts) on a plane-free batch of 16 frames of 1022 x 1022 (W % 4 == 2:
the parent walks rows, the branch takes the guarded column walk).  HIP events, 3 warm-ups, 15 repetitions; prints one JSON
line.  Run in alternating fresh processes, PCSEG_LIB selecting the parent's library."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from particle_col_image_segmentation_amd import ops  # noqa: E402

B, H, W = 16, 1022, 1022
rng = np.random.default_rng(1022)
cell = rng.integers(0, 4000, (B, (H + 12) // 13, (W + 12) // 13))  # blobs of 13 x 13, label 0 included
labs = torch.from_numpy(np.repeat(np.repeat(cell, 13, 1), 13, 2)[:, :H, :W].astype(np.int32)).cuda()
counts = torch.full((B,), 4000, dtype=torch.int32, device="cuda")
for _ in range(3):
    stats = ops.region_reduce(labels=labs, counts=counts, cap=4000)[0]
torch.cuda.synchronize()
ms = []
for _ in range(15):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    stats = ops.region_reduce(labels=labs, counts=counts, cap=4000)[0]
    b.record()
    b.synchronize()
    ms.append(a.elapsed_time(b))
print(json.dumps({"lib": os.environ.get("PCSEG_LIB", "branch"), "shape": [B, H, W], "median_ms": float(np.median(ms)),
                  "min_ms": min(ms), "max_ms": max(ms), "checksum": int(stats[:, :, 0].sum().item())}))
