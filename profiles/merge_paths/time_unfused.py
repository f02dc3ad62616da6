"""Times the calls test_merge_groups makes to the grouping entry points that are off the benchmark path (2 frames of
160 x 160, the test's inputs): median of 50 launches each, in microseconds, as one JSON line.  PCSEG_LIB selects the library."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from particle_col_image_segmentation_amd import ops, synth  # noqa: E402

st = torch.from_numpy(synth.gen_batch(90, 2, 160, 160)).cuda()
cm, labels, counts = ops.classmap_label(st)
stats, cls_out, _, _ = ops.region_reduce(labels, counts, cls=cm)
cap = stats.shape[1]
ch, ah, n = cls_out.cpu().numpy(), stats[:, :, 0].cpu().numpy(), counts.cpu().numpy()
rl = np.full((2, cap), -1, np.int32)
nl = np.zeros(2, np.int32)
for b in range(2):
    sel = [r for r in range(n[b]) if ch[b, r] in (1, 2) and ah[b, r] >= 20]
    rl[b, :len(sel)] = sel
    nl[b] = len(sel)
rl, nl = torch.from_numpy(rl).cuda(), torch.from_numpy(nl).cuda()
bits = (1 << 1) | (1 << 2)
dl, _ = ops.label_bool8(ops.dilate_disk(cm, bits, 2))
roots = ops.dilated_roots(cm, bits, 2)
dbits, run_par = ops.dilated_runs(cm, bits, 2)
g, ng = ops.merge_groups_runs(dbits, run_par, stats, rl, nl)
calls = {
    "merge_groups(labels)": lambda: ops.merge_groups(dl, stats, rl, nl),
    "merge_groups(roots)": lambda: ops.merge_groups(roots, stats, rl, nl, roots=True),
    "merge_groups_runs": lambda: ops.merge_groups_runs(dbits, run_par, stats, rl, nl),
    "group_reduce": lambda: ops.group_reduce(stats, rl, nl, g, ng, 160, 160),
    "merge_groups_fused": lambda: ops.merge_groups_fused(dbits, run_par, stats, rl[:, None, :].contiguous(), nl[:, None].contiguous(), 0),
    "dilated_runs": lambda: ops.dilated_runs(cm, bits, 2),
    "dilated_roots": lambda: ops.dilated_roots(cm, bits, 2),
}
out = {"list": nl.tolist(), "groups": ng.tolist()}
for name, fn in calls.items():
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(50):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b) * 1e3)
    out[name + "_us"] = round(float(np.median(t)), 1)
print(json.dumps(out))
