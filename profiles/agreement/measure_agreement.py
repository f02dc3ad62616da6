"""Figures of the agreement stage on the benchmark batch (64 x 1024 x 1024, seed 10 000): the contingency table of the
class-map components against the refined ROIs -- pairs per frame, table load factor, the library's per-launch times of the
count pass, the compaction and the match step -- beside the count pass of pcseg_label_parent on the same two images (the same
walk with a cheaper commit).  Per-launch times are the mean over 5 calls after 2 warm-ups (pcseg_timing_enable).  The table
of frame 0 is checked against torch.unique on the way.
``PYTHONPATH=. python profiles/agreement/measure_agreement.py OUT.json`` from the repository root."""
import ctypes
import json
import sys

import torch

from particle_col_image_segmentation_amd import _lib, ops, synth
from particle_col_image_segmentation_amd.pipeline import FramePipeline


def kernel_times(fn, n=5, warm=2):
    """{kernel: (launches per call, mean ms per call)} from the library's per-launch events"""
    lib = _lib.load()
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    lib.pcseg_timing_enable(1)
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    nbytes = lib.pcseg_timing_report(None, 0)
    buf = ctypes.create_string_buffer(nbytes + 16)
    lib.pcseg_timing_report(buf, nbytes + 16)
    lib.pcseg_timing_enable(0)
    out = {}
    for line in buf.value.decode().splitlines():
        name, calls, ms = line.split("\t")
        out[name.split("(")[0]] = (int(calls) / n, round(float(ms) / n, 4))
    return out


def main(path):
    dev = torch.device("cuda")
    B, H, W = 64, 1024, 1024
    pipe = FramePipeline(dict(synth.CELL_TYPES_5))
    res = pipe.run(synth.gen_batch_torch(10_000, B, H, W, dev))
    res.synchronize()
    T, S = res["labels"], res["ws_labels"]
    cap_t, cap_s = int(res["counts"].max().item()), int(res["n_markers"].max().item())
    ct = ops.label_contingency(T, S, cap_t=cap_t, cap_s=cap_s)
    assert ct["n_overflow"] == 0 and not ct["overflow"].any()
    per_frame = torch.bincount(ct["frame"], minlength=B)
    out = {"batch": [B, H, W], "cap_t": cap_t, "cap_s": cap_s, "pair_cap": ct["pair_cap"],
           "pairs_per_frame": {"min": int(per_frame.min()), "median": float(per_frame.float().median()), "max": int(per_frame.max())},
           "load_factor_max": round(int(per_frame.max()) / ct["pair_cap"], 4)}
    # frame 0 against torch.unique
    code, n = torch.unique(T[0].to(torch.int64) * (cap_s + 1) + S[0], return_counts=True)
    keep = code != 0
    sel = ct["frame"] == 0
    assert torch.equal(ct["t"][sel] * (cap_s + 1) + ct["s"][sel], code[keep]) and torch.equal(ct["n"][sel], n[keep])
    hot = ct["n"][sel].max().item()
    out["hot_pair_share_frame0"] = round(hot / (H * W), 4)
    rows = ops._contingency_rows(T, S, cap_t, cap_s, None)
    kt = kernel_times(lambda: ops._contingency_rows(T, S, cap_t, cap_s, None))
    out["contingency_kernels"] = {k: v for k, v in kt.items() if "ag_" in k or "pair_" in k}
    kt = kernel_times(lambda: ops._agreement_match(rows, (0.5, 0.75, 0.9)))
    out["match_kernels"] = {k: v for k, v in kt.items() if "ag_" in k}
    cap = res["stats"].shape[1]
    kt = kernel_times(lambda: ops.label_parent(T, S, res["n_markers"], cap=cap, stats_r=res["ws_stats"]))
    out["label_parent_kernels"] = {k: v for k, v in kt.items() if "lp_" in k}
    print(json.dumps(out, indent=1), flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
