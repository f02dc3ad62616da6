"""One-off timing of spatial.window_pair_counts against what a user could do before it: the zero-padded
torch.fft.rfft2 autocorrelation of the mask in float64 on the same device, rounded to integers, and binned with torch (frames in
chunks, so that the padded spectra fit).  Device events, 2 warm-ups, mean of 10 with minimum .. maximum, the two routes
alternating in one process; the two histograms must be equal (checked during the first warm-up).
Workload: 64 frames of 1024 x 1024 particle masks (holes filled) of synth.py; reaches 32, 128 and 512 px.

    python profiles/window_pairs/time_window_pairs.py [--frames 64] [--size 1024] [--reaches 32,128,512] [--out profiles/window_pairs/timing.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from particle_col_image_segmentation_amd import ops, spatial, synth  # noqa: E402

SCALE = 9.95  # px per um


def fft_route(mask, thr, R, chunk=8):
    """[n_px, bins.., over] int64 (B, m + 2) from the float64 autocorrelation"""
    B, H, W = mask.shape
    dev = mask.device
    m = thr.shape[0] - 1
    Ry, Rx = min(R, H - 1), min(R, W - 1)
    dy = torch.arange(0, Ry + 1, device=dev)
    dx = torch.arange(-Rx, Rx + 1, device=dev)
    k = torch.bucketize(dy[:, None] ** 2 + dx[None, :] ** 2, thr, right=True) - 1
    weight = torch.where(dy[:, None] > 0, 2, 1)
    keep = (k < m).reshape(-1)
    idx = k.reshape(-1)[keep]
    out = torch.zeros((B, m + 2), dtype=torch.int64, device=dev)
    for lo in range(0, B, chunk):
        x = mask[lo:lo + chunk].to(torch.float64)
        f = torch.fft.rfft2(x, s=(2 * H, 2 * W))
        ac = torch.fft.irfft2(f * f.conj(), s=(2 * H, 2 * W))
        g = torch.round(ac[:, dy[:, None] % (2 * H), dx[None, :] % (2 * W)]).to(torch.int64) * weight
        out[lo:lo + chunk, 1:m + 1].index_add_(1, idx, g.reshape(g.shape[0], -1)[:, keep])
    A = mask.reshape(B, -1).to(torch.int64).sum(dim=1)
    out[:, 0] = A
    out[:, m + 1] = A * A - out[:, 1:m + 1].sum(dim=1)
    return out


def timed(fn, reps):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reaches", default="32,128,512")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: a time is a time on the device")
    dev = torch.device("cuda")
    stack = synth.gen_batch_torch(2200, a.frames, a.size, a.size, dev)
    mask = ops.fill_holes((ops.argmax_planes(stack) == 3).view(torch.uint8))
    del stack
    rows = []
    for R in (int(v) for v in a.reaches.split(",")):
        edges = np.linspace(0.0, (R + 0.5) / SCALE, 33)
        assert spatial.window_reach(edges, SCALE) == R
        thr = torch.from_numpy(ops.surface_thresholds(edges, SCALE)).to(dev)
        new = lambda: spatial.window_pair_counts(mask, edges, SCALE)
        old = lambda: fft_route(mask, thr, R)
        assert torch.equal(new(), old()), "the two routes differ at reach %d" % R
        t_new, t_old = [], []
        for rep in range(12):  # alternating; the first two rounds are warm-ups
            tn, to = timed(new, 1), timed(old, 1)
            if rep >= 2:
                t_new += tn
                t_old += to
        row = {"reach_px": R, "frames": a.frames, "size": a.size, "bins": 32, "window_px_mean": float(mask.sum().item()) / a.frames,
               "window_pair_counts_ms": {"mean": float(np.mean(t_new)), "min": min(t_new), "max": max(t_new)},
               "rfft2_float64_ms": {"mean": float(np.mean(t_old)), "min": min(t_old), "max": max(t_old)}, "equal": True}
        print(json.dumps(row))
        rows.append(row)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
