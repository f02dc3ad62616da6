"""One-off timing of ops.pair_label_mixing against what a user could do before it: P + 1 calls of
ops.point_neighbours on labels shuffled by the same rule (made here in numpy, resident on the device before the clock
starts).  Device events, 2 warm-ups, mean of 10, the two routes alternating in one process; the baseline's histograms
must equal the new route's counts (checked during the first warm-up).

    python profiles/mixing/time_mixing.py [--only NAME] [--perms 199,999] [--out profiles/mixing/timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from particle_col_image_segmentation_amd import ops  # noqa: E402

SCALE = 512.0 / 19.0
SIDE = 2048.0
WORKLOADS = {"64x4000_k2": (64, 4000, 2), "64x4000_k3": (64, 4000, 3), "1x100000_k3": (1, 100000, 3)}


def labellings(slots, K, P, keys, seed):
    """include/pcseg.h's rule for B frames of n typed points each: slots (B, n) -> (P + 1, B, n) int8."""
    B, n = slots.shape
    u = np.uint64
    lab = np.empty((P + 1, B, n), np.int8)
    lab[0] = slots
    rem = np.stack([(slots == s).sum(axis=1) for s in range(K)], axis=1).astype(u)[:, None, :].repeat(P, axis=1)  # (B, P, K)
    head = (u(0xFFFFFF) & np.asarray(keys, u))[:, None] << u(40) ^ (np.arange(1, P + 1, dtype=u) << u(24))[None, :]
    bi, pi = np.meshgrid(np.arange(B), np.arange(P), indexing="ij")
    with np.errstate(over="ignore"):
        for i in range(n):
            tot = u(n - i)
            z = (head ^ u(i)) * u(0x9E3779B97F4A7C15) + u(seed)
            z ^= z >> u(30); z *= u(0xBF58476D1CE4E5B9)
            z ^= z >> u(27); z *= u(0x94D049BB133111EB)
            z ^= z >> u(31)
            r = ((z >> u(32)) * tot + (((z & u(0xFFFFFFFF)) * tot) >> u(32))) >> u(32)
            s = (r[:, :, None] >= np.cumsum(rem, axis=2)).sum(axis=2)
            lab[1:, :, i] = s.T
            rem[bi, pi, s] -= u(1)
    return lab


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(ms):
    ms = np.asarray(ms[2:])  # after 2 warm-ups
    return {"mean_ms": float(ms.mean()), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "std_ms": float(ms.std(ddof=1)),
            "n": int(ms.size)}


def kernel_times(fn, reps=5):
    """The library's own per-launch times (pcseg_timing_enable) of ``fn``: {kernel: ms per call of fn}."""
    import ctypes
    from particle_col_image_segmentation_amd import _lib
    lib = _lib.load()
    fn()
    torch.cuda.synchronize()
    lib.pcseg_timing_enable(1)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    n = lib.pcseg_timing_report(None, 0)
    buf = ctypes.create_string_buffer(n + 16)
    lib.pcseg_timing_report(buf, n + 16)
    lib.pcseg_timing_enable(0)
    out = {}
    for line in buf.value.decode().splitlines():
        name, calls, ms = line.split("\t")
        out[name.split("(")[0].split("::")[-1]] = out.get(name.split("(")[0].split("::")[-1], 0.0) + float(ms) / reps
    return out


def measure(name, P, seed=11, baseline=True):
    B, n, K = WORKLOADS[name]
    dev = torch.device("cuda")
    rng = np.random.default_rng(1234)
    xy = rng.uniform(0.0, SIDE, (B * n, 2))
    slots = rng.integers(0, K, (B, n))
    e = np.linspace(0.0, SIDE / 10.0 / SCALE, 65)
    m = 64
    t0 = time.time()
    lab = labellings(slots, K, P, np.arange(B), seed)
    print("  labels made on the host in %.1f s" % (time.time() - t0), flush=True)
    d_xy = torch.from_numpy(xy).to(dev)
    d_slot = torch.from_numpy(slots.reshape(-1).astype(np.int32)).to(dev)
    d_lab = torch.from_numpy(lab.reshape(P + 1, B * n)).to(dev).to(torch.int32)
    d_ids = torch.arange(B * n, dtype=torch.int32, device=dev)
    d_foff = torch.arange(B + 1, dtype=torch.int64, device=dev) * n

    new = lambda: ops.pair_label_mixing(d_xy, d_slot, d_foff, K, SCALE, e, P, seed=seed, counts=True)
    state = {"equal": None}

    def old(check=None):
        ok = torch.ones((), dtype=torch.bool, device=dev)
        for p in range(P + 1):
            h = ops.point_neighbours(d_xy, d_lab[p], d_ids, d_foff, K, SCALE, e)[2]
            if check is not None:
                ok &= (h[:, :, 1:m + 1] == check[:, p]).all()
        return ok

    if not baseline:
        return {"workload": name, "permutations": P, "new_ms": [timed(new)[0] for _ in range(5)], "kernels_ms": kernel_times(new)}
    t_new, t_old = [], []
    for rep in range(12):
        ms, out = timed(new)
        t_new.append(ms)
        if rep == 0:
            counts = out["counts"].clone()
            state["equal"] = bool(old(counts).item())
            print("  baseline histograms equal the new route's counts:", state["equal"], flush=True)
        ms, _ = timed(old)
        t_old.append(ms)
        print("  rep %2d: new %.3f ms, baseline %.1f ms" % (rep, t_new[-1], t_old[-1]), flush=True)
    in_range = int(counts[:, 0].sum().item())
    a, b = stats(t_new), stats(t_old)
    return {"workload": name, "frames": B, "points_per_frame": n, "strains": K, "bins": m, "permutations": P,
            "in_range_pairs": in_range, "pairs": B * n * (n - 1) // 2, "counts_equal_baseline": state["equal"],
            "new": a, "baseline": b, "kernels_ms": kernel_times(new), "ratio": b["mean_ms"] / a["mean_ms"],
            "increments_per_s": P * in_range / (a["mean_ms"] * 1e-3)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--perms", default="199,999")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", action="store_true", help="the new route and its per-kernel times only, no baseline")
    args = ap.parse_args()
    rows = []
    for name in WORKLOADS:
        if args.only and name != args.only:
            continue
        for P in (int(v) for v in args.perms.split(",")):
            print("%s, P = %d" % (name, P), flush=True)
            rows.append(measure(name, P, baseline=not args.kernels))
            print(json.dumps(rows[-1]), flush=True)
            if args.out:
                with open(args.out, "w") as f:
                    json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
