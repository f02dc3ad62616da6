"""One child of ab_ops_call.py: what a call of a wrapper costs the host.
``python time_calls.py PACKAGE_ROOT`` (PCSEG_LIB: the library) prints one JSON line, us per call: the wall time of ``median5``,
``fill_holes``, ``edt_sq`` and ``region_shape`` on a 1 x 64 x 64 input -- N calls in a row with no synchronise between them (one
after the last, outside the clock: the kernels are a few us each and the queue never fills, so the clock sees the host side
of a call: checks, allocations, marshalling, the launches) -- and of ``label_contingency`` (a pair table: two calls, its
readback and its sorts between them) -- and of ``watershed`` and ``region_reduce`` (with a class map and planes), the two
wrappers with the most argument checks (profiles/ops_contract).  The best of five repeats of N = 2000 calls (200 for the
pair table)."""
import json
import sys
import time

sys.path.insert(0, sys.argv[1])

import torch  # noqa: E402

from particle_col_image_segmentation_amd import ops  # noqa: E402


def us_per_call(fn, n, repeats=5):
    for _ in range(max(n // 10, 10)):
        fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        dt = time.perf_counter() - t0
        torch.cuda.synchronize()
        best = dt if best is None else min(best, dt)
    return round(best * 1e6 / n, 3)


def main():
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(5)
    mask = (torch.rand((1, 64, 64), generator=g) < 0.6).to(torch.uint8).to(dev)
    labels, counts = ops.label_bool8(mask)
    cap = int(counts.max().item())
    other = torch.roll(labels, 3, dims=2).contiguous()
    img = torch.rand((1, 64, 64), generator=g).to(dev)
    planes = torch.rand((1, 5, 64, 64), generator=g).to(dev)
    markers = labels * (labels % 7 == 1)
    out = {"median5": us_per_call(lambda: ops.median5(mask), 2000),
           "fill_holes": us_per_call(lambda: ops.fill_holes(mask), 2000),
           "edt_sq": us_per_call(lambda: ops.edt_sq(mask), 2000),
           "region_shape": us_per_call(lambda: ops.region_shape(labels, counts, cap=cap), 2000),
           "label_contingency": us_per_call(lambda: ops.label_contingency(labels, other, cap_t=cap, cap_s=cap), 200),
           "watershed": us_per_call(lambda: ops.watershed(img, markers, mask, mode=2), 2000),
           "region_reduce": us_per_call(lambda: ops.region_reduce(labels, counts, mask, planes, cap=cap), 2000)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
