"""Timings of the territory stage on the benchmark batch (64 x 1024 x 1024, seed 10 000): device events, median of 20 after 2
warm-ups, with min and max.  ``python profiles/territory/measure_territory.py OUT.json`` from the repository root."""
import json
import statistics
import sys
import time

import torch

from particle_col_image_segmentation_amd import ops, synth
from particle_col_image_segmentation_amd.pipeline import RATIOS_5, FramePipeline, TableSwitches


def timed(fn, wall=False, n=20, warm=2):
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


def main(path):
    dev = torch.device("cuda")
    B, H, W = 64, 1024, 1024
    pipe = FramePipeline(dict(synth.CELL_TYPES_5))
    res = pipe.run(synth.gen_batch_torch(10_000, B, H, W, dev))
    res.synchronize()
    cap = res["stats"].shape[1]
    fid = torch.arange(B, dtype=torch.int64, device=dev)
    raw = ops.build_tables(res, res.get("groups") or {}, fid, 5, RATIOS_5, tables=pipe.tables_, switches=TableSwitches(refined=True))
    out = {"batch": [B, H, W], "cap": cap}
    for name, rows in (("cells", ops.class_rows(res)), ("refined", ops.refined_rows(res, raw["kind_r"], raw["slot_r"]))):
        labels, live, slot_of = rows.labels, rows.live, rows.slot_of
        sel = live.view(torch.uint8)
        # the same sites as a mask for the distance transform: 0 on a site, 1 elsewhere
        lut = torch.cat([torch.ones((B, 1), dtype=torch.uint8, device=dev), 1 - sel], dim=1)
        idx = labels.clamp(0, cap).to(torch.int64).reshape(B, -1)
        not_site = torch.gather(lut, 1, idx).reshape(B, H, W).contiguous()
        d2, near, _ = ops.nearest_label(labels, sel, cap)
        assert torch.equal(d2, ops.edt_sq(not_site))
        r = {"sites_rows": int(live.sum().item()), "site_px": int((not_site == 0).sum().item())}
        r["nearest_label"] = timed(lambda: ops.nearest_label(labels, sel, cap))
        r["edt_sq_same_mask"] = timed(lambda: ops.edt_sq(not_site))
        r["ratio"] = round(r["nearest_label"]["median_ms"] / r["edt_sq_same_mask"]["median_ms"], 3)
        r["territory_reduce"] = timed(lambda: ops.territory_reduce(near, d2, None, -1, cap))
        r["territory_pairs"] = timed(lambda: ops.territory_pairs(near, d2, -1, 8 * cap, slot_of=slot_of, n_types=2), wall=True)
        r["pairs"] = int(ops.territory_pairs(near, d2, -1, 8 * cap)["a"].shape[0])
        out[name] = r
        print(name, json.dumps(r), flush=True)
    for terr in (False, True):
        out["tables_device_territory_%s" % terr] = timed(
            lambda: pipe.tables_device(res, refined=True, neighbours=True, territory=terr, check=False), wall=True)
        print(terr, json.dumps(out["tables_device_territory_%s" % terr]), flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
