"""Figures of the gap table on the benchmark batch (64 x 1024 x 1024, seed 10 000): ``gaps.label_gaps`` over the rows of
``cells`` (class-map components) and over the refined ROIs, for the batch's strains, beside the yardstick -- ``ops.nearest_label``
once per type slot on the same labels and selections, the existing code doing the nearest comparable work.  Call times are
device events around 5 calls after 2 warm-ups; the per-launch times are the library's own (pcseg_timing_enable), the mean over 5
calls after 2 warm-ups, and say where the time goes: column pass, row pass, reduce.  Frame 0 is checked on the way: the table's
symmetry and ``gap2 == 1`` against touching labels.
``PYTHONPATH=. python profiles/gaps/measure_gaps.py OUT.json`` from the repository root."""
import json
import sys

import torch

from particle_col_image_segmentation_amd import gaps, ops, synth
from particle_col_image_segmentation_amd.pipeline import FramePipeline

sys.path.insert(0, __file__.rsplit("/", 2)[0] + "/agreement")
from measure_agreement import kernel_times  # noqa: E402


def event_ms(fn, n=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return round(t0.elapsed_time(t1) / n, 4)


def touching(lab, live, slot_of, K):
    """(cap, K) bool of one frame: label l has a 4-neighbour pixel of another live label of slot t"""
    cap = live.shape[0]
    out = torch.zeros((cap, K), dtype=torch.bool, device=lab.device)
    l64 = lab.to(torch.int64)
    for p, q in ((l64[:, :-1], l64[:, 1:]), (l64[:-1], l64[1:])):
        on = (p >= 1) & (q >= 1) & (p <= cap) & (q <= cap) & (p != q)
        for a, b in ((p[on], q[on]), (q[on], p[on])):
            ok = live[a - 1] & live[b - 1] & (slot_of[b - 1] < K)
            out[a[ok] - 1, slot_of[b[ok] - 1].to(torch.int64)] = True
    return out


def main(path):
    dev = torch.device("cuda")
    B, H, W = 64, 1024, 1024
    pipe = FramePipeline(dict(synth.CELL_TYPES_5))
    res = pipe.run(synth.gen_batch_torch(10_000, B, H, W, dev))
    res.synchronize()
    K = len(pipe.tables_.slot_names)
    pos = torch.arange(B, dtype=torch.int64, device=dev)
    _, d = ops._dense_tables(res, res.get("groups") or {}, pos, 5, (), True)
    rt = ops.refined_tables(res, pos, pipe.tables_, d.ws, (d.n_roi, d.n_cell), check=True)
    out = {"batch": [B, H, W], "slots": K}
    for name, rows in (("cells", ops.class_rows(res)), ("refined", ops.refined_rows(res, rt["kind_r"], rt["slot_r"]))):
        labels, live, slot_of = rows.labels, rows.live.to(torch.uint8), rows.slot_of
        cap = live.shape[1]
        sels = [(live != 0) & (slot_of == t) for t in range(K)]
        gap2, partner = gaps.label_gaps(labels, live, slot_of, K)
        # frame 0: gap2 == 1 exactly where the label touches one of that slot; partners are live labels of the slot
        touch = touching(labels[0], live[0] != 0, slot_of[0], K)
        assert torch.equal((gap2[0] == 1) & (live[0] != 0)[:, None], touch)
        some = partner[0] > 0
        back = partner[0].to(torch.int64).clamp(min=1) - 1
        assert bool(((live[0] != 0)[back] | ~some).all())
        table = lambda: gaps.label_gaps(labels, live, slot_of, K)
        yard = lambda: [ops.nearest_label(labels, s, cap) for s in sels]
        kt_table, kt_yard = kernel_times(table), kernel_times(yard)
        t_table, t_yard = event_ms(table), event_ms(yard)
        n_live = (live != 0).sum(dim=1)
        out[name] = {"cap": cap, "live_per_frame": {"min": int(n_live.min()), "median": float(n_live.float().median()), "max": int(n_live.max())},
                     "label_gaps_ms": t_table, "nearest_label_per_slot_ms": t_yard, "ratio": round(t_table / t_yard, 3),
                     "with_gap": int((gap2 >= 0).sum()), "touching": int((gap2 == 1).sum()),
                     # (kernel_times cuts a name at "(": the templated row kernels, launched as "(name<RB>)", come back as "")
                     "label_gaps_kernels": {k or "gap_table_row_kernel": v for k, v in kt_table.items() if "gap_" in k or not k},
                     "nearest_label_kernels": {k or "vor_row_kernel": v for k, v in kt_yard.items() if "vor_" in k or "col_" in k or not k}}
    print(json.dumps(out, indent=1), flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
