"""What the pair-table wrappers return, stored so that two trees can be compared bit for bit.
``python profiles/pair_tables/outputs.py dump PACKAGE_ROOT OUT.npz`` runs PACKAGE_ROOT's package (with PCSEG_LIB set: that
library) on ``synth.gen_batch(9, 2, 256, 256)``: ``ops.territory_pairs`` with ``slot_of``, ``ops.label_contingency`` and
``ops.label_agreement`` of ``labels`` against ``ws_labels``, ``ops.label_borders`` (conn 4 and 8) and ``ops.merge_by_border``
(mean and saddle) of ``ws_labels`` on the boundary plane, ``FramePipeline.agreement``, ``FramePipeline.borders`` and the
adjacency and territory tables of ``tables_device`` (of the cells and of the refined ROIs).  Every tensor and array of the returned dicts
and tuples is stored under ``<call>/<key>``, other values as 0-d arrays.
``python profiles/pair_tables/outputs.py compare A.npz B.npz`` exits non-zero unless both files hold the same names with the
same dtypes, shapes and bytes."""
import sys

import numpy as np


def flat(out, name, v):
    import torch
    if isinstance(v, dict):
        for k, x in v.items():
            flat(out, "%s/%s" % (name, k), x)
    elif isinstance(v, (tuple, list)) and any(isinstance(x, (torch.Tensor, np.ndarray, dict)) for x in v):
        for i, x in enumerate(v):
            flat(out, "%s/%d" % (name, i), x)
    elif isinstance(v, torch.Tensor):
        out[name] = v.cpu().numpy()
    elif v is not None:
        out[name] = np.asarray(v)


def dump(root, path):
    sys.path.insert(0, root)
    import torch
    from particle_col_image_segmentation_amd import ops, synth
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    pipe = FramePipeline(dict(synth.CELL_TYPES_5))
    stack = torch.from_numpy(synth.gen_batch(9, 2, 256, 256)).cuda()
    res = pipe.run(stack)
    res.synchronize()
    T, S, V, counts = res["labels"], res["ws_labels"], stack[:, pipe.boundary_plane], res["n_markers"]
    cap = res["stats"].shape[1]
    rows = ops.class_rows(res)
    d2, near, _ = ops.nearest_label(rows.labels, rows.live.view(torch.uint8), cap)
    calls = {"territory_pairs": ops.territory_pairs(near, d2, -1, 8 * cap, slot_of=rows.slot_of, n_types=2),
             "territory_pairs_reach": ops.territory_pairs(near, d2, 9),
             "label_contingency": ops.label_contingency(T, S),
             "label_agreement": ops.label_agreement(T, S),
             "label_borders_4": ops.label_borders(S, V, conn=4),
             "label_borders_8": ops.label_borders(S, V, conn=8),
             "merge_by_mean": ops.merge_by_border(S, V, 0.3, by="mean", counts=counts),
             "merge_by_saddle": ops.merge_by_border(S, V, 0.3, by="saddle", counts=counts),
             "pipe_agreement": pipe.agreement(res, T),
             "pipe_borders": pipe.borders(res)}
    dt = pipe.tables_device(res, territory=True, territory_reach=3.0, refined=True, check=False)
    calls["tables_device"] = {k: dt[k] for k in dt if "adjacency" in k or "territor" in k}
    assert "adjacency" in calls["tables_device"] and "territories" in calls["tables_device"]
    out = {}
    flat(out, "", calls)
    np.savez(path, **out)
    print("%d arrays, %d bytes" % (len(out), sum(a.nbytes for a in out.values())))


def compare(a_path, b_path):
    a, b = np.load(a_path, allow_pickle=False), np.load(b_path, allow_pickle=False)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            bad.append(k)
    print("%s vs %s: %d arrays, %s" % (a_path, b_path, len(a.files), "identical" if not bad else "DIFFERENT: %s" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(dump(*sys.argv[2:4]) if sys.argv[1] == "dump" else compare(*sys.argv[2:4]))
