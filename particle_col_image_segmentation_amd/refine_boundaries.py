"""Boundary refinement: the reference's ``refine_boundaries.py`` as a function.

The reference file is an unguarded script (refine_boundaries.py:27-79): it loads
an ilastik probabilities ``.h5``, takes channel 3 as the boundary map,
thresholds at 0.5, and runs EDT -> local maxima -> label -> marker-controlled
watershed.  Here the same chain is a function over the HIP kernels, plus a
script-compatible ``__main__``.
"""
import numpy as np
import torch

from . import ops
from .tiff_analysis import _device

DEFAULT_FILE = "working_folder/Tp_C3M10_1_120h_60X_RFP_GFP_1_MIP_probabilities.h5"  # refine_boundaries.py:28
BOUNDARY_CHANNEL = 3  # refine_boundaries.py:34
THRESHOLD = 0.5  # refine_boundaries.py:44


def refine_boundaries_batch(boundary_maps, threshold=THRESHOLD, mode=0, marker_h=None, merge_below=None, merge_by="mean", merge_conn=8):
    """(B,H,W) float32 CUDA tensor -> dict of device stages (refine_boundaries.py:44-73).

    ``marker_h`` (pixels of the distance map; None: the script's chain): the markers are the maxima of the distance map that
    rise at least ``marker_h`` above their surroundings (``skimage.morphology.h_maxima(distance, marker_h)``) instead of
    every local maximum, ``local_max`` is their mask, and the dict gains ``marker_flags`` int32 (B,): non-zero where the
    frame's reconstruction did not reach its fixed point and the frame is no result (``ops.reconstruct``).

    ``merge_below`` (a boundary probability in [0, 1]; None: the chain as it was, nothing more is launched): after the flood,
    touching regions whose border is weaker than ``merge_below`` in ``boundary_maps`` itself are joined
    (``ops.merge_by_border`` with ``by=merge_by``, ``conn=merge_conn``: one pass over the region adjacency graph, the remedy
    for one cell cut in pieces by two maxima of its distance map).  ``labels`` is then the merged image and the dict gains
    ``labels_unmerged``, ``n_merged`` int32 (B,), ``merge_map`` int32 (B, cap + 1) and ``border_flags`` int32 (B,)
    (:func:`check_border_flags`); ``markers`` / ``n_markers`` stay the flood's."""
    d2, mask = ops.edt_sq_lt(boundary_maps, threshold)          # :44-45, :60
    st = {}
    if marker_h is None:
        local_max, markers, n_markers = ops.local_maxima(d2)    # :63-64
    else:
        local_max, markers, n_markers, st["marker_flags"] = ops.edt_maxima(d2, marker_h)
    labels, tie_flags = ops.watershed(boundary_maps, markers, mask, mode=mode)  # :73
    if merge_below is not None:
        st["labels_unmerged"] = labels
        cap = max(int(n_markers.max().item()), 1)
        labels, st["n_merged"], st["merge_map"], st["border_flags"] = ops.merge_by_border(
            labels, boundary_maps, merge_below, by=merge_by, conn=merge_conn, counts=n_markers, cap=cap)
    st.update({"binary_mask": mask, "distance_sq": d2, "local_max": local_max, "markers": markers,
               "n_markers": n_markers, "labels": labels, "tie_flags": tie_flags})
    return st


def check_marker_flags(st):
    """RuntimeError where the h-maxima markers of a frame are no result (``marker_flags`` of refine_boundaries_batch)."""
    flags = st.get("marker_flags")
    if flags is not None and int((flags != 0).sum().item()):
        raise RuntimeError("the h-maxima markers did not converge in frame(s) %s"
                           % [int(b) for b in torch.nonzero(flags.cpu())[:, 0]])


def check_border_flags(st):
    """RuntimeError where the border merge of a frame is no result (``border_flags`` of refine_boundaries_batch)."""
    ops.check_border_flags(st.get("border_flags"))


def refine_boundaries(boundary_map, threshold=THRESHOLD, return_stages=False, marker_h=None, merge_below=None, merge_by="mean",
                      merge_conn=8):
    """2-D boundary probability map -> int32 label image (the script's ``labels``).

    ``return_stages=True`` returns the script's globals instead: ``binary_mask``, ``distance`` (float64 =
    sqrt of the exact integer squared distance), ``local_max``, ``markers``, ``labels``.  ``marker_h``: see
    :func:`refine_boundaries_batch` (``local_max`` is then the h-maxima mask).  ``merge_below`` / ``merge_by`` /
    ``merge_conn``: its merge by border strength (``labels`` is then the merged image)."""
    was_tensor = isinstance(boundary_map, torch.Tensor)
    t = boundary_map if was_tensor else torch.from_numpy(np.ascontiguousarray(np.asarray(boundary_map, dtype=np.float32)))
    if t.dim() != 2:
        raise ValueError("expected a 2-D boundary map, got shape %s" % (tuple(t.shape),))
    t = t.to(device=_device(), dtype=torch.float32).contiguous()[None]
    st = refine_boundaries_batch(t, threshold, marker_h=marker_h, merge_below=merge_below, merge_by=merge_by, merge_conn=merge_conn)
    check_marker_flags(st)
    check_border_flags(st)
    conv = (lambda x: x) if was_tensor else (lambda x: x.cpu().numpy())
    labels = conv(st["labels"][0])
    if not return_stages:
        return labels
    d2 = st["distance_sq"][0]
    return {"binary_mask": conv(st["binary_mask"][0].bool()),
            "distance": conv(torch.sqrt(d2.to(torch.float64))),
            "local_max": conv(st["local_max"][0].bool()),
            "markers": conv(st["markers"][0]),
            "labels": labels}


def score_refinement(boundary_maps, truth, thresholds=(THRESHOLD,), marker_hs=(None,), iou_thresholds=(0.5, 0.75, 0.9),
                     merge_belows=(None,)):
    """The sweep over the chain's knobs: :func:`refine_boundaries_batch` once per (threshold, marker_h, merge_below) on
    ``boundary_maps`` ((B, H, W) float32 CUDA tensor), each result scored against ``truth`` (int32 (B, H, W) CUDA label
    image, 0: background) on the device (``ops.label_agreement``).  Returns a list of dicts, one per setting in the order of
    ``itertools.product(thresholds, marker_hs, merge_belows)``: ``threshold``, ``marker_h``, ``merge_below``,
    ``frames_agreement`` (float64 numpy, one row per frame) and ``frames_agreement_columns`` as ``FramePipeline.agreement``
    returns them."""
    out = []
    truth_cap = max(int(truth.max().item()), 1)
    for threshold in thresholds:
        for marker_h in marker_hs:
            for merge_below in merge_belows:
                st = refine_boundaries_batch(boundary_maps, threshold, marker_h=marker_h, merge_below=merge_below)
                check_marker_flags(st)
                check_border_flags(st)
                ag = ops.label_agreement(truth, st["labels"], iou_thresholds, cap_t=truth_cap,
                                         cap_s=max(int(st["n_markers"].max().item()), 1))
                ops.check_agreement_overflow(ag)
                tables = ops.agreement_tables(ag)
                out.append({"threshold": threshold, "marker_h": marker_h, "merge_below": merge_below,
                            "frames_agreement": tables["frames_agreement"],
                            "frames_agreement_columns": tables["frames_agreement_columns"]})
    return out


def refine_from_h5(file_path=DEFAULT_FILE, channel=BOUNDARY_CHANNEL, threshold=THRESHOLD, return_stages=False, marker_h=None,
                   merge_below=None, merge_by="mean", merge_conn=8):
    """refine_boundaries.py:28-34 + the chain; ``.npy`` probability stacks are accepted without h5py."""
    if file_path.endswith(".npy"):
        probabilities = np.load(file_path, allow_pickle=False)
    else:
        try:
            import h5py
        except ImportError as e:  # pragma: no cover
            raise ImportError("reading .h5 probabilities needs h5py; save the stack as .npy instead") from e
        with h5py.File(file_path, "r") as f:
            probabilities = np.array(f["exported_data"])
    return refine_boundaries(probabilities[channel], threshold, return_stages, marker_h=marker_h, merge_below=merge_below,
                             merge_by=merge_by, merge_conn=merge_conn)


if __name__ == "__main__":  # script-compatible entry: same default path, prints the number of segments
    import sys
    out = refine_from_h5(sys.argv[1] if len(sys.argv) > 1 else DEFAULT_FILE)
    print("segments:", int(out.max()))
