"""Drop-in for the hot-path functions of the reference's ``tiff_analysis.py``.

Same names, positional arguments, return shapes and error behaviour as
ssilverman16/particle_col_image_segmentation ``tiff_analysis.py`` (cited per
function); the pixel work runs in the HIP kernels of ``libpcseg.so`` through
``ops`` -- there is no CPU path.  Images go in and come back as numpy arrays
(torch CUDA tensors are accepted and then returned as tensors).

Not reproduced on purpose (out of scope, SURVEY.md section 2: C9-C11, C13):
matplotlib plotting and the ``main()`` folder walk.
"""
import csv
import os

import numpy as np
import torch

from . import gaps, ops

# --- constants: tiff_analysis.py:47-82 (they are the reference's whole flag system)
BASE_TYPE_MAP = {1: "3D05", 2: "6B07", 3: "C3M10", 4: "Particle", 5: "Background"}
CELL_TYPES = ["3D05", "6B07", "C3M10"]
CHANNELS = ["RFP", "DAPI", "GFP"]
CHANNEL_MAP = {"RFP": "3D05", "DAPI": "6B07", "GFP": "C3M10"}
STRAIN_MAP = {"3D05": "RFP", "6B07": "DAPI", "C3M10": "GFP"}
MIN_CELL_AREA = {"3D05": 20, "6B07": 20, "C3M10": 20}
MIN_CLUSTER_AREA = {"3D05": 200, "6B07": 200, "C3M10": 370}
DENOISE_SIZE = 5
DILATION_RADIUS = 20
DISTANCE_THRESHOLD = 2
CELL_CLUSTER_DISTANCE_THRESHOLD = 5
DAPI_RFP_OVERLAP_THRESHOLD = 0.1
PX_TO_UM_CONV = 9.95


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("particle_col_image_segmentation_amd needs a ROCm GPU: the HIP path has no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _to_dev_u8(a):
    """(H, W) integer / bool image -> (1, H, W) uint8 CUDA tensor, plus 'caller passed a tensor'."""
    if isinstance(a, torch.Tensor):
        t = a
        was_tensor = True
    else:
        arr = np.asarray(a)
        if arr.dtype != np.uint8 and arr.dtype != bool and arr.size and (arr.min() < 0 or arr.max() > 255):
            raise ValueError("class maps must hold values 0..255")
        t = torch.from_numpy(np.ascontiguousarray(arr.astype(np.uint8, copy=False)))
        was_tensor = False
    if t.dim() != 2:
        raise ValueError("expected a 2-D image, got shape %s" % (tuple(t.shape),))
    return t.to(device=_device(), dtype=torch.uint8).contiguous()[None], was_tensor


def _back(t, was_tensor, dtype=None):
    if was_tensor:
        return t
    a = t.cpu().numpy()
    return a.astype(dtype) if dtype is not None else a


class _LabelImage:
    """Device label image of one frame with a lazily fetched host copy (for Region.coords) and, shared by the frame's
    regions, the lazily computed shape columns (``stats``: the frame's (1, cap, 8) region table on the device, ``n``: its
    label count)."""

    def __init__(self, dev_labels, stats=None, n=0):
        self.dev = dev_labels
        self._host = None
        self._stats, self._n, self._shape, self._hull, self._skeleton = stats, int(n), None, None, None

    @property
    def shape_columns(self):
        """(n, 12) float64 in the order of ``ops.SHAPE_COLUMNS``: ONE device call for the whole frame, at the first
        access to a shape attribute of any of its regions."""
        if self._shape is None:
            if self._stats is None:
                raise AttributeError("this region carries no label image to take its shape from")
            counts = torch.full((1,), self._n, dtype=torch.int32, device=self.dev.device)
            table, _ = ops.region_shape(self.dev[None], counts, cap=self._stats.shape[1])
            self._shape = ops.shape_properties(self._stats, table, counts)[0, :self._n].cpu().numpy()
        return self._shape

    @property
    def hull_columns(self):
        """(n, 4) float64 in the order of ``ops.HULL_COLUMNS``: ONE device call for the whole frame, at the first
        :func:`get_cell_convexity` that meets one of its regions."""
        if self._hull is None:
            if self._stats is None:
                raise AttributeError("this region carries no label image to take its shape from")
            counts = torch.full((1,), self._n, dtype=torch.int32, device=self.dev.device)
            table, _ = ops.region_hull(self.dev[None], counts, self._stats)
            self._hull = ops.hull_properties(self._stats, table, counts)[0, :self._n].cpu().numpy()
        return self._hull

    @property
    def skeleton_columns(self):
        """(n, 8) float64 in the order of ``ops.SKELETON_COLUMNS``: ONE device call for the whole frame, at the first
        :func:`get_cell_skeletons` that meets one of its regions."""
        if self._skeleton is None:
            if self._stats is None:
                raise AttributeError("this region carries no label image to take its shape from")
            counts = torch.full((1,), self._n, dtype=torch.int32, device=self.dev.device)
            peel, _ = ops.thin_labels(self.dev[None])
            table = ops.region_skeleton(self.dev[None], peel, counts, cap=self._stats.shape[1])
            props = ops.skeleton_properties(self._stats, table, counts)
            self._skeleton = torch.cat([table.to(torch.float64), props], dim=2)[0, :self._n].cpu().numpy()
        return self._skeleton

    @property
    def host(self):
        if self._host is None:
            self._host = self.dev.cpu().numpy()
        return self._host


class Region:
    """Duck type of skimage RegionProperties restricted to what the reference touches:
    .label (:270), .area (:275, 769-781, 855, 1031, 1055), ["area"] (:1033), .centroid (:406, 844, 1054),
    .bbox (:860-863, 912), .coords[0] (:1042), dynamically added .cells (:781, 1029, 1063); refined regions
    (get_refined_cell_positions_and_areas) also carry .parent, the class-map label they lie in.

    What a cell looks like, under scikit-image 0.18.3's names and conventions and in pixels: .inertia_tensor,
    .inertia_tensor_eigvals, .major_axis_length, .minor_axis_length, .eccentricity, .orientation, .equivalent_diameter,
    .extent, .perimeter.  They are lazy: the regions of a frame share one holder, the first access to any of them costs
    one device call for the whole frame (csrc/shape.hip), a caller that never asks pays nothing.  Any other
    RegionProperties attribute raises AttributeError."""

    __slots__ = ("label", "area", "centroid", "bbox", "first", "sum_row", "sum_col", "cells", "parent", "_im")

    def __init__(self, label_id, row, width, label_image=None):
        self.label = int(label_id)
        # numpy scalars on purpose: the reference's CSV writers call round() on them, and numpy's round
        # (x*10^n -> rint -> /10^n) differs from Python's float round on decimal ties (tiff_analysis.py:1057)
        self.area = np.int64(row[0])
        self.sum_row = int(row[1])
        self.sum_col = int(row[2])
        # np.mean of integer coordinates = float64(sum) / count (skimage/measure/_regionprops.py:296-297)
        self.centroid = (np.float64(row[1]) / np.float64(row[0]), np.float64(row[2]) / np.float64(row[0]))
        self.bbox = (int(row[3]), int(row[4]), int(row[5]), int(row[6]))
        self.first = (int(row[7]) // width, int(row[7]) % width)
        self._im = label_image

    @property
    def coords(self):
        if self._im is None:
            return np.array([self.first])
        return np.argwhere(self._im.host == self.label)

    def _shape(self, k):
        if self._im is None:
            raise AttributeError("this region carries no label image to take its shape from")
        return self._im.shape_columns[self.label - 1, k]

    @property
    def inertia_tensor(self):
        a, b, c = (self._shape(k) for k in range(3))
        return np.array([[a, b], [b, c]])

    @property
    def inertia_tensor_eigvals(self):
        return [self._shape(3), self._shape(4)]

    major_axis_length = property(lambda self: self._shape(5))
    minor_axis_length = property(lambda self: self._shape(6))
    eccentricity = property(lambda self: self._shape(7))
    orientation = property(lambda self: self._shape(8))
    equivalent_diameter = property(lambda self: self._shape(9))
    extent = property(lambda self: self._shape(10))
    perimeter = property(lambda self: self._shape(11))

    def __getitem__(self, key):
        return getattr(self, key)


def median_filter(ds_arr, size=DENOISE_SIZE):
    """scipy.ndimage.median_filter(ds_arr, size=5) as called at tiff_analysis.py:122, 643."""
    if size != 5:
        raise ValueError("only size=5 (DENOISE_SIZE) is built")
    t, was = _to_dev_u8(ds_arr)
    return _back(ops.median5(t)[0], was)


def label(image):
    """skimage.measure.label(image) as called at tiff_analysis.py:743 (int) and :260, :829 (bool)."""
    is_bool = (image.dtype == torch.bool) if isinstance(image, torch.Tensor) else (np.asarray(image).dtype == bool)
    t, was = _to_dev_u8(image)
    lab, _ = (ops.label_bool8 if is_bool else ops.label_equal8)(t)
    return _back(lab[0], was, np.int64 if not is_bool else np.int32)


def _regions_of(z_dev):
    """label + regionprops of one frame on the device: (regions, class at first pixel, label holder, and the device
    tensors stats / cls_out / counts that the classification and merge kernels take)."""
    labels, counts = ops.label_equal8(z_dev)
    n = int(counts[0].item())
    stats, cls_out, _, _ = ops.region_reduce(labels, counts, cls=z_dev, cap=max(n, 1))
    holder = _LabelImage(labels[0], stats, n)
    st = stats[0, :n].cpu().numpy()
    cl = cls_out[0, :n].cpu().numpy()
    width = z_dev.shape[2]
    regions = [Region(i + 1, st[i], width, holder) for i in range(n)]
    return regions, cl, holder, (stats, cls_out, counts)


def regionprops(label_im):
    """skimage.measure.regionprops(label_im) reduced to the fields the reference reads (tiff_analysis.py:746)."""
    if isinstance(label_im, torch.Tensor):
        lab = label_im.to(device=_device(), dtype=torch.int32).contiguous()[None]
    else:
        lab = torch.from_numpy(np.ascontiguousarray(np.asarray(label_im).astype(np.int32)))[None].to(_device())
    n = int(lab.max().item()) if lab.numel() else 0
    stats, _, _, _ = ops.region_reduce(lab, cap=max(n, 1))
    st = stats[0, :n].cpu().numpy()
    holder = _LabelImage(lab[0], stats, n)
    return [Region(i + 1, st[i], lab.shape[2], holder) for i in range(n) if st[i][0] > 0]


def get_type(region, data):
    """tiff_analysis.py:1041-1044."""
    point = getattr(region, "first", None)
    if point is None:
        point = region.coords[0]
    return data[point[0], point[1]]


def get_cell_positions_and_areas(z_slice, cell_types, merged=False):
    """tiff_analysis.py:742-789.  Returns (cell_pos, cell_clusters, particle_area, merged_clusters).

    The per-region decisions (Particle area, cell / cluster by the area thresholds of the region's type, cluster cell
    count = int(area // mean single-cell area)) are ``pcseg_classify_regions`` -- the kernel the batched pipeline uses
    -- and the host only files the regions under their type names."""
    z_dev, _ = _to_dev_u8(z_slice)
    regions, classes, _, (stats, cls_out, counts) = _regions_of(z_dev)
    for value in np.unique(classes):
        cell_types[int(value)]  # KeyError for an unmapped class value, as at :756
    tables = ops.ClassTables(cell_types, CELL_TYPES, MIN_CELL_AREA, MIN_CLUSTER_AREA)
    verdict = ops.classify_regions(stats, cls_out, counts, tables)
    n = len(regions)
    kind = verdict["kind"][0, :n].cpu().numpy()
    slot = verdict["slot_of"][0, :n].cpu().numpy()
    n_cells = verdict["cells"][0, :n].cpu().numpy()
    first_region = verdict["type_stats"][0, :, 3].cpu().numpy()
    # the reference's dicts are keyed in the order the types first appear among the regions (:763-765)
    order = sorted((int(first_region[t]), t) for t in range(len(tables.slot_names)) if first_region[t] != 0x7FFFFFFF)
    cell_pos = {tables.slot_names[t]: [] for _, t in order}
    cell_clusters = {tables.slot_names[t]: [] for _, t in order}
    if int(verdict["nan_flag"][0].item()):
        # a type with clusters but without a single cell: np.average([]) is NaN and int(NaN) raises (:776-781)
        raise ValueError("cannot convert float NaN to integer")
    for i in np.nonzero(kind)[0]:
        name = tables.slot_names[slot[i]]
        if kind[i] == 1:
            cell_pos[name].append(regions[i])
        else:
            regions[i].cells = int(n_cells[i])
            cell_clusters[name].append(regions[i])
    particle_area = int(verdict["particle_area"][0].item())
    merged_clusters = {}
    if merged:
        merged_clusters, _ = _clusters_from_distances(z_dev, stats, cell_pos, cell_clusters, cell_types, False)
    return cell_pos, cell_clusters, particle_area, merged_clusters


def get_refined_cell_positions_and_areas(z_slice, boundary_map, cell_types, threshold=0.5, marker_h=None, merge_below=None):
    """Goal 2 of refine_boundaries.py:1-12 for one frame: the watershed-refined ROIs of ``boundary_map`` (the chain of
    refine_boundaries.refine_boundaries) classified by the class-map component of ``z_slice`` they share the most
    pixels with (``ops.label_parent``), with the reference's own per-region loop (tiff_analysis.py:754-781) run on
    them.  Returns ``(cell_pos, cell_clusters, particle_area, resolution)``: refined ``Region``s per strain (keyed in
    first-appearance order, with ``.parent`` and, for clusters, ``.cells``), the class map's particle area, and per
    strain ``{"resolved": [class-map labels of clusters split into >= 2 refined cells / clusters], "residual":
    [(label, cells) of the other clusters], "count_integrated": cells + sum of the integrated cluster counts}``
    (-1 where a term is -1).  Raises ValueError as the reference loop does where a strain has refined clusters but no
    refined cell.  ``marker_h``: the h-maxima markers of ``refine_boundaries_batch`` (None: every local maximum);
    ``merge_below``: its merge of refined ROIs across borders weaker than this boundary probability (None: no merge)."""
    from .refine_boundaries import check_border_flags, check_marker_flags, refine_boundaries_batch
    z_dev, _ = _to_dev_u8(z_slice)
    bm = boundary_map if isinstance(boundary_map, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(np.asarray(boundary_map, dtype=np.float32)))
    if bm.dim() != 2 or tuple(bm.shape) != tuple(z_dev.shape[1:]):
        raise ValueError("boundary_map must be a 2-D map of the class map's shape %s, got %s"
                         % (tuple(z_dev.shape[1:]), tuple(bm.shape)))
    bm = bm.to(device=z_dev.device, dtype=torch.float32).contiguous()[None]
    regions, classes, holder, (stats, cls_out, counts) = _regions_of(z_dev)
    for value in np.unique(classes):
        cell_types[int(value)]  # KeyError for an unmapped class value, as at :756
    tables = ops.ClassTables(cell_types, CELL_TYPES, MIN_CELL_AREA, MIN_CLUSTER_AREA)
    verdict = ops.classify_regions(stats, cls_out, counts, tables)
    st = refine_boundaries_batch(bm, threshold, marker_h=marker_h, merge_below=merge_below)
    check_marker_flags(st)
    check_border_flags(st)
    ws_labels, n_markers = st["labels"], st.get("n_merged", st["n_markers"])
    n, m = len(regions), int(n_markers[0].item())
    cap = max(n, m, 1)
    cls_a = torch.zeros((1, cap), dtype=torch.uint8, device=z_dev.device)
    cls_a[:, :n] = cls_out[:, :n]
    ws_stats, _, _, _ = ops.region_reduce(ws_labels, n_markers, cap=cap)
    parent, _, _, cls_r, _ = ops.label_parent(holder.dev[None], ws_labels, n_markers, cls_a=cls_a, cap=cap, stats_r=ws_stats)
    rv = ops.classify_regions(ws_stats, cls_r, n_markers, tables)
    if int(rv["nan_flag"][0].item()):
        raise ValueError("cannot convert float NaN to integer")  # :776-781 on the refined regions
    wst = ws_stats[0, :m].cpu().numpy()
    r_kind = rv["kind"][0, :m].cpu().numpy()
    r_slot = rv["slot_of"][0, :m].cpu().numpy()
    r_cells = rv["cells"][0, :m].cpu().numpy()
    r_parent = parent[0, :m].cpu().numpy()
    first_region = rv["type_stats"][0, :, 3].cpu().numpy()
    order = sorted((int(first_region[t]), t) for t in range(len(tables.slot_names)) if first_region[t] != 0x7FFFFFFF)
    cell_pos = {tables.slot_names[t]: [] for _, t in order}
    cell_clusters = {tables.slot_names[t]: [] for _, t in order}
    r_holder = _LabelImage(ws_labels[0], ws_stats, m)
    for i in np.nonzero(r_kind)[0]:
        reg = Region(i + 1, wst[i], z_dev.shape[2], r_holder)
        reg.parent = int(r_parent[i])
        if r_kind[i] == 1:
            cell_pos[tables.slot_names[r_slot[i]]].append(reg)
        else:
            reg.cells = int(r_cells[i])
            cell_clusters[tables.slot_names[r_slot[i]]].append(reg)
    # cluster resolution: a class-map cluster with >= 2 refined children is counted by its children
    kind = verdict["kind"][0, :n].cpu().numpy()
    slot = verdict["slot_of"][0, :n].cpu().numpy()
    cells = verdict["cells"][0, :n].cpu().numpy()
    live = (r_kind >= 1) & (r_parent >= 1) & (r_parent <= n)
    children = np.bincount(r_parent[live] - 1, minlength=n)[:n]
    child_sum = np.bincount(r_parent[live] - 1, weights=np.maximum(r_cells[live], 0), minlength=n)[:n].astype(np.int64)
    child_neg = np.bincount(r_parent[live] - 1, weights=(r_cells[live] < 0), minlength=n)[:n] > 0
    resolution = {}
    for t, name in enumerate(tables.slot_names):
        res = {"resolved": [], "residual": [], "count_integrated": 0}
        neg = False
        for a in np.nonzero((kind >= 1) & (slot == t))[0]:
            if kind[a] == 1:
                res["count_integrated"] += 1
            elif children[a] >= 2:
                res["resolved"].append(int(a + 1))
                neg = neg or bool(child_neg[a])
                res["count_integrated"] += int(child_sum[a])
            else:
                res["residual"].append((int(a + 1), int(cells[a])))
                neg = neg or cells[a] < 0
                res["count_integrated"] += int(cells[a])
        if neg:
            res["count_integrated"] = -1
        if res["resolved"] or res["residual"] or res["count_integrated"]:
            resolution[name] = res
    return cell_pos, cell_clusters, int(verdict["particle_area"][0].item()), resolution


def get_cell_neighbour_distances(cell_pos, px_to_um=PX_TO_UM_CONV, edges=None):
    """Goal 3 of refine_boundaries.py:8-12 for one frame, on the regions of ``cell_pos`` (strain -> regions, as
    get_cell_positions_and_areas returns it): per strain a dict with ``labels`` (the regions' labels in list order),
    ``same_um`` / ``same_label`` (distance in um to the nearest OTHER region of the same strain and its label) and
    ``other_um`` / ``other_label`` (other strain -> the same for that strain); NaN / -1 where there is no such region.
    Distances are between raw centroids, ``sqrt(drow^2 + dcol^2) / px_to_um``.  With ``edges`` (increasing, from 0, in
    um) the pair histogram comes back as well: ``(per_strain, pair_hist)``, ``pair_hist[(a, b)]`` (strain names in
    ``cell_pos`` order, ``a`` before or equal to ``b``) = ``{"n_pairs", "bins", "over"}``."""
    names = list(cell_pos)
    if len(names) > 4:
        raise ValueError("at most 4 strains")
    regs = [(t, r) for t, name in enumerate(names) for r in cell_pos[name]]
    dev = _device()
    xy = torch.tensor([[float(r.centroid[1]), float(r.centroid[0])] for _, r in regs], dtype=torch.float64).reshape(-1, 2).to(dev)
    slot = torch.tensor([t for t, _ in regs], dtype=torch.int32).to(dev)
    ids = torch.tensor([int(r.label) for _, r in regs], dtype=torch.int32).to(dev)
    foff = torch.tensor([0, len(regs)], dtype=torch.int64).to(dev)
    K = max(len(names), 1)
    dist, nn_id, hist = ops.point_neighbours(xy, slot, ids, foff, K, px_to_um, edges)
    dist, nn_id = dist.cpu().numpy(), nn_id.cpu().numpy()
    out, row = {}, 0
    for t, name in enumerate(names):
        n = len(cell_pos[name])
        d, i = dist[row:row + n], nn_id[row:row + n]
        out[name] = {"labels": ids[row:row + n].cpu().numpy(), "same_um": d[:, t], "same_label": i[:, t],
                     "other_um": {o: d[:, u] for u, o in enumerate(names) if u != t},
                     "other_label": {o: i[:, u] for u, o in enumerate(names) if u != t}}
        row += n
    if edges is None:
        return out
    h = hist[0].cpu().numpy()
    pairs = [(a, b) for a in range(K) for b in range(a, K)]
    return out, {(names[a], names[b]): {"n_pairs": int(h[p, 0]), "bins": h[p, 1:-1], "over": int(h[p, -1])}
                 for p, (a, b) in enumerate(pairs) if b < len(names)}


MIXING_COLUMNS = ["frame", "slot_a", "slot_b", "bin", "r_lo_um", "r_hi_um", "n_perm", "obs", "mean", "lo", "hi", "n_le", "n_ge",
                  "cum_obs", "cum_mean", "cum_lo", "cum_hi", "cum_n_le", "cum_n_ge"]


def get_cell_mixing(cell_pos, edges, permutations=199, seed=0, px_to_um=PX_TO_UM_CONV):
    """Do the strains of one frame sit closer together or further apart than chance?  The random-labelling test of the
    pair-distance histogram (csrc/mixing.hip) on the regions of ``cell_pos`` (strain -> regions, as
    get_cell_positions_and_areas returns it; strain t of the dict is slot t): the regions stay where they are, their strain
    labels are shuffled ``permutations`` times (``seed``; frame key 0), and every bin ``[edges[k], edges[k + 1])`` (um,
    increasing from 0) of every strain pair is compared with the shuffled counts.  One device call.  Returns ``(columns,
    rows)``: the ``mixing`` table of ``FramePipeline.tables`` for this frame as numpy, one row per (slot_a <= slot_b, bin):
    ``obs`` the observed pairs, ``mean`` / ``lo`` / ``hi`` of the shuffled ones, ``n_le`` / ``n_ge`` how many shuffles
    gave at most / at least ``obs``, and ``cum_*`` the same for the counts summed over the bins 0 .. k.  The one-sided
    Monte Carlo p-values are ``(1 + n_ge) / (1 + n_perm)`` for attraction and ``(1 + n_le) / (1 + n_perm)`` for
    segregation.  The regions are taken in label order at the tables' positions (centroid_col + 1, centroid_row + 1), so
    the shuffles are those of the pipeline's table for a frame with id 0."""
    names = list(cell_pos)
    if len(names) > 4:
        raise ValueError("at most 4 strains")
    regs = sorted(((int(r.label), t, r) for t, name in enumerate(names) for r in cell_pos[name]), key=lambda v: v[:2])
    dev = _device()
    xy = torch.tensor([[float(r.centroid[1]) + 1.0, float(r.centroid[0]) + 1.0] for _, _, r in regs],
                      dtype=torch.float64).reshape(-1, 2).to(dev)
    slot = torch.tensor([t for _, t, _ in regs], dtype=torch.int32).to(dev)
    foff = torch.tensor([0, len(regs)], dtype=torch.int64).to(dev)
    K, P = max(len(names), 1), int(permutations)
    mix = ops.pair_label_mixing(xy, slot, foff, K, px_to_um, edges, P, seed=seed)
    host = {k: v[0].cpu().numpy().astype(np.float64) for k, v in mix.items()}
    e = np.asarray(edges, np.float64).reshape(-1)
    Q, m = host["obs"].shape
    ab = np.array([(a, b) for a in range(K) for b in range(a, K)], np.float64)
    per = np.full((Q, m), float(P))
    with np.errstate(invalid="ignore"):
        half = lambda c: [host[c + "obs"], host[c + "sum"] / per, host[c + "lo"], host[c + "hi"], host[c + "n_le"], host[c + "n_ge"]]
        cols = [np.zeros((Q, m)), np.repeat(ab[:, :1], m, 1), np.repeat(ab[:, 1:], m, 1), np.tile(np.arange(m, dtype=np.float64), (Q, 1)),
                np.tile(e[:-1], (Q, 1)), np.tile(e[1:], (Q, 1)), per] + half("") + half("cum_")
    return list(MIXING_COLUMNS), np.stack(cols, axis=2).reshape(Q * m, -1)


def get_cell_convexity(cell_pos, px_to_um=PX_TO_UM_CONV):
    """One cell or a clump, for the regions of ``cell_pos`` (strain -> regions, as get_cell_positions_and_areas returns
    ``cell_pos`` or ``cell_clusters``): per strain a dict with ``labels`` (the regions' labels in list order) and, in the
    same order, ``convex_area`` (pixels of the convex hull image), ``solidity`` (area / convex_area: 1 for a convex cell,
    lower for a clump), ``feret_um`` (``feret_diameter_max / px_to_um``) and ``euler_number`` (8-connectivity), all equal to
    scikit-image 0.18.3's ``regionprops`` values.  Lazy like the shape attributes: the regions of a frame share one
    holder, the first call costs one device call for the frame (csrc/hull.hip), later ones none.  The regions themselves
    gain no attribute."""
    out = {}
    for name, regs in cell_pos.items():
        rows = []
        for r in regs:
            if r._im is None:
                raise AttributeError("this region carries no label image to take its shape from")
            rows.append(r._im.hull_columns[r.label - 1])
        t = np.array(rows, np.float64).reshape(-1, 4)
        out[name] = {"labels": np.array([int(r.label) for r in regs], np.int32), "convex_area": t[:, 0], "solidity": t[:, 1],
                     "feret_um": t[:, 2] / px_to_um, "euler_number": t[:, 3]}
    return out


def get_cell_skeletons(cell_pos, px_to_um=PX_TO_UM_CONV):
    """How long and how wide, for the regions of ``cell_pos`` (strain -> regions, as get_cell_positions_and_areas returns
    ``cell_pos`` or ``cell_clusters``): per strain a dict with ``labels`` (the regions' labels in list order) and, in the same
    order, the skeleton of ``skimage.morphology.thin`` of every region (scikit-image 0.18.3) as ``skel_px``, ``n_orth`` /
    ``n_diag`` (its orthogonal and diagonal links), ``n_end`` / ``n_junction`` (pixels with one link, with three or more:
    two ends and no junction is one rod, a junction a clump), ``passes`` (the full iterations the region took),
    ``length_um`` ((n_orth + n_diag sqrt 2) / px_to_um) and ``width_um`` (area / length in pixels, / px_to_um).  Lazy like
    :func:`get_cell_convexity`: the regions of a frame share one holder, the first call costs one device call for the
    frame (csrc/skeleton.hip), later ones none.  The regions themselves gain no attribute."""
    out = {}
    cols = ops.SKELETON_COLUMNS
    for name, regs in cell_pos.items():
        rows = []
        for r in regs:
            if r._im is None:
                raise AttributeError("this region carries no label image to take its shape from")
            rows.append(r._im.skeleton_columns[r.label - 1])
        t = np.array(rows, np.float64).reshape(-1, len(cols))
        out[name] = {"labels": np.array([int(r.label) for r in regs], np.int32), **{c: t[:, k] for k, c in enumerate(cols[:6])},
                     "length_um": t[:, 6] / px_to_um, "width_um": t[:, 7] / px_to_um}
    return out


def get_segmentation_agreement(truth_labels, labels, thresholds=(0.5, 0.75, 0.9)):
    """How well the label image ``labels`` agrees with the truth label image ``truth_labels`` (both (H, W), integers, 0:
    background; numpy arrays or tensors): ``ops.label_agreement`` for ONE frame -- the same dict without the frame
    dimension, its arrays numpy if both images came as numpy.  ``t``, ``s``, ``n``: the pairs of labels that share pixels;
    ``best_s`` / ``iou_s`` / ``match_s``: per label of ``labels`` its best truth label (row l - 1), the IoU and the
    thresholds it is matched at; ``scores``: precision, recall, f1, ap per threshold, the adapted Rand error and the
    variation of information of the frame (csrc/agreement.hip)."""
    was_tensor = isinstance(truth_labels, torch.Tensor) or isinstance(labels, torch.Tensor)
    dev = _device()

    def frame(a):
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int32)))
        if t.dim() != 2:
            raise ValueError("expected a 2-D label image, got shape %s" % (tuple(t.shape),))
        return t.to(device=dev, dtype=torch.int32).contiguous()[None]
    ag = ops.label_agreement(frame(truth_labels), frame(labels), thresholds)
    ops.check_agreement_overflow(ag)
    conv = (lambda x: x) if was_tensor else (lambda x: x.cpu().numpy())
    out = {}
    for k, v in ag.items():
        if k == "scores":
            out[k] = {name: col[0] for name, col in v.items()}
        elif k in ("t", "s", "n"):
            out[k] = conv(v)
        elif k == "frame":
            continue
        elif isinstance(v, torch.Tensor):
            out[k] = conv(v[0])
        else:
            out[k] = v
    return out


def get_cell_territories(z_slice, cell_pos, cell_clusters, cell_types, reach=None, px_to_um=PX_TO_UM_CONV):
    """How much of the frame every cell has to itself and which cells are its neighbours (csrc/voronoi.hip): the regions
    of ``cell_pos`` and ``cell_clusters`` (strain -> regions of ONE denoised class map ``z_slice``, as
    get_cell_positions_and_areas returns them) are the sites of the exact nearest-label transform; a pixel belongs to the
    nearest of them (the smallest label among equally near ones) if it lies closer than ``reach`` um (None: unbounded).
    Returns a dict: ``names`` (the strains: type slot k = ``names[k]``), ``territories`` float64 (n, 8 + 2 K) in label order
    with ``territories_columns`` = label, slot, territory_px, territory_on_px (the part on the reconstructed, hole-filled
    particle), reach2_max, clipped, n_adj_<strain>.., n_contact_<strain>.., territory_um2, territory_on_um2, and
    ``adjacency`` float64 (m, 6) sorted by (label_a, label_b) with ``adjacency_columns`` = label_a, label_b, slot_a, slot_b,
    border_px (4-neighbour links between the two territories), contact_px (those where the regions themselves touch).
    One device call chain for the frame."""
    cell_clusters = cell_clusters or {}
    names = list(cell_pos) + [n for n in cell_clusters if n not in cell_pos]
    if len(names) > 4:
        raise ValueError("at most 4 strains")
    regs = [(t, r) for t, name in enumerate(names) for r in list(cell_pos.get(name, [])) + list(cell_clusters.get(name, []))]
    z_dev, _ = _to_dev_u8(z_slice)
    dev = z_dev.device
    holders = {id(r._im): r._im for _, r in regs}
    if None in [r._im for _, r in regs] or len(holders) > 1:
        raise AttributeError("the regions must carry the label image of one frame")
    K = max(len(names), 1)
    cols_t = (["label", "slot", "territory_px", "territory_on_px", "reach2_max", "clipped"] + ["n_adj_%s" % n for n in names]
              + ["n_contact_%s" % n for n in names] + ["territory_um2", "territory_on_um2"])
    cols_a = ["label_a", "label_b", "slot_a", "slot_b", "border_px", "contact_px"]
    out = {"names": names, "territories_columns": cols_t, "adjacency_columns": cols_a}
    if not regs:
        out.update(territories=np.zeros((0, len(cols_t))), adjacency=np.zeros((0, 6)))
        return out
    labels = next(iter(holders.values())).dev[None]
    cap = max(r.label for _, r in regs)
    live, slot_of = np.zeros((1, cap), bool), np.full((1, cap), 255, np.uint8)
    for t, r in regs:
        live[0, r.label - 1], slot_of[0, r.label - 1] = True, t
    cell_labels = [label for label, name in cell_types.items() if name in CELL_TYPES]
    particle_labels = [label for label, name in cell_types.items() if name == "Particle"]
    particle_label = particle_labels[-1] if particle_labels else None
    gained = None
    for cell_label in (cell_labels if particle_label is not None else []):
        z_dev, gained = ops.fill_particle(z_dev, particle_label, cell_label, particle_label, DILATION_RADIUS, DISTANCE_THRESHOLD,
                                          gained)
    rows, adj, _ = ops.territory_rows(labels, torch.from_numpy(live).to(dev), torch.from_numpy(slot_of).to(dev),
                                      torch.zeros((1,), dtype=torch.int64, device=dev), float(px_to_um), len(names),
                                      r2=ops.reach_um_r2(reach, float(px_to_um)), mask=ops.particle_mask(z_dev, particle_label),
                                      check=True)
    out.update(territories=rows.cpu().numpy()[:, 1:], adjacency=adj.cpu().numpy()[:, 1:])
    return out


def get_cell_gaps(cell_pos, cell_clusters=None, reach=None, px_to_um=PX_TO_UM_CONV):
    """How far every cell is from the nearest OTHER cell of each strain, rim to rim (csrc/gaps.hip; refine_boundaries.py:8-12,
    goal 3, between the regions' pixels instead of their centroids): the regions of ``cell_pos`` and ``cell_clusters``
    (strain -> regions of ONE frame, as get_cell_positions_and_areas returns them, all carrying one label image).  Returns
    a dict: ``names`` (the strains: type slot k = ``names[k]``, at most 4) and ``gaps`` float64 (n, 2 + 3 K) in label order
    with ``gaps_columns`` = label, slot, gap_um_<strain>.. (the smallest distance between a pixel of the region and a pixel
    of another region of that strain, / px_to_um; NaN where there is none closer than ``reach`` um, None: unbounded),
    gap_label_<strain>.. (that region's label, the smallest among equally near ones; -1 for none), gap_px2_<strain>.. (the
    squared gap in pixels; 1: the two touch along an edge; -1 for none).  One device call chain for the frame."""
    cell_clusters = cell_clusters or {}
    names = list(cell_pos) + [n for n in cell_clusters if n not in cell_pos]
    if len(names) > 4:
        raise ValueError("at most 4 strains")
    regs = [(t, r) for t, name in enumerate(names) for r in list(cell_pos.get(name, [])) + list(cell_clusters.get(name, []))]
    holders = {id(r._im): r._im for _, r in regs}
    if None in [r._im for _, r in regs] or len(holders) > 1:
        raise AttributeError("the regions must carry the label image of one frame")
    out = {"names": names, "gaps_columns": gaps.gap_columns(names)[1:]}
    if not regs:
        out["gaps"] = np.zeros((0, 2 + 3 * len(names)))
        return out
    labels = next(iter(holders.values())).dev[None]
    dev = labels.device
    cap = max(r.label for _, r in regs)
    live, slot_of = np.zeros((1, cap), bool), np.full((1, cap), 255, np.uint8)
    for t, r in regs:
        live[0, r.label - 1], slot_of[0, r.label - 1] = True, t
    rows = gaps.gap_rows(labels, torch.from_numpy(live).to(dev), torch.from_numpy(slot_of).to(dev),
                         torch.zeros((1,), dtype=torch.int64, device=dev), float(px_to_um), names,
                         r2=ops.reach_um_r2(reach, float(px_to_um)))
    out["gaps"] = rows.cpu().numpy()[:, 1:]
    return out


def get_cell_surface_distances(z_slice, cell_types, cell_pos=None, cell_clusters=None, px_to_um=PX_TO_UM_CONV, edges=None):
    """Where the cells of one denoised class map sit relative to the particle
    (HCN_nanosims_rois_activity_distance_5iso_YG.m:271-309, the distance of every ROI to the aggregate boundary): the
    particle is reconstructed as ``recreate_particle_area`` does, its holes are filled, and every region of ``cell_pos``
    and ``cell_clusters`` (strain -> regions; those of ``get_cell_positions_and_areas`` when none are passed) is measured
    from its centroid to the nearest pixel of that mask's surface.  Returns per strain a list of ``(region, inside,
    distance_um, (nearest_row, nearest_col))`` (cells first, then clusters): ``inside`` = the centroid's pixel lies in
    the filled particle, ``distance_um = sqrt(drow^2 + dcol^2) / px_to_um``; ``(False, nan, (-1, -1))`` without a
    particle.  With ``edges`` (increasing, from 0, in um) also the two histograms of a colonisation profile:
    ``(per_strain, {"hist": {(side, strain): {"n", "bins", "over"}}, "shells": {side: {"n_px", "bins", "over"}}})``,
    side 0 = outside the particle, 1 = inside; regions per um2 of a shell = hist bins / (shell bins / px_to_um^2)."""
    if cell_pos is None:
        cell_pos, found_clusters, _, _ = get_cell_positions_and_areas(z_slice, cell_types)
        cell_clusters = found_clusters if cell_clusters is None else cell_clusters
    cell_clusters = cell_clusters or {}
    names = list(cell_pos) + [n for n in cell_clusters if n not in cell_pos]
    if len(names) > 4:
        raise ValueError("at most 4 strains")
    regs = [(t, r) for t, name in enumerate(names) for r in list(cell_pos.get(name, [])) + list(cell_clusters.get(name, []))]
    z_dev, _ = _to_dev_u8(z_slice)
    dev = z_dev.device
    cell_labels = [label for label, name in cell_types.items() if name in CELL_TYPES]
    particle_labels = [label for label, name in cell_types.items() if name == "Particle"]
    particle_label = particle_labels[-1] if particle_labels else None
    gained = None
    for cell_label in (cell_labels if particle_label is not None else []):
        z_dev, gained = ops.fill_particle(z_dev, particle_label, cell_label, particle_label, DILATION_RADIUS, DISTANCE_THRESHOLD,
                                          gained)
    mask, surface = ops.particle_surface(z_dev, particle_label)
    rc = torch.tensor([[float(r.centroid[0]), float(r.centroid[1])] for _, r in regs], dtype=torch.float64).reshape(-1, 2).to(dev)
    slot = torch.tensor([t for t, _ in regs], dtype=torch.int32).to(dev)
    foff = torch.tensor([0, len(regs)], dtype=torch.int64).to(dev)
    K = max(len(names), 1)
    dist, nearest, inside, hist = ops.surface_distances(rc, foff, surface, px_to_um, mask=mask, slot=slot, n_types=K, edges=edges)
    dist, nearest, inside = dist.cpu().numpy(), nearest.cpu().numpy(), inside.cpu().numpy()
    out = {name: [] for name in names}
    for i, (t, r) in enumerate(regs):
        out[names[t]].append((r, bool(inside[i]), float(dist[i]), (int(nearest[i, 0]), int(nearest[i, 1]))))
    if edges is None:
        return out
    h = hist[0].cpu().numpy()
    sh = ops.surface_shells(surface, mask, edges, px_to_um)[0].cpu().numpy()
    return out, {"hist": {(side, name): {"n": int(h[side, t, 0]), "bins": h[side, t, 1:-1], "over": int(h[side, t, -1])}
                          for side in (0, 1) for t, name in enumerate(names)},
                 "shells": {side: {"n_px": int(sh[side, 0]), "bins": sh[side, 1:-1], "over": int(sh[side, -1])} for side in (0, 1)}}


def _window_points(who, z_slice, cell_types, cell_pos, cell_clusters, edges, window):
    """What :func:`get_cell_clustering` and :func:`get_cell_neighbourhoods` are made from, after their refusals: ``(names, z_dev,
    mask, points, rc)`` -- the strains in slot order, the class map as a (1, H, W) uint8 CUDA tensor, the window as one, the
    regions of ``cell_pos`` and ``cell_clusters`` as :class:`ops.Points` (positions as the pair tables take them) and their
    (row, col) centroids."""
    if edges is None:
        raise ValueError("%s needs edges" % who)
    if isinstance(window, str) and window not in ("particle", "frame"):
        raise ValueError('window must be "particle", "frame" or an (H, W) mask')
    if cell_pos is None:
        cell_pos, found_clusters, _, _ = get_cell_positions_and_areas(z_slice, cell_types)
        cell_clusters = found_clusters if cell_clusters is None else cell_clusters
    cell_clusters = cell_clusters or {}
    names = list(cell_pos) + [n for n in cell_clusters if n not in cell_pos]
    if len(names) > 4:
        raise ValueError("at most 4 strains")
    regs = [(t, r) for t, name in enumerate(names) for r in list(cell_pos.get(name, [])) + list(cell_clusters.get(name, []))]
    z_dev, _ = _to_dev_u8(z_slice)
    dev = z_dev.device
    if not isinstance(window, str):
        mask = (torch.as_tensor(np.asarray(window.cpu() if isinstance(window, torch.Tensor) else window)) != 0).to(torch.uint8)
        mask = mask.reshape((1,) + tuple(z_dev.shape[-2:])).to(dev)
    elif window == "frame":
        mask = torch.ones_like(z_dev)
    else:
        particle_labels = [label for label, name in cell_types.items() if name == "Particle"]
        particle_label = particle_labels[-1] if particle_labels else None
        gained = None
        filled = z_dev
        for cell_label in ([label for label, name in cell_types.items() if name in CELL_TYPES] if particle_label is not None else []):
            filled, gained = ops.fill_particle(filled, particle_label, cell_label, particle_label, DILATION_RADIUS, DISTANCE_THRESHOLD,
                                               gained)
        mask = ops.particle_mask(filled, particle_label)
    rc = torch.tensor([[float(r.centroid[0]), float(r.centroid[1])] for _, r in regs], dtype=torch.float64).reshape(-1, 2).to(dev)
    xy = torch.stack([rc[:, 1] + 1.0, rc[:, 0] + 1.0], dim=1)  # positions as the pair tables take them (pcseg_point_neighbours)
    points = ops.Points(xy, torch.tensor([t for t, _ in regs], dtype=torch.int32).to(dev),
                        torch.tensor([int(r.label) for _, r in regs], dtype=torch.int32).to(dev),
                        torch.tensor([0, len(regs)], dtype=torch.int64).to(dev))
    return names, z_dev, mask, points, rc


def get_cell_clustering(z_slice, cell_types, cell_pos=None, cell_clusters=None, edges=None, window="particle", px_to_um=PX_TO_UM_CONV):
    """Are the cells of one denoised class map clumped or spread evenly over the window they can sit in?  The two tables of
    ``FramePipeline.clustering`` (which describes them) for one frame: ``window_pairs`` and ``clustering`` with their
    ``<name>_columns``, frame 0.  The points are the regions of ``cell_pos`` and ``cell_clusters`` (strain -> regions; those
    of ``get_cell_positions_and_areas`` when none are passed) at their centroids, the slots the strains in ``cell_pos`` order;
    ``window``: "particle" (the particle reconstructed as ``recreate_particle_area`` does, holes filled: the mask of
    ``get_cell_surface_distances``), "frame" or an (H, W) mask of the caller's; ``edges`` (increasing, from 0) in um."""
    from . import spatial
    names, _, mask, points, rc = _window_points("get_cell_clustering", z_slice, cell_types, cell_pos, cell_clusters, edges, window)
    out = {k: v.cpu().numpy() for k, v in
           spatial._clustering_tables(points, rc, mask, edges, px_to_um, max(len(names), 1), np.zeros(1)).items()}
    out.update((k + "_columns", v) for k, v in spatial.clustering_columns(edges).items())
    return out


def get_cell_neighbourhoods(z_slice, cell_types, cell_pos=None, cell_clusters=None, edges=None, window="particle", px_to_um=PX_TO_UM_CONV):
    """What lies around every cell of one denoised class map: the table of ``FramePipeline.neighbourhoods`` (which describes
    it) for one frame, ``neighbourhoods`` with ``neighbourhoods_columns``, frame 0.  Points, slots, ``window`` and ``edges`` as in
    :func:`get_cell_clustering`; the pixels of strain t are the pixels of ``z_slice`` whose class value ``cell_types`` maps to
    the strain of slot t."""
    from . import local
    names, z_dev, mask, points, rc = _window_points("get_cell_neighbourhoods", z_slice, cell_types, cell_pos, cell_clusters, edges,
                                                    window)
    K = max(len(names), 1)
    slot = np.full(256, 255, np.uint8)
    for value, name in cell_types.items():
        if name in names and 0 <= int(value) < 256:
            slot[int(value)] = names.index(name)
    planes = local.set_planes(mask, z_dev, slot)
    out = {k: v.cpu().numpy() for k, v in local.neighbourhood_tables(points, rc, planes, edges, px_to_um, K, np.zeros(1)).items()}
    out["neighbourhoods_columns"] = local.neighbourhood_columns(names if names else K, edges)
    return out


def _group_regions(dl_dev, stats_dev, og_cell_regions):
    """device grouping (pcseg_merge_groups) + host assembly of the reference's merged-region dicts (:850-872)."""
    n = len(og_cell_regions)
    dev = dl_dev.device
    lst = torch.full((1, max(n, 1)), -1, dtype=torch.int32)
    if n:
        lst[0, :n] = torch.tensor([r.label - 1 for r in og_cell_regions], dtype=torch.int32)
    group_of, n_groups = ops.merge_groups(dl_dev, stats_dev, lst.to(dev), torch.tensor([n], dtype=torch.int32, device=dev))
    gof = group_of[0, :n].cpu().numpy()
    merged_regions = []
    for g in range(1, int(n_groups[0].item()) + 1):
        members = [og_cell_regions[k] for k in np.nonzero(gof == g)[0]]
        areas = [m.area for m in members]
        boxes = np.array([m.bbox for m in members])
        merged_regions.append({
            "area": sum(areas),
            "centroid": np.average([m.centroid for m in members], axis=0, weights=areas),
            "regions": members,
            "bbox": (boxes[:, 0].min(), boxes[:, 1].min(), boxes[:, 2].max(), boxes[:, 3].max()),
        })
    return merged_regions, gof


def _stats_from_regions(regions, dev):
    cap = max([r.label for r in regions], default=1)
    st = np.zeros((1, cap, 8), np.int64)
    for r in regions:
        st[0, r.label - 1, :3] = (r.area, r.sum_row, r.sum_col)
    return torch.from_numpy(st).to(dev)


def _merged_regions_dev(z_dev, value_bits, stats_dev, og_cell_regions, want_image):
    dil = ops.dilate_disk(z_dev, value_bits, CELL_CLUSTER_DISTANCE_THRESHOLD // 2)
    dl, dl_counts = ops.label_bool8(dil)
    merged_regions, _ = _group_regions(dl, stats_dev, og_cell_regions)
    merged_image = None
    if want_image:
        # union of the dilated components that hold a listed centroid, holes filled (:876-880)
        K = int(dl_counts[0].item())
        keep = torch.zeros((K + 1,), dtype=torch.uint8, device=dl.device)
        H, W = dl.shape[1:]
        ys = torch.tensor([min(max(int(r.centroid[0]), 0), H - 1) for r in og_cell_regions], dtype=torch.long, device=dl.device)
        xs = torch.tensor([min(max(int(r.centroid[1]), 0), W - 1) for r in og_cell_regions], dtype=torch.long, device=dl.device)
        if len(og_cell_regions):
            keep[dl[0, ys, xs].long()] = 1
        keep[0] = 0
        sel = keep[dl.long()]
        merged_image = ops.fill_holes(sel)[0].bool()
    return merged_regions, merged_image


def _clusters_from_distances(z_dev, stats_dev, cell_pos, cell_clusters, cell_types, want_images):
    """:791-824 on the device: one dilated-mask grouping per cell type over that type's cells + clusters, and one over
    all of them on the union of the masks ("combined").  The reference walks a set of the type names (hash-randomised
    order, :794); here the types come in the insertion order of the two dicts."""
    names = list(cell_pos) + [k for k in cell_clusters if k not in cell_pos]
    first_value = {}
    for value, name in cell_types.items():
        first_value.setdefault(name, value)  # the class value of a type is the FIRST key that maps to it (:806-810)
    merged_regions, merged_images = {}, {}
    everything, all_bits = [], 0
    for name in names:
        members = cell_pos.get(name, []) + cell_clusters.get(name, [])
        value = first_value.get(name, 0)
        all_bits |= 1 << value
        everything += members
        merged_regions[name], merged_images[name] = _merged_regions_dev(z_dev, 1 << value, stats_dev, members, want_images)
    merged_regions["combined"], merged_images["combined"] = _merged_regions_dev(z_dev, all_bits, stats_dev, everything, want_images)
    return merged_regions, merged_images


def get_cell_clusters_from_distances(z_slice, cell_pos, cell_clusters, cell_types):
    """tiff_analysis.py:791-824.  Returns (merged_regions, merged_images)."""
    z_dev, was = _to_dev_u8(z_slice)
    all_regions = [r for regs in list(cell_pos.values()) + list(cell_clusters.values()) for r in regs]
    stats_dev = _stats_from_regions(all_regions, z_dev.device)
    merged_regions, merged_images = _clusters_from_distances(z_dev, stats_dev, cell_pos, cell_clusters, cell_types, True)
    return merged_regions, {k: _back(v, was) for k, v in merged_images.items()}


def get_merged_regions(binary_image, og_cell_regions):
    """tiff_analysis.py:826-883.  Returns (merged_regions, merged_image)."""
    b_dev, was = _to_dev_u8(binary_image)
    b_dev = (b_dev != 0).to(torch.uint8)
    stats_dev = _stats_from_regions(og_cell_regions, b_dev.device)
    merged_regions, merged_image = _merged_regions_dev(b_dev, 1 << 1, stats_dev, og_cell_regions, True)
    return merged_regions, _back(merged_image, was)


def fill_particle_area(ds_arr, particle_label, cell_label, overlap_label):
    """tiff_analysis.py:982-1015.  Returns (updated_ds_arr, overlap_area); the input is not modified (:1010)."""
    ds_dev, was = _to_dev_u8(ds_arr)
    out, area = ops.fill_particle(ds_dev, particle_label, cell_label, overlap_label, DILATION_RADIUS, DISTANCE_THRESHOLD)
    res = _back(out[0], was)
    if not was:
        res = res.astype(np.asarray(ds_arr).dtype, copy=False)
    return res, int(area[0].item())


def recreate_particle_area(ds_arr, cell_types, particle_area):
    """tiff_analysis.py:931-950: one fill per cell class, each on the output of the previous one; the overlap areas
    are accumulated on the device and read once."""
    cell_labels = [label for label, name in cell_types.items() if name in CELL_TYPES]
    if not cell_labels:
        return ds_arr, particle_area
    particle_labels = [label for label, name in cell_types.items() if name == "Particle"]
    if not particle_labels:
        raise TypeError("no 'Particle' entry in cell_types")  # the reference fails inside fill_particle_area
    particle_label = particle_labels[-1]  # the last match wins in the reference's loop (:933-935)
    ds_dev, was = _to_dev_u8(ds_arr)
    gained = None
    for cell_label in cell_labels:
        ds_dev, gained = ops.fill_particle(ds_dev, particle_label, cell_label, particle_label, DILATION_RADIUS,
                                           DISTANCE_THRESHOLD, gained)
    res = _back(ds_dev[0], was)
    if not was:
        res = res.astype(np.asarray(ds_arr).dtype, copy=False)
    return res, particle_area + int(gained[0].item())


def get_cell_counts_and_densities(cell_pos, cell_clusters, particle_area):
    """tiff_analysis.py:1018-1038: count = cells + cells inside clusters; density and area ratio per um^2 of particle,
    both rounded to 5 decimals (Python's round on a Python float, as there)."""
    um2 = PX_TO_UM_CONV ** 2
    particle_um2 = particle_area / um2
    counts, densities, ratios = {}, {}, {}
    for name in (t for t in cell_pos if t in CELL_TYPES):
        clusters = cell_clusters[name]
        counts[name] = len(cell_pos[name]) + sum(c.cells for c in clusters)
        pixels = np.sum([np.int64(c.area) for c in cell_pos[name]])  # np.sum([]) is 0.0, like the reference's
        for c in clusters:
            pixels = pixels + c["area"]
        densities[name] = round(counts[name] / particle_um2, 5)
        ratios[name] = round((pixels / um2) / particle_um2, 5)
    return counts, densities, ratios


def combine_cell_positions_and_clusters(dapi_channel, other_channel):
    """tiff_analysis.py:252-287: drop DAPI cells that overlap cells of the other channel by > 10 %."""
    d_dev, was = _to_dev_u8(dapi_channel)
    o_dev, _ = _to_dev_u8(other_channel)
    out = ops.remove_overlapping(d_dev, o_dev, DAPI_RFP_OVERLAP_THRESHOLD)
    res = _back(out[0], was)
    if not was:
        res = res.astype(np.asarray(dapi_channel).dtype, copy=False)
    return res


def get_rfp_base_arr(rfp_arr, cell_strains):
    """Lift a per-channel RFP class map into the 5-class numbering, in place (tiff_analysis.py:224-231): without a
    3D05 strain the RFP channel holds (particle, background) = (1, 2), otherwise (cell, particle, background)."""
    particle, background = (1, 2) if cell_strains in (["6B07"], ["6B07", "C3M10"]) else (2, 3)
    rfp_arr[rfp_arr == particle] = 4   # order matters: the particle value is remapped before the background value
    rfp_arr[rfp_arr == background] = 5
    return rfp_arr


def combine_channels(rfp_base, channel_ds_arrs, cell_strains):
    """Paint the cells of every non-3D05 strain (value 1 of its own channel) into the RFP base map with the strain's
    value of BASE_TYPE_MAP (tiff_analysis.py:233-249)."""
    value_of = {name: val for val, name in BASE_TYPE_MAP.items()}
    for strain in cell_strains:
        if strain != "3D05":
            rfp_base[channel_ds_arrs[STRAIN_MAP[strain]] == 1] = value_of[strain]
    return rfp_base


def normalize_ds_arr(ds_arr):
    """Squeeze an ilastik export to (H, W) (tiff_analysis.py:727-737): (H, W, 1), (1, H, W) or exactly 2048 x 2048."""
    shape = ds_arr.shape
    if shape[-1] == 1:
        return np.squeeze(ds_arr)
    if shape[0] == 1:
        return ds_arr[0]
    if shape[0] == 2048 and shape[1] == 2048:
        return ds_arr
    raise ValueError(f"DS arr shape is not (2048,2048,1) or (1,2048,2048) or (2048,2048). Shape: {ds_arr.shape}")


def get_strains_from_file(file_name):
    """Strain names (in CELL_TYPES order) that occur in the upper-cased path (tiff_analysis.py:673-678)."""
    upper = file_name.upper()
    return [strain for strain in CELL_TYPES if strain in upper]


def get_channel_from_file(file_name):
    """The one fluorescence channel named in the file (tiff_analysis.py:680-687); IndexError without any."""
    upper = file_name.upper()
    found = [channel for channel in CHANNELS if channel in upper]
    if len(found) > 1:
        raise ValueError("More than one channel found in file path")
    return found[0]


def get_cell_type_map(file_path):
    """{1..k: strains named in the file, k+1: "Particle", k+2: "Background"} (tiff_analysis.py:694-702).  Like the
    reference this needs at least one strain in the name (UnboundLocalError otherwise)."""
    strains = get_strains_from_file(file_path)
    if not strains:
        raise UnboundLocalError("local variable 'i' referenced before assignment")
    cell_type_map = dict(enumerate(strains, start=1))
    cell_type_map[len(strains) + 1] = "Particle"
    cell_type_map[len(strains) + 2] = "Background"
    return cell_type_map


def get_cell_type_map_from_channel(strain_types, channel):
    """Class values of one channel file of a multi-channel sample (tiff_analysis.py:709-712)."""
    if channel == "RFP" and strain_types in (["6B07"], ["6B07", "C3M10"]):
        return {1: "Particle", 2: "Background"}
    return {1: CHANNEL_MAP[channel], 2: "Particle", 3: "Background"}


def get_pos_and_density_file_names(cur_folder):
    """tiff_analysis.py:619-624: (<grandparent>_<parent>_cell_density_info.csv next to the folder, <folder>_cell_pos.csv in it)."""
    parts = cur_folder.split("/")
    density_csv = os.path.join(cur_folder, "..", "%s_%s_cell_density_info.csv" % (parts[-3], parts[-2]))
    return density_csv, os.path.join(cur_folder, parts[-1] + "_cell_pos.csv")


def _um2(area_px):
    """pixels^2 -> micrometres^2 with the reference's conversion factor (PX_TO_UM_CONV, tiff_analysis.py:82)."""
    return area_px / (PX_TO_UM_CONV ** 2)


def _write_rows(csv_output_file, header, rows):
    # csv.writer's default dialect on a file opened without newline="" -- the reference's output has \r\n line ends
    with open(csv_output_file, "w") as f:
        out = csv.writer(f)
        out.writerow(header)
        out.writerows(rows)


def write_cell_position_info(cell_positions, cell_clusters, csv_output_file, particle_area):
    """``<folder>_cell_pos.csv`` (tiff_analysis.py:1047-1063): one row per single cell (area rounded to 5 decimals,
    count 1) then one per cluster (area left unrounded, count = cluster.cells); x = column, y = row, 2 decimals."""
    particle_um2 = _um2(particle_area)

    def rows():
        for kind, table in (("cell", cell_positions), ("cluster", cell_clusters)):
            for strain_type, regions in table.items():
                for region in regions:
                    row_pos, col_pos = region.centroid
                    area = _um2(region.area)
                    shown_area = round(area, 5) if kind == "cell" else area
                    count = 1 if kind == "cell" else region.cells
                    yield [strain_type, kind, round(col_pos, 2), round(row_pos, 2), shown_area,
                           round(area / particle_um2, 8), count]

    _write_rows(csv_output_file, ["strain", "cell_type", "x_pos", "y_pos", "cell_area", "cell_area_ratio", "cell_count"],
                rows())


def write_merged_cell_position_info(merged_clusters, csv_output_file, particle_area):
    """``<folder>_merged_cell_pos.csv`` (tiff_analysis.py:1065-1075): one row per merged group."""
    particle_um2 = _um2(particle_area)

    def rows():
        for strain_type, groups in merged_clusters.items():
            for group in groups:
                row_pos, col_pos = group["centroid"]
                area = _um2(group["area"])
                yield [strain_type, round(col_pos, 2), round(row_pos, 2), round(area, 5), round(area / particle_um2, 8),
                       len(group["regions"])]

    _write_rows(csv_output_file, ["strain_type", "x_pos", "y_pos", "cell_area", "cell_area_ratio", "cell_num"], rows())


def write_density_info(csv_output_file, h5_folder, cell_density, cell_area_ratio, cell_count):
    """Per-parent-folder density summary (tiff_analysis.py:1078-1107): rows of ``h5_folder`` already in the file are
    dropped (the file is rewritten without them), then this run's rows are appended -- reruns stay idempotent."""
    header = ["folder", "strain", "cell_density", "cell_area_ratio", "cell_count"]
    is_new = not os.path.exists(csv_output_file)
    if not is_new:
        with open(csv_output_file, "r") as f:
            old_rows = list(csv.reader(f))[1:]
        kept = [row for row in old_rows if row[0] != h5_folder]
        if len(kept) != len(old_rows):
            _write_rows(csv_output_file, header, kept)
    with open(csv_output_file, "a") as f:
        out = csv.writer(f)
        if is_new:
            out.writerow(header)
        out.writerows([h5_folder, strain, cell_density[strain], cell_area_ratio[strain], cell_count[strain]]
                      for strain in cell_density)


def read_class_map(path):
    """The reference reads the first dataset of an ilastik .h5 (tiff_analysis.py:118-121, 639-642).
    h5py is optional here; ``.npy`` files are always accepted."""
    if path.endswith(".npy"):
        return np.load(path, allow_pickle=False)
    try:
        import h5py
    except ImportError as e:  # pragma: no cover
        raise ImportError("reading .h5 class maps needs h5py; save the class map as .npy instead") from e
    with h5py.File(path, "r") as f:
        return f[next(iter(f.keys()))][()]


def process_single_h5_file(cur_folder, file_path):
    """tiff_analysis.py:627-671 without the matplotlib figures: position CSV, merged-position CSV, density row."""
    cell_types = get_cell_type_map(file_path)
    if not cell_types:
        raise ValueError("Cell type not found in file path")
    density_csv, cell_pos_csv = get_pos_and_density_file_names(cur_folder)
    denoised = median_filter(normalize_ds_arr(read_class_map(os.path.join(cur_folder, file_path))), size=DENOISE_SIZE)
    positions, clusters, particle_area, merged = get_cell_positions_and_areas(denoised, cell_types, merged=True)
    counts, densities, ratios = get_cell_counts_and_densities(positions, clusters, particle_area)  # BEFORE the particle fill (:652)
    _, particle_area = recreate_particle_area(denoised, cell_types, particle_area)
    write_cell_position_info(positions, clusters, cell_pos_csv, particle_area)
    write_merged_cell_position_info(merged, cell_pos_csv.replace("_cell_pos.csv", "_merged_cell_pos.csv"), particle_area)
    write_density_info(density_csv, cur_folder.split("/")[-1], densities, ratios, counts)


def _analyse_channel_file(cur_folder, file, cell_strains):
    """One channel file of a multi-channel sample (loop body of tiff_analysis.py:107-157, no figures)."""
    channel = get_channel_from_file(file)
    cell_types = get_cell_type_map_from_channel(cell_strains, channel)
    denoised = median_filter(normalize_ds_arr(read_class_map(os.path.join(cur_folder, file))), size=DENOISE_SIZE)
    positions, clusters, particle_area, _ = get_cell_positions_and_areas(denoised, cell_types)
    return channel, cell_types, denoised, positions, clusters, particle_area


def process_multiple_h5_files(cur_folder, h5_files):
    """A sample exported as one class map per fluorescence channel (tiff_analysis.py:92-222), without the figures.

    Per file: denoise + region table; the RFP file also yields the (recreated) particle area every density refers to.
    Then the raw position CSV, DAPI cells that overlap the other channel by more than 10 % removed (:167-170), densities,
    the channels recombined into one 5-class map (:198-204) whose merged clusters go to ``*_merged_cell_pos.csv``.
    Returns (combined class map, merged clusters)."""
    density_csv, cell_pos_csv = get_pos_and_density_file_names(cur_folder)
    raw_csv = cell_pos_csv.replace("_cell_pos.csv", "_cell_pos_raw.csv")
    combined_csv = cell_pos_csv.replace("_cell_pos.csv", "_cell_pos_combined.csv")
    merged_csv = combined_csv.replace("_cell_pos_combined.csv", "_merged_cell_pos.csv")
    sample_name = cur_folder.split("/")[-1]
    cell_strains = get_strains_from_file(cur_folder)

    all_positions, all_clusters, denoised_by_channel = {}, {}, {}
    rfp_particle_area, dapi_cell_types = None, None
    for file in h5_files:
        channel, cell_types, denoised, positions, clusters, particle_area = _analyse_channel_file(cur_folder, file, cell_strains)
        denoised_by_channel[channel] = denoised
        first_type = cell_types[1]
        if channel == "RFP":
            _, rfp_particle_area = recreate_particle_area(denoised, cell_types, particle_area)
            if first_type == "Particle":  # an RFP channel that only shows the particle carries no cells (:131-132)
                continue
        elif channel == "DAPI":
            dapi_cell_types = cell_types
        if first_type not in CELL_TYPES:
            raise ValueError(f"Strain type not in cell types. {first_type}")
        all_positions.update(positions)
        all_clusters.update(clusters)
    if rfp_particle_area is None:
        raise ValueError("RFP particle area not found")
    write_cell_position_info(all_positions, all_clusters, raw_csv, rfp_particle_area)

    if len(cell_strains) > 1:
        other = "GFP" if cell_strains == ["6B07", "C3M10"] else "RFP"
        dapi_clean = combine_cell_positions_and_clusters(denoised_by_channel["DAPI"], denoised_by_channel[other])
        dapi_positions, dapi_clusters, _, _ = get_cell_positions_and_areas(dapi_clean, dapi_cell_types)
        all_positions["6B07"] = dapi_positions["6B07"]
        all_clusters["6B07"] = dapi_clusters["6B07"]

    counts, densities, area_ratios = get_cell_counts_and_densities(all_positions, all_clusters, rfp_particle_area)
    write_density_info(density_csv, sample_name, densities, area_ratios, counts)

    base = get_rfp_base_arr(denoised_by_channel["RFP"].copy(), cell_strains)
    combined_channels = combine_channels(base, denoised_by_channel, cell_strains)
    _, _, _, merged_clusters = get_cell_positions_and_areas(combined_channels, BASE_TYPE_MAP, merged=True)
    write_cell_position_info(all_positions, all_clusters, combined_csv, rfp_particle_area)
    write_merged_cell_position_info(merged_clusters, merged_csv, rfp_particle_area)
    return combined_channels, merged_clusters


def process_h5_folder(cur_folder, h5_files):
    """tiff_analysis.py:85-89."""
    if len(h5_files) == 1:
        process_single_h5_file(cur_folder, h5_files[0])
    else:
        process_multiple_h5_files(cur_folder, h5_files)


def get_h5_files_recursively(folder_path, suffixes=(".h5", ".npy")):
    """tiff_analysis.py:1113-1123 (also picks up .npy class maps)."""
    h5_files = {}
    for root, _, files in os.walk(folder_path):
        for file in files:
            if file.endswith(tuple(suffixes)):
                h5_files.setdefault(root, []).append(file)
    return h5_files
