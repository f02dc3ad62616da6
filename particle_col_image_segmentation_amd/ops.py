"""Batched device operators: torch tensors in, torch tensors out, HIP inside.

Every function takes ``(B, H, W)`` (or ``(B, C, H, W)``) CUDA tensors, allocates
its outputs and workspace through torch's caching allocator and enqueues the
libpcseg kernels on torch's current stream.  PyTorch is plumbing here (device
memory + streams); all arithmetic is in ``csrc/*.hip``.

The library takes bare pointers, so the wrappers are where an argument's device, dtype, rank and size are checked, against
each other too, before anything is enqueued: what is refused, what is copied and what is read in place is stated once, in
DESIGN.md ("The argument contract of ops"), and held by tests/ops_contract_cases.py.
"""
import collections
import ctypes
import functools

import numpy as np
import torch

from . import _lib


def _stream():  # (for scripts that call the library themselves: _call takes the stream on its own)
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _on_device(t):
    """The one test of "a tensor the library can be handed": a torch tensor in device memory (the HIP path has no CPU
    fallback).  Every wrapper's first check goes through here (tests/test_ops_contract_cpu.py replaces it to run the argument
    checks on a machine without a GPU)."""
    return isinstance(t, torch.Tensor) and t.is_cuda


_NOT_ON_DEVICE = "expected a CUDA tensor (the HIP path has no CPU fallback)"


def _req(t, dtype, ndim):
    """An input: on the device, of ``dtype`` (bool is read as uint8) and ``ndim`` dimensions; a non-contiguous one is copied."""
    if not _on_device(t):
        raise TypeError(_NOT_ON_DEVICE)
    if t.dtype == torch.bool and dtype == torch.uint8:
        t = t.view(torch.uint8)
    if t.dtype != dtype:
        raise TypeError("expected dtype %s, got %s" % (dtype, t.dtype))
    if t.dim() != ndim:
        raise ValueError("expected %d dims, got shape %s" % (ndim, tuple(t.shape)))
    return t.contiguous()


def _label_batch(labels, what="labels"):
    """An int32 (B, H, W) CUDA tensor of any width and alignment (a contiguous view keeps its base address)."""
    if not _on_device(labels):
        raise TypeError(_NOT_ON_DEVICE)
    if labels.dtype != torch.int32 or labels.dim() != 3:
        raise TypeError("%s must be an int32 (B, H, W) tensor" % what)
    return labels if labels.is_contiguous() else labels.contiguous()


def _inout(t, dtype, shape, what):
    """An argument the library writes in place: it is never copied (the result would be lost in the copy) and never written
    through strides the library does not know, so it must be on the device, of ``dtype`` and ``shape`` (-1: any size) -- and
    contiguous."""
    if not _on_device(t):
        raise TypeError(_NOT_ON_DEVICE)
    if t.dtype != dtype:
        raise TypeError("%s: expected dtype %s, got %s" % (what, dtype, t.dtype))
    if t.dim() != len(shape) or any(v != w and w >= 0 for v, w in zip(t.shape, shape)):
        raise ValueError("%s of shape %s, expected %s" % (what, tuple(t.shape), shape))
    if not t.is_contiguous():
        raise ValueError("%s is written in place: it must be contiguous (strides %s)" % (what, t.stride()))
    return t


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


_HOST_ONLY = ("surface_thresholds", "border_block")  # the entries called through _call that take no stream


@functools.lru_cache(maxsize=None)
def _entry(entry):
    """``pcseg_<entry>`` and whether a stream ends its arguments (looked up once per name: _call is on the launch path)."""
    return getattr(_lib.load(), "pcseg_" + entry), entry not in _HOST_ONLY


def _workspace(entry, device, *query):
    """``(workspace, nbytes)`` for ``pcseg_<entry>``: ``nbytes`` is the answer of the size query that ``_lib.WORKSPACE`` names
    for it, given ``query``.  :func:`_call` makes it; a wrapper does only where it allocates outputs after its workspace."""
    nbytes = getattr(_lib.load(), "pcseg_%s_workspace_bytes" % _lib.WORKSPACE["pcseg_" + entry])(*query)
    return _ws(nbytes, device), nbytes


def _call(entry, *args, ws=None):
    """``pcseg_<entry>(*args[, workspace, nbytes][, stream])``, the one way this module enters the library.  A tensor goes as
    its address -- it is what ``_req`` / ``_label_batch`` / ``_plane_view`` returned: nothing is checked here --, None as a
    null pointer, a numpy array as its data address; ctypes objects and numbers are left to the entry's ``argtypes``.
    ``ws``: the arguments of the entry's size query (a workspace of that size is allocated on the device of the first tensor
    argument) or the pair an earlier call returned; None: the entry has no workspace, or it stands among ``args``.  The
    current stream is appended, read now.  A non-zero status raises ``PcsegError``.  Returns the workspace pair, or None.
    Nothing but :func:`_entry`'s lookup is kept from one call to the next (eight host threads launch through here), and a
    call costs the host what the spelled-out form did (profiles/ops_call): hence the int test first -- most arguments are
    sizes."""
    fn, has_stream = _entry(entry)
    argv, first = [], None
    for a in args:
        if type(a) is not int and a is not None:
            if isinstance(a, torch.Tensor):
                first = a if first is None else first
                a = a.data_ptr()
            elif isinstance(a, np.ndarray):
                if not a.flags.c_contiguous:
                    raise ValueError("%s: a numpy argument must be C-contiguous" % entry)
                a = a.ctypes.data
        argv.append(a)
    if ws is not None:
        if not isinstance(ws[0], torch.Tensor):
            ws = _workspace(entry, first.device, *ws)
        argv += (ws[0].data_ptr(), ws[1])
    if has_stream:
        argv.append(torch.cuda.current_stream().cuda_stream)
    rc = fn(*argv)
    if rc:
        _lib.check(rc, entry)
    return ws


def _default_cap(x):
    """The cap of a table over the labels (or counts) ``x`` when the caller names none: the largest, read back; at least 1."""
    return max(int(x.max().item()), 1)


def argmax_planes(stack):
    """class map = argmax over planes + 1 (tiff_analysis.py:639-642 reads this from ilastik)."""
    stack = _req(stack, torch.float32, 4)
    B, C, H, W = stack.shape
    out = torch.empty((B, H, W), dtype=torch.uint8, device=stack.device)
    _call("argmax_planes_f32", stack, out, B, C, H, W)
    return out


def median5(x):
    """scipy.ndimage.median_filter(x, size=5) (tiff_analysis.py:122, 643)."""
    x = _req(x, torch.uint8, 3)
    B, H, W = x.shape
    out = torch.empty_like(x)
    _call("median5_u8", x, out, B, H, W)
    return out


def classmap_label(stack):
    """class map (argmax + 1) -> median_filter(size=5) -> label (tiff_analysis.py:639-643, 743) as one fused front end:
    returns (denoised uint8 (B,H,W), labels int32 (B,H,W), counts int32 (B,))."""
    stack = _req(stack, torch.float32, 4)
    B, C, H, W = stack.shape
    dev = stack.device
    z = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    labels = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    _call("classmap_label_f32", stack, C, z, labels, counts, B, H, W, ws=(B, H, W))
    return z, labels, counts


def _ccl(entry, x):
    x = _req(x, torch.uint8, 3)
    B, H, W = x.shape
    labels = torch.empty((B, H, W), dtype=torch.int32, device=x.device)
    counts = torch.empty((B,), dtype=torch.int32, device=x.device)
    _call(entry, x, labels, counts, B, H, W, ws=(B, H, W))
    return labels, counts


def label_equal8(x):
    """skimage.measure.label(int image): equal-valued 8-connected components (tiff_analysis.py:743)."""
    return _ccl("ccl8_equal_u8", x)


def label_bool8(x):
    """skimage.measure.label(bool image) (tiff_analysis.py:260, 829; refine_boundaries.py:64)."""
    return _ccl("ccl8_bool", x)


def label_bool4(x):
    """scipy.ndimage.label(bool image), 4-connectivity."""
    return _ccl("ccl4_bool", x)


def compact_labels(roots):
    roots = _req(roots, torch.int32, 3)
    B, H, W = roots.shape
    labels = torch.empty_like(roots)
    counts = torch.empty((B,), dtype=torch.int32, device=roots.device)
    _call("compact_labels", roots, labels, counts, B, H, W, ws=(B, H, W))
    return labels, counts


def region_init(counts, cap, C, shape, device):
    """Initialised (not yet filled) region tables of a (B, H, W) label batch: stats int64 (B, cap, 8) with the
    reduction's neutral rows, sums float64 (B, cap, C) zeroed (rows below counts[b]), overflow int32 (B,) cleared."""
    B, H, W = shape
    counts = _req(counts, torch.int32, 1)
    if counts.shape[0] != B:
        raise ValueError("counts must have one entry per frame")
    stats = torch.empty((B, cap, 8), dtype=torch.int64, device=device)
    sums = torch.empty((B, cap, C), dtype=torch.float64, device=device)
    overflow = torch.empty((B,), dtype=torch.int32, device=device)
    _call("region_init", counts, cap, C, B, H, W, stats, sums, overflow)
    return stats, sums, overflow


def region_sums2(labels_a, cls, sum_classes, sums_a, labels_b, sums_b, planes, stats_b=None, overflow_b=None):
    """Per-label plane sums of two label images in ONE pass over the planes (csrc/reduce.hip region_sums2_col_kernel):
    ``sums_a`` / ``sums_b`` (float64 (B, cap, C), zeroed by ``region_reduce(..., zero_sums=C)`` or ``region_init``) are
    added to in place; image A only under the class values in ``sum_classes`` (bit v = value v, 0 = everywhere).
    ``stats_b`` / ``overflow_b`` (from ``region_init``): image B's integer columns are accumulated too, by the plane-free pass.
    The four tables are written in place: each must be contiguous (a copy would take the sums with it)."""
    labels_a = _req(labels_a, torch.int32, 3)
    labels_b = _req(labels_b, torch.int32, 3)
    planes = _req(planes, torch.float32, 4)
    B, C, H, W = planes.shape
    if tuple(labels_a.shape) != (B, H, W) or labels_b.shape != labels_a.shape:
        raise ValueError("the label images do not match the planes")
    if cls is not None:
        cls = _req(cls, torch.uint8, 3)
        if cls.shape != labels_a.shape:
            raise ValueError("cls must have the labels' shape")
    _inout(sums_a, torch.float64, (B, -1, C), "sums_a")
    _inout(sums_b, torch.float64, (B, -1, C), "sums_b")
    if stats_b is not None:
        _inout(stats_b, torch.int64, (B, sums_b.shape[1], 8), "stats_b")
    if overflow_b is not None:
        _inout(overflow_b, torch.int32, (B,), "overflow_b")
    _call("region_sums2", labels_a, cls, int(sum_classes), sums_a.shape[1], sums_a, labels_b, sums_b.shape[1], sums_b, stats_b,
          overflow_b, planes, C, B, H, W)


def region_reduce(labels, counts=None, cls=None, planes=None, cap=None, sum_classes=0, zero_sums=0):
    """regionprops sums + optional class at first pixel + optional per-label plane sums.  ``sum_classes`` (bit v = class
    value v; 0 = all): plane sums only over pixels of those classes -- the other regions keep 0 and cost no plane reads.
    ``zero_sums`` = C (without ``planes``): also return a (B, cap, C) sums table with the rows below ``counts`` zeroed, for
    :func:`region_sums2`.

    Returns (stats int64 (B,cap,8), cls_out uint8 (B,cap) | None, sums float64 (B,cap,C) | None,
    overflow int32 (B,))."""
    labels = _req(labels, torch.int32, 3)
    shape = labels.shape  # (read once: every .shape makes a torch.Size, and this is the launch path)
    B, H, W = shape
    dev = labels.device
    if cap is None:
        if counts is None:
            raise ValueError("cap or counts is required")
        cap = _default_cap(counts)
    # no zero fill: the library initialises the rows it fills (all of them, or the first counts[b] of frame b); rows
    # beyond counts[b] are never read by anything that takes `counts`
    stats = torch.empty((B, cap, 8), dtype=torch.int64, device=dev)
    cls_out = None
    sums = None
    C = 0
    if cls is not None:
        cls = _req(cls, torch.uint8, 3)
        if cls.shape != shape:
            raise ValueError("cls must have the labels' shape")
        cls_out = torch.empty((B, cap), dtype=torch.uint8, device=dev)
    if planes is not None:
        planes = _req(planes, torch.float32, 4)
        pb, C, ph, pw = planes.shape
        if pb != B or ph != H or pw != W:
            raise ValueError("planes must be (B, C, H, W) over the labels' (B, H, W)")
        sums = torch.empty((B, cap, C), dtype=torch.float64, device=dev)
    elif zero_sums:
        C = int(zero_sums)
        sums = torch.empty((B, cap, C), dtype=torch.float64, device=dev)
    if counts is not None:
        counts = _req(counts, torch.int32, 1)
        if counts.shape[0] != B:
            raise ValueError("counts must have one entry per frame")
    overflow = torch.empty((B,), dtype=torch.int32, device=dev)
    if sum_classes and (cls is None or planes is None):
        raise ValueError("sum_classes needs cls and planes")
    _call("region_reduce_sel", labels, counts, cls, int(sum_classes), planes, C, B, H, W, cap, stats, cls_out, sums, overflow)
    return stats, cls_out, sums, overflow


SHAPE_COLUMNS = ("a", "b", "c", "l1", "l2", "major", "minor", "eccentricity", "orientation", "equivalent_diameter", "extent",
                 "perimeter")


def region_shape(labels, counts, cap=None):
    """The integer shape table of a label batch (csrc/shape.hip, include/pcseg.h): ``labels`` (B, H, W) int32 CUDA tensor
    of any width and alignment, ``counts`` (B,) int32.  Returns ``(shape, overflow)``: int64 (B, cap, 8) = sum r^2, sum
    r c, sum c^2, n_1, n_sqrt2, n_mid, n_border, 0 for the labels 1 .. min(counts[b], cap) (rows beyond are not
    initialised) and int32 (B,) set where a label exceeds ``cap`` (default: max(counts))."""
    labels = _label_batch(labels)
    counts = _req(counts, torch.int32, 1)
    B, H, W = labels.shape
    if counts.shape[0] != B:
        raise ValueError("counts must have one entry per frame")
    if cap is None:
        cap = _default_cap(counts)
    cap = int(cap)
    dev = labels.device
    shape = torch.empty((B, cap, 8), dtype=torch.int64, device=dev)
    overflow = torch.empty((B,), dtype=torch.int32, device=dev)
    _call("region_shape", labels, counts, shape, overflow, B, H, W, cap, ws=(B, H, W))
    return shape, overflow


def _properties(entry, stats, table, width, counts, columns, mismatch):
    """pcseg_<entry>: float64 (B, cap, columns) derived from ``stats`` (B, cap, 8) and the integer ``table`` (B, cap, width)."""
    stats = _req(stats, torch.int64, 3)
    table = _req(table, torch.int64, 3)
    counts = _req(counts, torch.int32, 1)
    B, cap = stats.shape[0], stats.shape[1]
    if tuple(stats.shape) != (B, cap, 8) or tuple(table.shape) != (B, cap, width) or counts.shape[0] != B:
        raise ValueError(mismatch)
    out = torch.empty((B, cap, columns), dtype=torch.float64, device=stats.device)
    _call(entry, stats, table, counts, out, B, cap)
    return out


def shape_properties(stats, shape, counts):
    """The derived shape columns (scikit-image 0.18.3 conventions, pixels): ``stats`` int64 (B, cap, 8) of
    :func:`region_reduce` and ``shape`` of :func:`region_shape` over the same labels -> float64 (B, cap, 12) in the order of
    ``SHAPE_COLUMNS``, rows below min(counts[b], cap); NaN for a label without pixel."""
    return _properties("shape_properties", stats, shape, 8, counts, len(SHAPE_COLUMNS),
                       "stats and shape must both be (B, cap, 8), counts (B,)")


HULL_COLUMNS = ("convex_area", "solidity", "feret_diameter_max", "euler_number")


def region_hull(labels, counts, stats, cap=None):
    """The integer convexity table of a label batch (csrc/hull.hip, include/pcseg.h): ``labels`` (B, H, W) int32 CUDA
    tensor of any width and alignment, ``counts`` (B,) int32, ``stats`` int64 (B, cap, 8) of :func:`region_reduce` over the
    same labels (a ROI is looked for inside the bounding box its row names).  Returns ``(hull, overflow)``: int64 (B, cap,
    4) = convex_area, feret_sq4, euler number, 0 for the labels 1 .. min(counts[b], cap) (rows beyond are not initialised)
    and int32 (B,) set where ``counts[b]`` exceeds ``cap`` (default: the height of ``stats``)."""
    labels = _label_batch(labels)
    counts = _req(counts, torch.int32, 1)
    stats = _req(stats, torch.int64, 3)
    B, H, W = labels.shape
    if counts.shape[0] != B:
        raise ValueError("counts must have one entry per frame")
    if cap is None:
        cap = stats.shape[1]
    cap = int(cap)
    if tuple(stats.shape) != (B, cap, 8):
        raise ValueError("stats must be (B, cap, 8)")
    dev = labels.device
    hull = torch.empty((B, cap, 4), dtype=torch.int64, device=dev)
    overflow = torch.empty((B,), dtype=torch.int32, device=dev)
    _call("region_hull", labels, counts, stats, hull, overflow, B, H, W, cap, ws=(B, H, W, cap))
    return hull, overflow


def hull_properties(stats, hull, counts):
    """The derived convexity columns (scikit-image 0.18.3 conventions, pixels): ``stats`` int64 (B, cap, 8) of
    :func:`region_reduce` and ``hull`` of :func:`region_hull` over the same labels -> float64 (B, cap, 4) in the order of
    ``HULL_COLUMNS``, rows below min(counts[b], cap); NaN for a label without pixel."""
    return _properties("hull_properties", stats, hull, 4, counts, len(HULL_COLUMNS),
                       "stats must be (B, cap, 8), hull (B, cap, 4), counts (B,)")


SKELETON_COLUMNS = ("skel_px", "n_orth", "n_diag", "n_end", "n_junction", "passes", "length_px", "width_px")
PEEL_SKELETON = 65535                # the peel value of a pixel that survives
THIN_TILE, THIN_HALO = (64, 32), 8   # csrc/skeleton.hip: a tile (width, height) and its halo = sub-iterations per launch


def thin_labels(labels, max_iter=None):
    """Exact Guo-Hall thinning of a label batch, every label on its own (csrc/skeleton.hip, include/pcseg.h): the union over
    l of ``skimage.morphology.thin(labels == l, max_iter)`` of scikit-image 0.18.3.  ``labels`` (B, H, W) int32 CUDA tensor
    of any width and alignment; values <= 0 are background, labels may touch and need not be consecutive.  Returns ``(peel,
    iters)``: uint16 (B, H, W) -- 0 background, 65535 the pixel survives (the skeleton), otherwise the 1-based sub-iteration
    that deleted it (full iteration ``(s + 1) // 2``) -- and int32 (B,), the full iterations of a frame that deleted a
    pixel.  Waits for the device between launches (the host decides whether another one follows): not for graph capture."""
    labels = _label_batch(labels)
    B, H, W = labels.shape
    dev = labels.device
    peel = torch.empty((B, H, W), dtype=torch.uint16, device=dev)
    iters = torch.empty((B,), dtype=torch.int32, device=dev)
    _call("thin_labels", labels, peel, iters, B, H, W, -1 if max_iter is None else int(max_iter), ws=(B, H, W))
    return peel, iters


def thin(image, max_iter=None):
    """``skimage.morphology.thin``: ``image`` a (B, H, W) CUDA tensor, bool / uint8 (a mask: non-zero is foreground) or int32
    (labels, each thinned on its own) -> the bool skeleton."""
    if isinstance(image, torch.Tensor) and image.dtype in (torch.bool, torch.uint8):
        image = (image != 0).to(torch.int32)
    peel, _ = thin_labels(image, max_iter)
    # (torch has no comparison kernel for uint16: its bit pattern as int16 -- 65535 is -1)
    return peel.view(torch.int16) == -1


def region_skeleton(labels, peel, counts, cap=None):
    """The integer skeleton table of a label batch: ``labels`` (B, H, W) int32, ``peel`` of :func:`thin_labels` over the same
    labels, ``counts`` (B,) int32.  Returns int64 (B, cap, 6) = skel_px, n_orth, n_diag, n_end, n_junction, passes for the
    labels 1 .. min(counts[b], cap) (rows beyond are not initialised; labels above are ignored; ``cap`` defaults to
    max(counts)): the skeleton's pixels, its orthogonal and diagonal links between pixels of the same label (a diagonal pair
    is a link only if neither pixel next to both is on the label's skeleton), the pixels with one link and with three or
    more, and the full iterations the label took."""
    labels = _label_batch(labels)
    counts = _req(counts, torch.int32, 1)
    B, H, W = labels.shape
    if not _on_device(peel) or peel.dtype != torch.uint16 or peel.dim() != 3:
        raise TypeError("peel must be a uint16 (B, H, W) CUDA tensor")
    if peel.shape != labels.shape:
        raise ValueError("peel must have the labels' shape")
    peel = peel.contiguous()
    if counts.shape[0] != B:
        raise ValueError("counts must have one entry per frame")
    if cap is None:
        cap = _default_cap(counts)
    cap = int(cap)
    table = torch.empty((B, cap, 6), dtype=torch.int64, device=labels.device)
    _call("region_skeleton", labels, peel, counts, table, B, H, W, cap, ws=(B, H, W, cap))
    return table


def skeleton_properties(stats, table, counts):
    """The derived skeleton columns, in pixels: ``stats`` int64 (B, cap, 8) of :func:`region_reduce` and ``table`` of
    :func:`region_skeleton` over the same labels -> float64 (B, cap, 2) = length_px (n_orth + n_diag * sqrt 2), width_px
    (area / length_px; inf for a one-pixel skeleton), rows below min(counts[b], cap); NaN for a label without pixel."""
    return _properties("skeleton_properties", stats, table, 6, counts, 2, "stats must be (B, cap, 8), table (B, cap, 6), counts (B,)")


def threshold_lt(img, threshold):
    """binary_mask = boundary_map < threshold (refine_boundaries.py:44-45)."""
    img = _req(img, torch.float32, 3)
    B, H, W = img.shape
    out = torch.empty((B, H, W), dtype=torch.uint8, device=img.device)
    _call("threshold_lt_f32", img, float(threshold), out, B, H, W)
    return out


def edt_sq(mask, cap=-1):
    """exact squared EDT of a 0/1 mask (refine_boundaries.py:60, tiff_analysis.py:996)."""
    mask = _req(mask, torch.uint8, 3)
    B, H, W = mask.shape
    d2 = torch.empty((B, H, W), dtype=torch.int32, device=mask.device)
    _call("edt_sq_u8", mask, d2, B, H, W, int(cap), ws=(B, H, W))
    return d2


def _plane_view(img):
    """(B,H,W) float32 view whose frames may be strided (a plane of a (B,C,H,W) stack): (tensor, frame stride)."""
    if not _on_device(img) or img.dtype != torch.float32 or img.dim() != 3:
        raise TypeError("expected a (B,H,W) float32 CUDA tensor")
    B, H, W = img.shape
    if img.stride(2) == 1 and img.stride(1) == W and (B == 1 or img.stride(0) >= H * W):
        return img, (img.stride(0) if B > 1 else H * W)
    return img.contiguous(), H * W


def edt_sq_lt(img, threshold, want_mask=True):
    """fused threshold + squared EDT (refine_boundaries.py:44-45, 60); img may be a plane view of a stack."""
    img, fstride = _plane_view(img)
    B, H, W = img.shape
    d2 = torch.empty((B, H, W), dtype=torch.int32, device=img.device)
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=img.device) if want_mask else None
    _call("edt_sq_lt_f32", img, fstride, float(threshold), d2, mask, B, H, W, ws=(B, H, W))
    return d2, mask


def dilate_disk(x, value_bits, radius):
    """binary_dilation(((value_bits >> x) & 1), disk(radius)) (tiff_analysis.py:827-828, 990)."""
    x = _req(x, torch.uint8, 3)
    B, H, W = x.shape
    out = torch.empty_like(x)
    _call("dilate_disk_u8", x, int(value_bits), int(radius), out, B, H, W, ws=(B, H, W))
    return out


def fill_particle(ds, particle_label, cell_label, overlap_label, dilation_radius, dist_threshold, overlap_area=None):
    """fill_particle_area (tiff_analysis.py:982-1015); overlap_area int64 (B,) is accumulated in place."""
    ds = _req(ds, torch.uint8, 3)
    B, H, W = ds.shape
    out = torch.empty_like(ds)
    if overlap_area is None:
        overlap_area = torch.zeros((B,), dtype=torch.int64, device=ds.device)
    else:
        _inout(overlap_area, torch.int64, (B,), "overlap_area")
    _call("fill_particle", ds, out, int(particle_label), int(cell_label), int(overlap_label), int(dilation_radius),
          int(dist_threshold), overlap_area, B, H, W, ws=(B, H, W))
    return out, overlap_area


def fill_holes(mask):
    """scipy.ndimage.binary_fill_holes (tiff_analysis.py:880)."""
    mask = _req(mask, torch.uint8, 3)
    B, H, W = mask.shape
    out = torch.empty_like(mask)
    _call("fill_holes", mask, out, B, H, W, ws=(B, H, W))
    return out


def local_maxima(img, want_mask=True, want_markers=True):
    """skimage.morphology.local_maxima + measure.label on an int32 image (refine_boundaries.py:63-64): (is_max, markers,
    counts); the counts come out of the numbering of the markers, so without markers there are none (None)."""
    img = _req(img, torch.int32, 3)
    B, H, W = img.shape
    is_max = torch.empty((B, H, W), dtype=torch.uint8, device=img.device) if want_mask else None
    markers = torch.empty((B, H, W), dtype=torch.int32, device=img.device) if want_markers else None
    counts = torch.empty((B,), dtype=torch.int32, device=img.device) if want_markers else None
    _call("local_maxima_i32", img, is_max, markers, counts, B, H, W, ws=(B, H, W))
    return is_max, markers, counts


RECONSTRUCT_TILE = (64, 32)          # csrc/reconstruct.hip: a tile (width, height)
RECONSTRUCT_GRID_ROUNDS = 6          # ... and the rounds it enqueues as grids before the per-frame tail kernel
RECONSTRUCT_SEED_BEYOND_MASK, RECONSTRUCT_NOT_CONVERGED = 1, 2  # bits of the per-frame flags (include/pcseg.h)
_RECONSTRUCT_METHODS = {"dilation": 0, "erosion": 1}
_SEED_MESSAGES = {"dilation": "Intensity of seed image must be less than that of the mask image for reconstruction by dilation.",
                  "erosion": "Intensity of seed image must be greater than that of the mask image for reconstruction by erosion."}


def _gray_pair(seed, mask):
    """two (B, H, W) CUDA tensors of one dtype, int32 or float64 (float32 is widened, which is exact)"""
    for t in (seed, mask):
        if not _on_device(t):
            raise TypeError(_NOT_ON_DEVICE)
        if t.dtype not in (torch.int32, torch.float32, torch.float64):
            raise TypeError("expected an int32, float32 or float64 image, got %s" % t.dtype)
        if t.dim() != 3:
            raise ValueError("expected 3 dims, got shape %s" % (tuple(t.shape),))
    if seed.shape != mask.shape:
        raise ValueError("seed and mask must have the same shape")
    if (seed.dtype == torch.int32) != (mask.dtype == torch.int32):
        raise TypeError("seed and mask must both be int32 or both be floating point")
    if seed.dtype != torch.int32:
        seed, mask = seed.to(torch.float64), mask.to(torch.float64)
    return seed.contiguous(), mask.contiguous()


def _reconstruct(seed, mask, method, conn, max_rounds=0):
    """(out, flags, workspace) of pcseg_reconstruct_*: enqueued, nothing is read back"""
    if method not in _RECONSTRUCT_METHODS:
        raise ValueError("Reconstruction method can be one of 'erosion' or 'dilation'. Got '%s'." % (method,))
    if conn not in (4, 8):
        raise ValueError("conn must be 4 or 8")
    B, H, W = seed.shape
    dev = seed.device
    out = torch.empty_like(seed)
    flags = torch.empty((B,), dtype=torch.int32, device=dev)
    ws, _ = _call("reconstruct_i32" if seed.dtype == torch.int32 else "reconstruct_f64", seed, mask, out, flags, B, H, W, int(conn),
                  _RECONSTRUCT_METHODS[method], int(max_rounds), ws=(B, H, W))
    return out, flags, ws


def _check_reconstruct_flags(flags, method=None):
    f = flags.cpu()
    if method is not None and bool((f & RECONSTRUCT_SEED_BEYOND_MASK).any()):
        raise ValueError(_SEED_MESSAGES[method])
    if bool((f & RECONSTRUCT_NOT_CONVERGED).any()):
        raise RuntimeError("reconstruction did not converge in frame(s) %s: the round cap was reached"
                           % [int(b) for b in torch.nonzero(f & RECONSTRUCT_NOT_CONVERGED)[:, 0]])


def reconstruct(seed, mask, method="dilation", conn=8, check=True, counters=False):
    """``skimage.morphology.reconstruction(seed, mask, method)`` of scikit-image 0.18.3 per frame (csrc/reconstruct.hip), exact:
    ``seed`` and ``mask`` (B, H, W) CUDA tensors, both int32 or both floating point (float32 is widened to float64, which is
    exact), NaN-free; ``conn`` 8 (the default 3 x 3 footprint) or 4.  Returns ``(out, flags)``: the reconstruction in the
    (widened) input type and int32 (B,) flags -- bit ``RECONSTRUCT_SEED_BEYOND_MASK`` where a seed pixel lies above (erosion:
    below) its mask pixel (the seed is clamped to the mask there), bit ``RECONSTRUCT_NOT_CONVERGED`` where the round cap was
    reached and the frame is no result.  ``check=True`` reads the flags and raises scikit-image's ``ValueError`` for the first,
    ``RuntimeError`` for the second; ``check=False`` never waits for the device.  ``counters=True`` also returns the call's
    int32 counters (include/pcseg.h)."""
    seed, mask = _gray_pair(seed, mask)
    out, flags, ws = _reconstruct(seed, mask, method, conn)
    if check:
        _check_reconstruct_flags(flags, method)
    return (out, flags, ws[:128].view(torch.int32)) if counters else (out, flags)


def _h_extrema(image, h, conn, sign):
    if not _on_device(image):
        raise TypeError(_NOT_ON_DEVICE)
    if image.dtype not in (torch.int32, torch.float64) or image.dim() != 3:
        raise TypeError("expected an int32 or float64 (B, H, W) image, got %s %s" % (image.dtype, tuple(image.shape)))
    if not h > 0:
        raise ValueError("h must be positive: h = 0 is ambiguous, use local_maxima() instead?")
    image = image.contiguous()
    B, H, W = image.shape
    dev = image.device
    rng = torch.empty((B, 2), dtype=torch.int64, device=dev)
    seed = torch.empty_like(image)
    mark = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    method = "dilation" if sign < 0 else "erosion"
    if image.dtype == torch.int32:
        if float(h) != int(h):
            raise ValueError("an int32 image needs an integral h (got %r): pass a float64 image instead" % (h,))
        h = int(h)
        if h > 0xFFFFFFFF:
            raise ValueError("The %s constant is not compatible with the image data type." % ("subtracted" if sign < 0 else "added"))
        _call("hmax_range_i32", image, rng, B, H, W)
        _call("hmax_shift_i32", image, h, sign, seed, B, H, W)
        rec, flags, _ = _reconstruct(seed, image, method, conn)
        _call("hmax_mark_i32", image, rec, h, sign, rng, mark, B, H, W)
    else:
        h = float(h)
        _call("hmax_range_f64", image, rng, B, H, W)
        _call("hmax_shift_f64", image, h, sign, seed, B, H, W)
        rec, flags, _ = _reconstruct(seed, image, method, conn)
        _call("hmax_mark_f64", image, rec, h, sign, rng, 0, mark, B, H, W)
    _check_reconstruct_flags(flags)
    return mark


def h_maxima(image, h, conn=8):
    """``skimage.morphology.h_maxima(image, h)`` of scikit-image 0.18.3 per frame: the uint8 mask of the maxima that rise at
    least ``h`` above their surroundings.  ``image`` (B, H, W) int32 or float64 CUDA tensor, NaN-free; an int32 image needs an
    integral ``h``.  A frame whose value range is below ``h`` has no h-maxima (the test is per frame).  ``conn`` 8 or 4."""
    return _h_extrema(image, h, conn, -1)


def h_minima(image, h, conn=8):
    """``skimage.morphology.h_minima(image, h)``: the mirror image of :func:`h_maxima` (reconstruction by erosion of
    ``image + h``)."""
    return _h_extrema(image, h, conn, 1)


def edt_maxima(d2, h, conn=8, want_mask=True, want_markers=True, counters=False):
    """The h-maxima of a distance map as watershed markers -- ``h_maxima(sqrt(d2), h)`` and ``measure.label`` of it -- in the
    place of :func:`local_maxima`: ``d2`` (B, H, W) int32, the squared distance of :func:`edt_sq` / :func:`edt_sq_lt`; ``h`` in
    pixels of the distance map.  Returns ``(is_max, markers, counts, flags)``: the uint8 mask, its 8-connected components
    numbered in raster order of their first pixel, their number per frame, and the reconstruction's per-frame flags (non-zero:
    the frame is no result, see :func:`reconstruct`).  Nothing is read back: the call can be captured into a graph."""
    d2 = _req(d2, torch.int32, 3)
    if not h > 0:
        raise ValueError("h must be positive: h = 0 is ambiguous, use local_maxima() instead?")
    h = float(h)
    B, H, W = d2.shape
    dev = d2.device
    rng = torch.empty((B, 2), dtype=torch.int64, device=dev)
    dist = torch.empty((B, H, W), dtype=torch.float64, device=dev)
    seed = torch.empty_like(dist)
    is_max = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    _call("hmax_range_i32", d2, rng, B, H, W)
    _call("hmax_shift_edt", d2, h, dist, seed, B, H, W)
    rec, flags, ws = _reconstruct(seed, dist, "dilation", conn)
    _call("hmax_mark_f64", dist, rec, h, -1, rng, 1, is_max, B, H, W)
    markers = counts = None
    if want_markers:
        markers, counts = label_bool8(is_max)
    out = (is_max if want_mask else None, markers, counts, flags)
    return out + (ws[:128].view(torch.int32),) if counters else out


# test-only mode bits of pcseg_watershed4_f32 (include/pcseg.h): poison the union-find parent image before one pass
WS_POISON_BORDER, WS_POISON_LABEL, WS_POISON_LEVEL2 = 8, 16, 32


def watershed(img, markers, mask, mode=0):
    """skimage.segmentation.watershed(img, markers, mask=mask) (refine_boundaries.py:73).

    Returns (labels int32, tie_flags int32 (B,)): tie_flags[b] = 1 where the parallel flood could not be
    proven exact (mode 0 re-runs those frames with the exact sequential flood)."""
    img, fstride = _plane_view(img)
    markers = _req(markers, torch.int32, 3)
    mask = _req(mask, torch.uint8, 3)
    shape = img.shape  # (read once: every .shape makes a torch.Size, and this is the launch path)
    if markers.shape != shape or mask.shape != shape:
        raise ValueError("img, markers and mask must have one shape")
    B, H, W = shape
    out = torch.empty((B, H, W), dtype=torch.int32, device=img.device)
    flags = torch.zeros((B,), dtype=torch.int32, device=img.device)
    _call("watershed4_f32", img, fstride, markers, mask, out, flags, B, H, W, int(mode), ws=(B, H, W))
    return out, flags


def dilated_roots(x, value_bits, radius):
    """components of binary_dilation(((value_bits >> x) & 1), disk(radius)) as a union-find parent image (A6)."""
    x = _req(x, torch.uint8, 3)
    B, H, W = x.shape
    roots = torch.empty((B, H, W), dtype=torch.int32, device=x.device)
    _call("dilate_ccl_roots_u8", x, int(value_bits), int(radius), roots, B, H, W, ws=(B, H, W))
    return roots


def dilated_runs(x, value_bits, radius, run_parent=None):
    """components of binary_dilation(((value_bits >> x) & 1), disk(radius)) WITHOUT a label image (A6): the dilated
    mask as 32-row column words int32 (B, ceil(H/32), W) and a union-find over its vertical runs (int32 (B,H,W) scratch
    of which only the run-head entries are written; pass ``run_parent`` to reuse one).  For merge_groups_runs."""
    x = _req(x, torch.uint8, 3)
    B, H, W = x.shape
    bits = torch.empty((B, (H + 31) // 32, W), dtype=torch.int32, device=x.device)
    if run_parent is None:
        run_parent = torch.empty((B, H, W), dtype=torch.int32, device=x.device)
    else:
        _inout(run_parent, torch.int32, (B, H, W), "run_parent")
    _call("dilate_ccl_runs_u8", x, int(value_bits), int(radius), bits, run_parent, B, H, W, ws=(B, H, W))
    return bits, run_parent


def _list_args(B, stats, region_list, n_list):
    """the region table and one region list per frame of a grouping over ``B`` frames"""
    if tuple(stats.shape) != (B, stats.shape[1], 8):
        raise ValueError("stats must be (B, cap, 8)")
    if region_list.shape[0] != B or n_list.shape[0] != B:
        raise ValueError("region_list must be (B, list_cap) and n_list (B,)")


def merge_groups_runs(bits, run_parent, stats, region_list, n_list):
    """get_merged_regions grouping (tiff_analysis.py:843-878) on the run components of dilated_runs()."""
    bits = _req(bits, torch.int32, 3)
    run_parent = _req(run_parent, torch.int32, 3)
    stats = _req(stats, torch.int64, 3)
    region_list = _req(region_list, torch.int32, 2)
    n_list = _req(n_list, torch.int32, 1)
    B, H, W = run_parent.shape
    cap = stats.shape[1]
    list_cap = region_list.shape[1]
    if tuple(bits.shape) != (B, (H + 31) // 32, W):
        raise ValueError("bits must be (B, ceil(H / 32), W) for run_parent's (B, H, W)")
    _list_args(B, stats, region_list, n_list)
    group_of = torch.zeros((B, list_cap), dtype=torch.int32, device=stats.device)
    n_groups = torch.zeros((B,), dtype=torch.int32, device=stats.device)
    _call("merge_groups_runs", bits, run_parent, stats, region_list, n_list, group_of, n_groups, B, H, W, cap, list_cap,
          ws=(B, list_cap))
    return group_of, n_groups


def dilated_runs_multi(x, value_bits_list, radius):
    """dilated_runs for several masks of one class map in one go (the class map is read once; every later pass is ONE launch
    over all masks): returns (bits int32 (M, B, ceil(H/32), W), run_parent int32 (M, B, H, W))."""
    x = _req(x, torch.uint8, 3)
    B, H, W = x.shape
    M = len(value_bits_list)
    bits = torch.empty((M, B, (H + 31) // 32, W), dtype=torch.int32, device=x.device)
    run_parent = torch.empty((M, B, H, W), dtype=torch.int32, device=x.device)
    vb = np.array([int(v) for v in value_bits_list], np.uint64)
    _call("dilate_ccl_runs_multi_u8", x, vb, M, int(radius), bits, run_parent, B, H, W, ws=(B * M, H, W))
    return bits, run_parent


def merge_groups_fused_multi(bits, run_parent, stats, region_lists, n_lists, slots):
    """merge_groups_fused for the M masks of dilated_runs_multi in one launch; mask m is grouped over the list of type slot
    ``slots[m]``.  Returns (group_of (M,B,cap), n_groups (M,B), group_stats (M,B,cap,8))."""
    bits = _req(bits, torch.int32, 4)
    run_parent = _req(run_parent, torch.int32, 4)
    stats = _req(stats, torch.int64, 3)
    region_lists = _req(region_lists, torch.int32, 3)
    n_lists = _req(n_lists, torch.int32, 2)
    M, B, H, W = run_parent.shape
    cap = stats.shape[1]
    n_slots = region_lists.shape[1]
    if (len(slots) != M or tuple(bits.shape) != (M, B, (H + 31) // 32, W) or tuple(stats.shape) != (B, cap, 8)
            or tuple(region_lists.shape) != (B, n_slots, cap) or tuple(n_lists.shape) != (B, n_slots)):
        raise ValueError("masks / lists / region table do not match")
    dev = stats.device
    group_of = torch.empty((M, B, cap), dtype=torch.int32, device=dev)
    n_groups = torch.empty((M, B), dtype=torch.int32, device=dev)
    gstats = torch.empty((M, B, cap, 8), dtype=torch.int64, device=dev)
    sl = np.array([int(v) for v in slots], np.int32)
    _call("merge_groups_fused_multi", bits, run_parent, stats, region_lists, n_lists, sl, M, n_slots, group_of, n_groups, gstats,
          B, H, W, cap, ws=(B * M, cap))
    return group_of, n_groups, gstats


def merge_groups_fused(bits, run_parent, stats, region_lists, n_lists, slot):
    """get_merged_regions grouping + the member sums of the groups (tiff_analysis.py:843-878) for type slot ``slot`` in
    one launch: ``region_lists`` int32 (B, n_slots, cap) / ``n_lists`` int32 (B, n_slots) as classify_regions returns
    them.  Returns (group_of int32 (B,cap), n_groups int32 (B,), group_stats int64 (B,cap,8)); entries beyond a frame's
    list length / group count are not initialised."""
    bits = _req(bits, torch.int32, 3)
    run_parent = _req(run_parent, torch.int32, 3)
    stats = _req(stats, torch.int64, 3)
    region_lists = _req(region_lists, torch.int32, 3)
    n_lists = _req(n_lists, torch.int32, 2)
    B, H, W = run_parent.shape
    cap = stats.shape[1]
    n_slots = region_lists.shape[1]
    if tuple(bits.shape) != (B, (H + 31) // 32, W) or tuple(stats.shape) != (B, cap, 8):
        raise ValueError("bits must be (B, ceil(H / 32), W) for run_parent's (B, H, W), stats (B, cap, 8)")
    if tuple(region_lists.shape) != (B, n_slots, cap) or tuple(n_lists.shape) != (B, n_slots):
        raise ValueError("region lists of shape %s / %s do not match the region table" % (tuple(region_lists.shape), tuple(n_lists.shape)))
    dev = stats.device
    group_of = torch.empty((B, cap), dtype=torch.int32, device=dev)
    n_groups = torch.empty((B,), dtype=torch.int32, device=dev)
    gstats = torch.empty((B, cap, 8), dtype=torch.int64, device=dev)
    _call("merge_groups_fused", bits, run_parent, stats, region_lists, n_lists, int(slot), n_slots, group_of, n_groups, gstats,
          B, H, W, cap, ws=(B, cap))
    return group_of, n_groups, gstats


def merge_groups(dilated_labels, stats, region_list, n_list, roots=False):
    """get_merged_regions grouping (tiff_analysis.py:843-878): group id per list entry, 0 = dropped.
    roots=True: `dilated_labels` is the parent image of dilated_roots()."""
    dl = _req(dilated_labels, torch.int32, 3)
    stats = _req(stats, torch.int64, 3)
    region_list = _req(region_list, torch.int32, 2)
    n_list = _req(n_list, torch.int32, 1)
    B, H, W = dl.shape
    cap = stats.shape[1]
    list_cap = region_list.shape[1]
    _list_args(B, stats, region_list, n_list)
    group_of = torch.zeros((B, list_cap), dtype=torch.int32, device=dl.device)
    n_groups = torch.zeros((B,), dtype=torch.int32, device=dl.device)
    _call("merge_groups", dl, int(bool(roots)), stats, region_list, n_list, group_of, n_groups, B, H, W, cap, list_cap,
          ws=(B, list_cap))
    return group_of, n_groups


def group_reduce(stats, region_list, n_list, group_of, n_groups, H, W):
    """member sums of merged groups (tiff_analysis.py:855-872): int64 (B, list_cap, 8)."""
    stats = _req(stats, torch.int64, 3)
    region_list = _req(region_list, torch.int32, 2)
    n_list = _req(n_list, torch.int32, 1)
    group_of = _req(group_of, torch.int32, 2)
    n_groups = _req(n_groups, torch.int32, 1)
    B, cap = stats.shape[0], stats.shape[1]
    list_cap = region_list.shape[1]
    _list_args(B, stats, region_list, n_list)
    if group_of.shape != region_list.shape or n_groups.shape[0] != B:
        raise ValueError("group_of must have region_list's shape, n_groups one entry per frame")
    gstats = torch.zeros((B, list_cap, 8), dtype=torch.int64, device=stats.device)
    _call("group_reduce", stats, region_list, n_list, group_of, n_groups, gstats, B, H, W, cap, list_cap)
    return gstats


class ClassTables:
    """Host-side class tables of pcseg_classify_regions built from the reference's ``cell_types`` dict and its
    MIN_CELL_AREA / MIN_CLUSTER_AREA constants (tiff_analysis.py:54-60, 754-773)."""

    def __init__(self, cell_types, cell_type_names, min_cell_area, min_cluster_area):
        self.slot_names = []
        slot = np.full(256, 255, np.uint8)
        particle = np.zeros(256, np.uint8)
        for val, name in cell_types.items():
            if name in cell_type_names:
                if name not in self.slot_names:
                    self.slot_names.append(name)
                slot[val] = self.slot_names.index(name)
            elif name == "Particle":
                particle[val] = 1
        if len(self.slot_names) > 4:
            raise ValueError("at most 4 cell types")
        if any(not (0 <= int(v) < 64) for v, t in cell_types.items() if t in cell_type_names or t == "Particle"):
            raise ValueError("cell / particle class values must be below 64 (they index a 64-bit class set)")
        self.slot = slot
        self.particle = particle
        self.min_cell = np.array([min_cell_area[n] for n in self.slot_names] or [0], np.int32)
        self.min_cluster = np.array([min_cluster_area[n] for n in self.slot_names] or [0], np.int32)
        # class value that get_cell_clusters_from_distances looks up per type: the FIRST key with that name (:806-810)
        self.slot_value = []
        for n in self.slot_names:
            self.slot_value.append([v for v, t in cell_types.items() if t == n][0])
        self.cell_values = [v for v, t in cell_types.items() if t in cell_type_names]
        self.particle_value = None
        for v, t in cell_types.items():
            if t == "Particle":
                self.particle_value = v


def classify_regions(stats, cls_out, counts, tables):
    """per-region loop of get_cell_positions_and_areas + region lists (tiff_analysis.py:754-781, 794-796)."""
    stats = _req(stats, torch.int64, 3)
    cls_out = _req(cls_out, torch.uint8, 2)
    counts = _req(counts, torch.int32, 1)
    B, cap = stats.shape[0], stats.shape[1]
    if tuple(stats.shape) != (B, cap, 8) or tuple(cls_out.shape) != (B, cap) or counts.shape[0] != B:
        raise ValueError("stats must be (B, cap, 8), cls_out (B, cap), counts (B,)")
    dev = stats.device
    # no fills: the kernel writes kind / slot_of / cells for every region below counts[b], the lists up to their lengths and
    # every per-frame scalar; nothing reads beyond those (eight fill launches per batch, 26 MB of them, for nothing)
    out = {
        "kind": torch.empty((B, cap), dtype=torch.uint8, device=dev),
        "slot_of": torch.empty((B, cap), dtype=torch.uint8, device=dev),
        "cells": torch.empty((B, cap), dtype=torch.int32, device=dev),
        "particle_area": torch.empty((B,), dtype=torch.int64, device=dev),
        "type_stats": torch.empty((B, 4, 4), dtype=torch.int64, device=dev),
        "region_list": torch.empty((B, 5, cap), dtype=torch.int32, device=dev),
        "n_list": torch.empty((B, 5), dtype=torch.int32, device=dev),
        "nan_flag": torch.empty((B,), dtype=torch.int32, device=dev),
    }
    _call("classify_regions", stats, cls_out, counts, tables.slot, tables.particle, tables.min_cell, tables.min_cluster,
          len(tables.slot_names), out["kind"], out["slot_of"], out["cells"], out["particle_area"], out["type_stats"],
          out["region_list"], out["n_list"], out["nan_flag"], B, cap)
    return out


Points = collections.namedtuple("Points", "coords slot ids frame_offsets")
Points.__doc__ = """A packed point set on the device: ``coords`` (n, 2) float64, ``slot`` (n,) int32 type slot (-1: none),
``ids`` (n,) int32 labels and ``frame_offsets`` (B + 1,) int64, the points of a frame contiguous."""


def _alloc_points(n, B, device):
    """Buffers for ``n`` points of ``B`` frames, one spare row each (an empty set still has non-null pointers): hand the
    buffers to the library, then keep ``_head(points, n)``."""
    return Points(torch.empty((n + 1, 2), dtype=torch.float64, device=device), torch.empty((n + 1,), dtype=torch.int32, device=device),
                  torch.empty((n + 1,), dtype=torch.int32, device=device), torch.empty((B + 1,), dtype=torch.int64, device=device))


def _head(points, n):
    return Points(points.coords[:n], points.slot[:n], points.ids[:n], points.frame_offsets)


def _addr(keep, what, t, dtype, shape):
    """Address of a checked tensor for a field of a ctypes struct; ``keep`` holds the tensor until the kernels are enqueued."""
    t = _req(t, dtype, len(shape))
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s input of shape %s, expected %s" % (what, tuple(t.shape), tuple(shape)))
    keep.append(t)
    return t.data_ptr()


# the dense tables of a batch as the optional stages need them: `cells` with its spare row, row counts, table workspace
_Dense = collections.namedtuple("_Dense", "cells n_roi n_cell ws B")


def _dense_tables(res, groups, frame_ids, C, ratios, check):
    """pcseg_table_layout + pcseg_table_write: (dict of ``rois`` / ``cells`` / ``groups`` / ``frames``, :class:`_Dense`)."""
    B, cap = res["stats"].shape[0], res["stats"].shape[1]
    dev = res["stats"].device
    if len(ratios) > 8 or any(len(den) > 4 for _, _, den in ratios):
        raise ValueError("at most 8 ratios of at most 4 denominator planes")
    ti = _lib.TableInputs()
    ti.B, ti.cap, ti.C, ti.n_ratios = B, cap, C, len(ratios)
    keep = []  # tensors referenced by raw pointers until the kernels are enqueued
    ptr = functools.partial(_addr, keep, "table")
    ti.frame_ids = ptr(frame_ids, torch.int64, (B,))
    ti.counts = ptr(res["counts"], torch.int32, (B,))
    ti.stats = ptr(res["stats"], torch.int64, (B, cap, 8))
    ti.cls_out = ptr(res["cls_out"], torch.uint8, (B, cap))
    ti.cc_sums = ptr(res["cc_sums"], torch.float64, (B, cap, C))
    ti.kind = ptr(res["kind"], torch.uint8, (B, cap))
    ti.slot_of = ptr(res["slot_of"], torch.uint8, (B, cap))
    ti.cells = ptr(res["cells"], torch.int32, (B, cap))
    ti.particle_area = ptr(res["particle_area"], torch.int64, (B,))
    ti.overlap_area = ptr(res["overlap_area"], torch.int64, (B,))
    ti.type_stats = ptr(res["type_stats"], torch.int64, (B, 4, 4))
    ti.tie_flags = ptr(res["tie_flags"], torch.int32, (B,))
    ti.region_list = ptr(res["region_list"], torch.int32, (B, 5, cap))
    ti.n_list = ptr(res["n_list"], torch.int32, (B, 5))
    for s, g in groups.items():
        ti.group_of[s] = ptr(g["group_of"], torch.int32, (B, cap))
        ti.n_groups[s] = ptr(g["n_groups"], torch.int32, (B,))
        ti.group_stats[s] = ptr(g["group_stats"], torch.int64, (B, cap, 8))
    ti.n_markers = ptr(res["n_markers"], torch.int32, (B,))
    ti.ws_stats = ptr(res["ws_stats"], torch.int64, (B, cap, 8))
    ti.ws_sums = ptr(res["ws_sums"], torch.float64, (B, cap, C))
    for k, (_, num, den) in enumerate(ratios):
        ti.ratio_num[k] = int(num)
        for j in range(4):
            ti.ratio_den[k][j] = int(den[j]) if j < len(den) else -1
    ti.overflow = ptr(res["overflow"], torch.int32, (B,))
    ti.ws_overflow = ptr(res["ws_overflow"], torch.int32, (B,))
    ti.nan_flag = ptr(res["nan_flag"], torch.int32, (B,))
    ws = _workspace("table_layout", dev, B, cap)
    totals = torch.empty((6,), dtype=torch.int64, device=dev)
    _call("table_layout", ctypes.byref(ti), totals, ws=ws)
    # the one host read: sizes of the outputs, plus the flags BatchResult.check() would otherwise fetch one by one
    n_roi, n_cell, n_group, n_overflow, n_ws_overflow, n_nan = (int(v) for v in totals.cpu())
    if check and (n_overflow or n_ws_overflow):
        raise RuntimeError("region table capacity exceeded: raise FramePipeline(cap=...)")
    if check and n_nan:
        raise ValueError("cannot convert float NaN to integer")  # tiff_analysis.py:776-781
    nr = len(ratios)
    # (one spare row each: an empty table still needs a non-null pointer for the library's argument check)
    rois = torch.empty((n_roi + 1, 5 + C + nr), dtype=torch.float64, device=dev)
    cells = torch.empty((n_cell + 1, 14 + C + nr), dtype=torch.float64, device=dev)
    grp = torch.empty((n_group + 1, 11), dtype=torch.float64, device=dev)
    frames = torch.empty((B, 17), dtype=torch.int64, device=dev)
    _call("table_write", ctypes.byref(ti), rois, cells, grp, frames, ws=ws)
    out = {"rois": rois[:n_roi], "cells": cells[:n_cell], "groups": grp[:n_group], "frames": frames, "frame_ids": frame_ids}
    return out, _Dense(cells, n_roi, n_cell, ws[0], B)


def _cell_distances(d, slots, raster):
    """pcseg_cell_distances: one value per row of ``cells``, NaN = no entry."""
    dist = torch.empty((d.n_cell + 1,), dtype=torch.float64, device=d.cells.device)
    _call("cell_distances", d.cells, d.n_cell, d.cells.shape[1], slots, float(raster), 512.0, dist, d.B, d.ws, d.ws.numel())
    return dist[:d.n_cell]


def _pack_cells(name, d, slots):
    """pcseg_<name>: the rows of ``cells`` as :class:`Points` (``slots``: class value -> type slot, uint8[256] numpy)."""
    pts = _alloc_points(d.n_cell, d.B, d.cells.device)
    _call(name, d.cells, d.cells.shape[1], slots, d.B, d.ws, d.ws.numel(), *pts)
    return _head(pts, d.n_cell)


def _neighbours(points, K, scale, edges):
    dist, nn_id, hist = point_neighbours(*points, K, scale, edges)
    return {"dist": dist, "nn_id": nn_id, "hist": hist, "points": points}


def _surface_rows(points, surface, mask, scale, K, edges):
    """:func:`surface_distances` of packed query rows, with what a table of them needs: dict of ``dist``, ``nearest``,
    ``inside``, ``hist`` (None without ``edges``) and ``points``."""
    dist, nearest, inside, hist = surface_distances(points.coords, points.frame_offsets, surface, scale, mask=mask,
                                                    slot=points.slot, n_types=K, edges=edges)
    return {"dist": dist, "nearest": nearest, "inside": inside, "hist": hist, "points": points}


def _refined_surface(res, points, surface, mask, scale, K, edges):
    """:func:`_surface_rows` of the refined points, at their centroids (pcseg_surface_pack_refined)."""
    return _surface_rows(points._replace(coords=_refined_centroids(res, points)), surface, mask, scale, K, edges)


def _refined_centroids(res, points):
    """(row, col) of the refined points, 0-based, as the ``refined`` table prints them (pcseg_surface_pack_refined)."""
    B, cap, n = res["stats"].shape[0], res["stats"].shape[1], points.ids.shape[0]
    rc = torch.empty((n + 1, 2), dtype=torch.float64, device=points.ids.device)
    _call("surface_pack_refined", _req(res["ws_stats"], torch.int64, 3), cap, points.ids, points.frame_offsets, n, B, rc)
    return rc[:n]


# The ROIs of one label batch that a per-ROI table has a row for: the label image, its per-frame label counts, its region
# table ((B, cap, 8) of region_reduce), the rows wanted ((B, cap) bool) and their type slots ((B, cap) uint8).
RoiRows = collections.namedtuple("RoiRows", "labels counts stats live slot_of")


def _rows_below(counts, cap):
    return torch.arange(cap, device=counts.device)[None, :] < counts[:, None]


def class_rows(res):
    """:class:`RoiRows` of the class-map components of a batch: the rows of ``cells`` (kind >= 1)."""
    live = (res["kind"] >= 1) & _rows_below(res["counts"], res["stats"].shape[1])
    return RoiRows(res["labels"], res["counts"], res["stats"], live, res["slot_of"])


def refined_rows(res, kind_r, slot_r):
    """:class:`RoiRows` of the refined ROIs of a batch, classified by :func:`refined_tables` (its ``kind_r`` / ``slot_r``):
    the refined rows of kind >= 1 that own a pixel."""
    live = (kind_r >= 1) & (res["ws_stats"][:, :, 0] > 0) & _rows_below(res["n_markers"], res["stats"].shape[1])
    return RoiRows(res["ws_labels"], res["n_markers"], res["ws_stats"], live, slot_r)


def _slot_column(slot_of, b, l):
    slot = slot_of[b, l].to(torch.int64)
    return torch.where(slot < 4, slot, torch.full_like(slot, -1)).to(torch.float64)


def _row_head(live, slot_of, frame_ids):
    """The rows ``live`` in (frame, label) order: their indices ``b, l`` and the columns ``[frame, label, slot]``."""
    b, l = torch.nonzero(live, as_tuple=True)
    return b, l, [frame_ids[b].to(torch.float64), (l + 1).to(torch.float64), _slot_column(slot_of, b, l)]


def _over(x, divisor):
    """``x / divisor`` with a TENSOR divisor: a correctly rounded division per element (a Python scalar divisor is turned
    into a multiplication by its reciprocal on the device, one ulp off for some values -- the columns are promised equal to
    numpy's quotient)."""
    return x / torch.full_like(x, divisor)


def _shape_rows(rows, frame_ids, scale):
    """The ``shapes`` table of one label batch (:class:`RoiRows`): :func:`region_shape` + :func:`shape_properties` on the
    whole batch, then the rows ``live`` in (frame, label) order as ``[frame, label, slot, n_border, n_1, n_sqrt2, n_mid, mu_rr,
    mu_rc, mu_cc, major_um, minor_um, eccentricity, orientation, equivalent_diameter_um, extent, perimeter_um]``
    (lengths / ``scale``; the second central moments stay in pixels)."""
    shape, _ = region_shape(rows.labels, rows.counts, cap=rows.stats.shape[1])
    props = shape_properties(rows.stats, shape, rows.counts)
    b, l, head = _row_head(rows.live, rows.slot_of, frame_ids)
    sh, pr = shape[b, l].to(torch.float64), props[b, l]
    um = lambda k: pr[:, k] / scale
    return torch.stack(head + [sh[:, 6], sh[:, 3], sh[:, 4], sh[:, 5], pr[:, 2], -pr[:, 1], pr[:, 0], um(5), um(6), pr[:, 7],
                               pr[:, 8], um(9), pr[:, 10], um(11)], dim=1)


def _hull_rows(rows, frame_ids, scale):
    """The ``convexity`` table of one label batch (:class:`RoiRows`): :func:`region_hull` + :func:`hull_properties` on the
    whole batch, then the rows ``live`` in (frame, label) order as ``[frame, label, slot, convex_area, solidity, feret_um,
    euler_number, convex_area_um2]`` (the length / ``scale``, the area / ``scale`` ^ 2, each ONE correctly rounded division)."""
    hull, _ = region_hull(rows.labels, rows.counts, rows.stats, cap=rows.stats.shape[1])
    props = hull_properties(rows.stats, hull, rows.counts)
    b, l, head = _row_head(rows.live, rows.slot_of, frame_ids)
    pr = props[b, l]
    return torch.stack(head + [pr[:, 0], pr[:, 1], _over(pr[:, 2], scale), pr[:, 3], _over(pr[:, 0], scale * scale)], dim=1)


def _skeleton_rows(rows, frame_ids, scale):
    """The ``skeletons`` table of one label batch (:class:`RoiRows`): :func:`thin_labels` + :func:`region_skeleton` +
    :func:`skeleton_properties` on the whole batch, then the rows ``live`` in (frame, label) order as ``[frame, label, slot,
    skel_px, n_orth, n_diag, n_end, n_junction, passes, length_um, width_um]`` (the two lengths / ``scale``, each ONE correctly
    rounded division)."""
    # only the rows asked for are thinned (every label is thinned on its own, so their skeletons do not change): the class-map
    # components cover the whole frame, and background and particle would set the iteration count and keep every tile listed
    live, labels = rows.live, rows.labels
    B, cap = live.shape
    keep = torch.zeros((B, cap + 2), dtype=torch.int32, device=labels.device)
    keep[:, 1:cap + 1] = live * torch.arange(1, cap + 1, dtype=torch.int32, device=labels.device)
    labels = torch.gather(keep, 1, labels.clamp(0, cap + 1).reshape(B, -1).to(torch.int64)).reshape(labels.shape)
    peel, _ = thin_labels(labels)
    table = region_skeleton(labels, peel, rows.counts, cap=cap)
    props = skeleton_properties(rows.stats, table, rows.counts)
    b, l, head = _row_head(live, rows.slot_of, frame_ids)
    return torch.cat([torch.stack(head, dim=1), table[b, l].to(torch.float64), _over(props[b, l], scale)], dim=1)


TableSwitches = collections.namedtuple(
    "TableSwitches", "neighbours pair_edges mixing mixing_seed refined surface surface_edges territory territory_reach skeleton convex shape",
    defaults=(False, None, None, 0, False, False, None, False, None, False, False, False))
TableSwitches.__doc__ = """The switches of the optional tables, as ``FramePipeline.tables`` / ``tables_device`` /
``host_tables`` / ``table_columns`` / ``empty_device_tables`` take them as keywords and :func:`build_tables` as one object.
What each one adds is described once, in the docstring of ``FramePipeline.tables_device``; the tables and their columns
stand in ``pipeline.OPTIONAL_TABLES``."""

# the per-ROI tables that one RoiRows -> rows function makes: (table name, switch, rows function), in stage order
_ROI_TABLES = (("skeletons", "skeleton", _skeleton_rows), ("convexity", "convex", _hull_rows), ("shapes", "shape", _shape_rows))


def build_tables(res, groups, frame_ids, C, ratios, check=False, distance_slots=None, raster=19.0, tables=None,
                 switches=TableSwitches()):
    """csrc/tables.hip: dense row tables of one batch (see FramePipeline.tables_device), then one stage per switch of
    ``switches`` (a :class:`TableSwitches`), in this order; ``tables`` is the pipeline's :class:`ClassTables` (None only
    where no switch is on).  ``territory`` with ``territory_reach`` (um, None: unbounded): ``territories`` / ``adjacency`` =
    :func:`territory_rows` over the rows of ``cells`` (:func:`class_rows`: the labels of kind >= 1 are the sites), the
    particle mask of ``surface`` as its mask, and ``territory_overflow``.  ``skeleton`` / ``convex`` / ``shape``: ``skeletons`` /
    ``convexity`` / ``shapes`` = :func:`_skeleton_rows` / :func:`_hull_rows` / :func:`_shape_rows` over the same rows.
    ``distance_slots`` (the class value -> type slot table, uint8[256] numpy): ``cell_dist``, one value per row of ``cells``
    (NaN = no entry).  ``neighbours`` or ``pair_edges``: ``cell_nn`` = dict of ``dist`` / ``nn_id`` / ``hist`` of
    :func:`point_neighbours` (``hist`` None without ``pair_edges``) and the ``points`` (:class:`Points`) it ran over, the rows
    of ``cells``, at the scale of ``cell_dist``; ``mixing`` (P > 0, with ``pair_edges``): ``cell_mix`` =
    :func:`pair_label_mixing` over the same points (``mixing_seed``, keys = ``frame_ids``).  ``surface`` or ``surface_edges``
    (.m:271-309): ``cell_sf`` = the dict of :func:`_surface_rows` over the rows of ``cells`` against the surface of
    ``binary_fill_holes(res["recreated"] == Particle)``, plus ``surface_px`` / ``filled_area`` (B,) and with ``surface_edges``
    ``hist`` and ``shells`` (:func:`surface_shells`).  ``refined``: the outputs of :func:`refined_tables`, then ``refined_nn`` /
    ``refined_mix``, ``refined_sf`` and, with the ``refined_`` prefix, the per-ROI tables above: the same stages over the
    refined rows of kind >= 1 (:func:`refined_rows`, on the watershed labels)."""
    o = switches
    out, d = _dense_tables(res, groups, frame_ids, C, ratios, check)
    scale = 512.0 / float(raster)
    n_types = len(tables.slot_names) if tables is not None else 0
    pmask = None
    if o.territory:
        r2 = reach_um_r2(o.territory_reach, scale)
        pmask = particle_mask(res["recreated"], tables.particle_value)

    def roi_tables(prefix, rows):
        """the per-ROI stages over one set of rows: territory, then skeleton, convex and shape"""
        if o.territory:
            out[prefix + "territories"], out[prefix + "adjacency"], out[prefix + "territory_overflow"] = territory_rows(
                rows.labels, rows.live, rows.slot_of, frame_ids, scale, n_types, r2=r2, mask=pmask, check=check)
        for name, switch, rows_of in _ROI_TABLES:
            if getattr(o, switch):
                out[prefix + name] = rows_of(rows, frame_ids, scale)

    per_roi = o.territory or any(getattr(o, switch) for _, switch, _ in _ROI_TABLES)
    if per_roi:
        roi_tables("", class_rows(res))
    if distance_slots is not None:
        out["cell_dist"] = _cell_distances(d, distance_slots, raster)
    want_nn = o.neighbours or o.pair_edges is not None
    mixing = int(o.mixing or 0)
    if want_nn:
        out["cell_nn"] = _neighbours(_pack_cells("neighbours_pack_cells", d, tables.slot), n_types, scale, o.pair_edges)
        if mixing:
            out["mixing_args"] = (o.pair_edges, mixing)
            out["cell_mix"] = pair_label_mixing(out["cell_nn"]["points"], None, None, n_types, scale, o.pair_edges, mixing,
                                                o.mixing_seed, frame_keys=frame_ids)
    want_sf = o.surface or o.surface_edges is not None
    if want_sf:
        K = max(n_types, 1)
        mask, sf = particle_surface(res["recreated"], tables.particle_value, mask=pmask)
        out["cell_sf"] = _surface_rows(_pack_cells("surface_pack_cells", d, tables.slot), sf, mask, scale, K, o.surface_edges)
        out["cell_sf"].update(surface_px=sf["counts"], filled_area=sf["area"])
        if o.surface_edges is not None:
            out["cell_sf"]["shells"] = surface_shells(sf, mask, o.surface_edges, scale)
    if o.refined:
        refined_points = o.refined and want_nn
        out.update(refined_tables(res, frame_ids, tables, d.ws, (d.n_roi, d.n_cell), check=check, points=refined_points or want_sf))
        pts = out.pop("points", None)
        if refined_points:
            out["refined_nn"] = _neighbours(pts, n_types, scale, o.pair_edges)
            if mixing:
                out["refined_mix"] = pair_label_mixing(pts, None, None, n_types, scale, o.pair_edges, mixing, o.mixing_seed,
                                                       frame_keys=frame_ids)
        if want_sf:
            out["refined_sf"] = _refined_surface(res, pts, sf, mask, scale, K, o.surface_edges)
        if per_roi:
            roi_tables("refined_", refined_rows(res, out["kind_r"], out["slot_r"]))
    return out


def label_parent(labels_a, labels_r, counts_r, cls_a=None, cap=None, stats_r=None, return_spilled=False):
    """The class-map component every refined ROI lies in (refine_boundaries.py:1-12, goal 2; csrc/refined.hip).
    ``labels_a`` / ``labels_r`` (B, H, W) int32 CUDA tensors (A: class-map components, R: refined ROIs), ``counts_r``
    (B,) int32: rows r = 1 .. min(counts_r[b], cap).  With ov(r, a) = #pixels where R = r and A = a >= 1, returns
    ``(parent, parent_px, n_overlap, cls_r, overflow)``: (B, cap) int32 argmax_a ov(r, a) (the smallest a on ties, 0:
    none), (B, cap) int32 ov(r, parent), (B, cap) int32 #distinct a with ov > 0, (B, cap) uint8 ``cls_a[b, parent - 1]``
    (0 without ``cls_a`` or parent) and (B,) int32 set where a parent label exceeds ``cap`` (default: ``cls_a``'s
    second dimension, else max(counts_r)).  ``stats_r`` ((B, cap, 8) int64 of :func:`region_reduce` over ``labels_r``)
    bounds the exact pass that ROIs over more than sixteen components take; without it that pass scans the frame.
    ``return_spilled``: also the number of such ROIs, a (1,) int32 tensor."""
    la = _req(labels_a, torch.int32, 3)
    lr = _req(labels_r, torch.int32, 3)
    counts_r = _req(counts_r, torch.int32, 1)
    B, H, W = lr.shape
    if tuple(la.shape) != (B, H, W) or counts_r.shape[0] != B:
        raise ValueError("labels_a, labels_r and counts_r must agree on (B, H, W)")
    if cls_a is not None:
        cls_a = _req(cls_a, torch.uint8, 2)
        if cap is None:
            cap = cls_a.shape[1]
        if tuple(cls_a.shape) != (B, cap):
            raise ValueError("cls_a must be (B, cap)")
    if cap is None:
        cap = max(int(counts_r.max().item()) if B else 1, 1)
    cap = int(cap)
    if stats_r is not None:
        stats_r = _req(stats_r, torch.int64, 3)
        if tuple(stats_r.shape) != (B, cap, 8):
            raise ValueError("stats_r must be (B, cap, 8)")
    dev = lr.device
    parent = torch.empty((B, cap), dtype=torch.int32, device=dev)
    parent_px = torch.empty((B, cap), dtype=torch.int32, device=dev)
    n_overlap = torch.empty((B, cap), dtype=torch.int32, device=dev)
    cls_r = torch.empty((B, cap), dtype=torch.uint8, device=dev)
    overflow = torch.empty((B,), dtype=torch.int32, device=dev)
    n_spilled = torch.empty((1,), dtype=torch.int32, device=dev)
    _call("label_parent", la, lr, counts_r, stats_r, cls_a, parent, parent_px, n_overlap, cls_r, overflow, n_spilled, B, H, W, cap,
          ws=(B, H, W, cap))
    out = (parent, parent_px, n_overlap, cls_r, overflow)
    return out + (n_spilled,) if return_spilled else out


def _pair_fill(entry, head, shape, dev, query):
    """The first call of a per-frame pair table (csrc/pair_table.h), ``pcseg_<entry>(*head, overflow, offsets, totals, B, H, W,
    workspace, nbytes, stream)``: the workspace of the table's size query at ``query``, ``overflow`` int32 (B,), ``offsets``
    int64 (B + 1,) and ``totals`` int64 (2,) = (rows, frames whose table was full).  Nothing is read back.  Returns the state
    the second calls need."""
    B = shape[0]
    ws, nbytes = _workspace(entry, dev, *query)
    st = {"B": B, "nbytes": nbytes, "ws": ws, "overflow": torch.empty((B,), dtype=torch.int32, device=dev),
          "offsets": torch.empty((B + 1,), dtype=torch.int64, device=dev), "totals": torch.empty((2,), dtype=torch.int64, device=dev)}
    _call(entry, *head, st["overflow"], st["offsets"], st["totals"], *shape, ws=(ws, nbytes))
    return st


def _pair_rows(st, columns, write):
    """The second call on :func:`_pair_fill`'s state: the one host read (``totals``), the row buffers ``key`` int64, ``frame``
    int32 and one per (name, dtype, trailing shape) of ``columns`` -- each with a spare row: never a null pointer --,
    ``write(offsets, buffers, workspace, nbytes)`` with the buffers by name, and the rows in (frame, key) order.
    Returns ``(rows, n_overflow, sorted)``: ``sorted`` holds ``key``, ``frame`` (int64) and the columns."""
    dev = st["totals"].device
    rows, n_over = (int(v) for v in st["totals"].cpu())
    buf = {name: torch.empty((rows + 1,) + tuple(shape), dtype=dtype, device=dev)
           for name, dtype, shape in (("key", torch.int64, ()), ("frame", torch.int32, ())) + tuple(columns)}
    write(st["offsets"], buf, st["ws"], st["nbytes"])
    # (frame, key) order: the rows of a frame are contiguous already, in table order -- two stable sorts, plumbing; the
    # frames' offsets hold for the sorted rows too
    key, frame = buf["key"][:rows], buf["frame"][:rows].to(torch.int64)
    order = torch.sort(key, stable=True)[1]
    order = order[torch.sort(frame[order], stable=True)[1]]
    out = {name: t[:rows][order] for name, t in buf.items()}
    out["frame"] = frame[order]
    return rows, n_over, out


def _pair_ab(key):
    """The two labels of a pair key."""
    return key >> 32, key & 0xFFFFFFFF


def _contingency_rows(labels_t, labels_s, cap_t, cap_s, pair_cap):
    """The two calls of the contingency table and the (frame, t, s) sort of its rows."""
    lt, ls = _label_batch(labels_t, "labels_t"), _label_batch(labels_s, "labels_s")
    if lt.shape != ls.shape:
        raise ValueError("labels_t and labels_s must have one shape")
    B, H, W = lt.shape
    dev = lt.device
    if cap_t is None or cap_s is None:
        top = torch.stack([lt.max(), ls.max()]).cpu()  # (one read for both defaults)
        cap_t = int(top[0]) if cap_t is None else cap_t
        cap_s = int(top[1]) if cap_s is None else cap_s
    cap_t, cap_s = max(int(cap_t), 1), max(int(cap_s), 1)
    if pair_cap is None:
        pair_cap = 1 << (4 * (cap_t + cap_s) + 64 - 1).bit_length()
    pair_cap = int(pair_cap)
    st = _pair_fill("label_contingency", (lt, ls, cap_t, cap_s, pair_cap), (B, H, W), dev, (B, pair_cap))
    rows, n_over, r = _pair_rows(st, (("n", torch.int64, ()),), lambda offsets, out, ws, nbytes: _call(
        "contingency_write", pair_cap, offsets, out["key"], out["frame"], out["n"], B, ws=(ws, nbytes)))
    return {"key": r["key"], "frame": r["frame"], "n": r["n"], "offsets": st["offsets"], "rows": rows, "overflow": st["overflow"],
            "n_overflow": n_over, "cap_t": cap_t, "cap_s": cap_s, "pair_cap": pair_cap, "shape": (B, H, W)}


def _agreement_match(rows, thresholds):
    """pcseg_agreement_match on :func:`_contingency_rows`' result."""
    B = rows["shape"][0]
    cap_t, cap_s = rows["cap_t"], rows["cap_s"]
    dev = rows["offsets"].device
    thr = [float(v) for v in thresholds]
    if len(thr) > 8 or any(not 0.5 <= v <= 1.0 for v in thr):
        raise ValueError("at most 8 IoU thresholds, each in [0.5, 1]")
    thr_arg = (ctypes.c_double * max(len(thr), 1))(*thr)
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    out = {"area_t": new((B, cap_t), torch.int64), "area_s": new((B, cap_s), torch.int64),
           "best_t": new((B, cap_t, 3), torch.int32), "iou_t": new((B, cap_t), torch.float64),
           "best_s": new((B, cap_s, 3), torch.int32), "iou_s": new((B, cap_s), torch.float64),
           "match_t": new((B, cap_t), torch.uint8), "match_s": new((B, cap_s), torch.uint8),
           "frame_ints": new((B, 6 + len(thr)), torch.int64)}
    _call("agreement_match", rows["key"], rows["n"], rows["offsets"], rows["rows"], cap_t, cap_s, thr_arg, len(thr), out["area_t"],
          out["area_s"], out["best_t"], out["iou_t"], out["best_s"], out["iou_s"], out["match_t"], out["match_s"], out["frame_ints"], B)
    return out


def label_contingency(labels_t, labels_s, cap_t=None, cap_s=None, pair_cap=None):
    """The contingency table of two label images (csrc/agreement.hip, include/pcseg.h): ``labels_t`` (truth) / ``labels_s``
    (test) int32 (B, H, W) CUDA tensors of any width and alignment; a value outside 0 .. ``cap_t`` / ``cap_s`` (default: the
    largest label, read back once) is read as background.  Returns a dict: ``frame``, ``t``, ``s``, ``n`` int64 (rows,) --
    every pair with n > 0 pixels except (0, 0), pairs with the background included, sorted by (frame, t, s) --, ``area_t``
    int64 (B, cap_t) and ``area_s`` int64 (B, cap_s) the pixels per label, ``overflow`` int32 (B,): bit 1 (value 1) where
    the frame has more pairs than ``pair_cap`` (default: a power of two >= 4 (cap_t + cap_s) + 64; its rows are then
    incomplete), bit 2 (value 2) where a label above its cap was seen, and ``n_overflow``, the number of frames with bit 1
    (read back with the row total, the one host read between the two calls)."""
    rows = _contingency_rows(labels_t, labels_s, cap_t, cap_s, pair_cap)
    m = _agreement_match(rows, ())
    t, s = _pair_ab(rows["key"])
    return {"frame": rows["frame"], "t": t, "s": s, "n": rows["n"], "area_t": m["area_t"], "area_s": m["area_s"],
            "overflow": rows["overflow"], "n_overflow": rows["n_overflow"], "pair_cap": rows["pair_cap"]}


AGREEMENT_SCORES = ("tp", "fp", "fn", "precision", "recall", "f1", "ap", "mean_matched_iou")


def agreement_scores(frame_ints, iou_t, match_t, frame, t, s, n, area_t, area_s, n_px, n_thr):
    """Host only: the per-frame scores from the integers of the match step, float64, IEEE results for a zero denominator.
    Arrays are numpy: ``frame_ints`` (B, 6 + n_thr), ``iou_t`` / ``match_t`` (B, cap_t), the sorted pair rows, the areas and
    ``n_px`` = H W.  Returns a dict of arrays: the ``AGREEMENT_SCORES`` (B, n_thr); ``are``, ``are_precision``,
    ``are_recall`` (``skimage.metrics.adapted_rand_error(T, S)``: truth 0 ignored) and ``vi_split``, ``vi_merge``
    (``skimage.metrics.variation_of_information(T, S)``: label 0 and n(0, 0) included), (B,).  Sums of floats are
    ``math.fsum``: exactly rounded, so no order enters."""
    import math
    B = frame_ints.shape[0]
    out = {k: np.zeros((B, n_thr), np.float64) for k in AGREEMENT_SCORES}
    for k in ("are", "are_precision", "are_recall", "vi_split", "vi_merge"):
        out[k] = np.zeros((B,), np.float64)
    first = np.searchsorted(frame, np.arange(B + 1))
    f64 = np.float64
    with np.errstate(all="ignore"):
        for b in range(B):
            fi = [int(v) for v in frame_ints[b]]
            n_truth, n_rois, N1, S_pp, S_a, S_b = fi[:6]
            for k in range(n_thr):
                tp = fi[6 + k]
                matched = (match_t[b] >> k) & 1 != 0
                out["tp"][b, k], out["fp"][b, k], out["fn"][b, k] = tp, n_rois - tp, n_truth - tp
                out["precision"][b, k] = f64(tp) / f64(n_rois)
                out["recall"][b, k] = f64(tp) / f64(n_truth)
                out["f1"][b, k] = f64(2 * tp) / f64(n_truth + n_rois)
                out["ap"][b, k] = f64(tp) / f64(n_truth + n_rois - tp)
                out["mean_matched_iou"][b, k] = f64(math.fsum(iou_t[b][matched].tolist())) / f64(tp)
            p2 = S_pp - N1
            prec = f64(p2) / f64(S_a - N1)
            rec = f64(p2) / f64(S_b - N1)
            f = 2. * prec * rec / (prec + rec)
            out["are"][b], out["are_precision"][b], out["are_recall"][b] = 1. - f, prec, rec
            # variation of information over every pair, (0, 0) included
            lo, hi = first[b], first[b + 1]
            tt, ss, nn = t[lo:hi].tolist(), s[lo:hi].tolist(), n[lo:hi].tolist()
            n00 = n_px - sum(nn)
            a0 = n00 + sum(v for u, v in zip(tt, nn) if u == 0)
            b0 = n00 + sum(v for u, v in zip(ss, nn) if u == 0)
            at, bs = [a0] + area_t[b].tolist(), [b0] + area_s[b].tolist()
            if n00 > 0:
                tt, ss, nn = tt + [0], ss + [0], nn + [n00]
            split = [(v / n_px) * math.log2(v / at[u]) for u, v in zip(tt, nn)]
            merge = [(v / n_px) * math.log2(v / bs[u]) for u, v in zip(ss, nn)]
            out["vi_split"][b], out["vi_merge"][b] = -math.fsum(split), -math.fsum(merge)
    return out


def label_agreement(labels_t, labels_s, thresholds=(0.5, 0.75, 0.9), cap_t=None, cap_s=None, pair_cap=None):
    """How well the test labels ``labels_s`` agree with the truth labels ``labels_t`` (arguments as
    :func:`label_contingency`).  Returns a dict: the pair rows ``frame``, ``t``, ``s``, ``n``; the arrays of
    pcseg_agreement_match (include/pcseg.h) as CUDA tensors -- ``area_t``, ``area_s``, ``best_t`` / ``best_s`` int32 (B, cap,
    3) = best partner (the largest IoU, compared exactly; the smallest label among equals), its overlap, the number of
    partners, ``iou_t`` / ``iou_s`` float64 (NaN without partner), ``match_t`` / ``match_s`` uint8: bit k set where the label
    is matched at ``thresholds[k]`` (``2 n > U`` and ``iou >= tau``: at most one partner per label qualifies, so no
    assignment is needed), ``frame_ints`` int64 (B, 6 + n_thr) --; ``thresholds``; ``overflow`` / ``n_overflow``; and
    ``scores``, :func:`agreement_scores` of every frame (numpy, computed on the host from the integers)."""
    thresholds = tuple(float(v) for v in thresholds)
    rows = _contingency_rows(labels_t, labels_s, cap_t, cap_s, pair_cap)
    out = _agreement_match(rows, thresholds)
    key = rows["key"]
    out.update({"frame": rows["frame"], "t": key >> 32, "s": key & 0xFFFFFFFF, "n": rows["n"], "thresholds": thresholds,
                "overflow": rows["overflow"], "n_overflow": rows["n_overflow"], "pair_cap": rows["pair_cap"]})
    B, H, W = rows["shape"]
    host = {k: out[k].cpu().numpy() for k in ("frame_ints", "iou_t", "match_t", "frame", "t", "s", "n", "area_t", "area_s")}
    out["scores"] = agreement_scores(n_px=H * W, n_thr=len(thresholds), **host)
    return out


def agreement_columns(thresholds):
    """Column names of :func:`agreement_tables` for these IoU thresholds."""
    tags = ["%g" % v for v in thresholds]
    per_label = lambda partner: ["frame", "label", "area", partner, "overlap_px", "iou", "n_partners"] + ["matched_" + g for g in tags]
    return {"agreement_pairs": ["frame", "truth", "label", "px", "truth_area", "area", "iou"],
            "agreement_rois": per_label("best_truth"), "agreement_truth": per_label("best_label"),
            "frames_agreement": ["frame", "n_truth", "n_rois"] + ["%s_%s" % (k, g) for g in tags for k in AGREEMENT_SCORES]
                                + ["are", "are_precision", "are_recall", "vi_split", "vi_merge"]}


def agreement_tables(ag, frame_ids=None):
    """Host only: :func:`label_agreement`'s result as float64 numpy tables with ``<name>_columns`` lists --
    ``agreement_pairs`` (one row per pair of a truth label and a test label that share pixels), ``agreement_rois`` /
    ``agreement_truth`` (one row per test / truth label with pixels, in label order) and ``frames_agreement`` (one row per
    frame).  ``frame_ids``: the frames' ids (default: their position in the batch)."""
    thr = ag["thresholds"]
    host = {k: ag[k].cpu().numpy() for k in ("frame", "t", "s", "n", "area_t", "area_s", "best_t", "best_s", "iou_t", "iou_s", "match_t",
                                           "match_s", "frame_ints")}
    B = host["area_t"].shape[0]
    fid = np.arange(B, dtype=np.float64) if frame_ids is None else np.asarray(frame_ids, np.float64)
    if fid.shape != (B,):
        raise ValueError("frame_ids must name every frame of the batch")
    cols = agreement_columns(thr)
    out = {}
    fg = (host["t"] >= 1) & (host["s"] >= 1)
    f, t, s, n = (host[k][fg] for k in ("frame", "t", "s", "n"))
    at, bs = host["area_t"][f, t - 1], host["area_s"][f, s - 1]
    out["agreement_pairs"] = np.stack([fid[f], t, s, n, at, bs, n.astype(np.float64) / (at + bs - n).astype(np.float64)],
                                      axis=1).astype(np.float64).reshape(-1, 7)
    for name, side in (("agreement_rois", "s"), ("agreement_truth", "t")):
        area, best, iou, match = host["area_" + side], host["best_" + side], host["iou_" + side], host["match_" + side]
        b, l = np.nonzero(area > 0)
        columns = [fid[b], l + 1, area[b, l], best[b, l, 0], best[b, l, 1], iou[b, l], best[b, l, 2]]
        columns += [(match[b, l] >> k) & 1 for k in range(len(thr))]
        out[name] = np.stack(columns, axis=1).astype(np.float64).reshape(-1, len(cols[name]))
    sc = ag["scores"]
    columns = [fid, host["frame_ints"][:, 0], host["frame_ints"][:, 1]]
    columns += [sc[k][:, i] for i in range(len(thr)) for k in AGREEMENT_SCORES]
    columns += [sc[k] for k in ("are", "are_precision", "are_recall", "vi_split", "vi_merge")]
    out["frames_agreement"] = np.stack(columns, axis=1).astype(np.float64).reshape(B, len(cols["frames_agreement"]))
    for k, v in cols.items():
        out[k + "_columns"] = v
    return out


def check_agreement_overflow(ag):
    """RuntimeError where a frame's pair table was full (overflow bit 1): its rows are incomplete."""
    if ag["n_overflow"]:
        full = [int(b) for b in torch.nonzero((ag["overflow"] & 1).cpu())[:, 0]]
        raise RuntimeError("the contingency table of frame(s) %s is full: pair_cap = %d is too small" % (full, ag["pair_cap"]))


BORDER_TABLE_FULL, BORDER_ABOVE_CAP, BORDER_VALUE, BORDER_CORRUPT = 1, 2, 4, 8  # bits of the per-frame border flags (include/pcseg.h)
_BORDER_BY = {"mean": 0, "saddle": 1}


@functools.lru_cache(maxsize=None)
def border_block():
    """``(R, C, lds_labels)`` of csrc/borders.hip: rows and columns of a block of the fill kernel, and the ``cap + 1`` up to
    which the merge keeps its parents in LDS."""
    out = (ctypes.c_int32 * 3)()
    _call("border_block", out)
    return tuple(int(v) for v in out)


def _border_fill(labels, strength, conn, cap, pair_cap, counts=None):
    """pcseg_label_borders: the filled tables.  Returns the state the second calls need (``counts``, checked before anything
    is enqueued, among them)."""
    labels = _label_batch(labels)
    strength, fstride = _plane_view(strength)
    if tuple(strength.shape) != tuple(labels.shape):
        raise ValueError("labels and strength must have one shape")
    if counts is not None:
        counts = _req(counts, torch.int32, 1)
        if counts.shape[0] != labels.shape[0]:
            raise ValueError("counts must be (B,)")
    if conn not in (4, 8):
        raise ValueError("conn must be 4 or 8")
    B, H, W = labels.shape
    if cap is None:
        cap = int(labels.max().item())
    cap = max(int(cap), 1)
    pair_cap = 4 * cap if pair_cap is None else int(pair_cap)
    st = _pair_fill("label_borders", (labels, strength, fstride, cap, conn, pair_cap), (B, H, W), labels.device, (B, pair_cap, cap))
    st.update(labels=labels, cap=cap, pair_cap=pair_cap, counts=counts)
    return st


def label_borders(labels, strength, conn=8, cap=None, pair_cap=None):
    """The borders between touching regions of a label image, weighed by a probability image (csrc/borders.hip; the
    definitions: include/pcseg.h): ``labels`` int32 (B, H, W) CUDA tensor of any width and alignment, ``strength`` float32 of
    the same shape (a plane view of a (B, C, H, W) stack is read in place).  A link is a pair of 4- (``conn`` = 4) or
    8-neighbour pixels with different labels in 1 .. ``cap`` (default: the largest label, read back once), counted once; its
    value is the larger of the two pixels' strengths, NaN read as 0 and values clamped to [0, 1].  Returns a dict, rows sorted
    by (frame, a, b): ``frame``, ``a``, ``b`` (a < b), ``links`` int64; ``sum`` int64, the sum over the links of
    ``rint(value * 2**32)`` (exact, independent of any order: identical from run to run); ``saddle`` float32, the smallest
    link value; ``mean`` float64 = ``sum / (links * 2**32)``, one IEEE division: the correctly rounded quotient when ``sum <
    2**53``; ``overflow`` int32 (B,): bit 1 (value 1) where the frame has more pairs than ``pair_cap`` (its rows are then
    incomplete), 2 where a label above ``cap`` was seen, 4 where a strength was NaN or outside [0, 1]; ``n_overflow``, the
    frames with bit 1 (read back with the row total, the one host read between the two calls).  ``pair_cap`` defaults to
    ``4 * cap`` -- a region adjacency graph is planar for ``conn`` = 4 and nearly so for 8: about 3 pairs per label -- and a
    slot takes 24 bytes: 96 ``cap`` bytes of table per frame."""
    st = _border_fill(labels, strength, conn, cap, pair_cap)
    _, n_over, r = _pair_rows(st, (("links", torch.int32, ()), ("sum", torch.int64, ()), ("saddle", torch.float32, ())),
                              lambda offsets, out, ws, nbytes: _call(
                                  "label_borders_write", st["pair_cap"], st["cap"], offsets, out["key"], out["frame"], out["links"],
                                  out["sum"], out["saddle"], st["B"], ws=(ws, nbytes)))
    a, b = _pair_ab(r["key"])
    links, total = r["links"].to(torch.int64), r["sum"]
    mean = total.to(torch.float64) / (links.to(torch.float64) * 4294967296.0)
    return {"frame": r["frame"], "a": a, "b": b, "links": links, "sum": total, "saddle": r["saddle"], "mean": mean,
            "overflow": st["overflow"], "n_overflow": n_over, "pair_cap": st["pair_cap"]}


def relabel_map(labels, label_map):
    """``label_map[b, labels[b]]`` (0 where a label lies outside 0 .. ``label_map.shape[1] - 1``): int32 (B, H, W)."""
    labels = _label_batch(labels)
    label_map = _req(label_map, torch.int32, 2)
    B, H, W = labels.shape
    if label_map.shape[0] != B or label_map.shape[1] < 2:
        raise ValueError("label_map must be (B, cap + 1)")
    out = torch.empty_like(labels)
    _call("relabel_map", labels, label_map, label_map.shape[1] - 1, out, B, H, W)
    return out


def merge_by_border(labels, strength, below, by="mean", conn=8, counts=None, cap=None, pair_cap=None):
    """Dissolve the weak borders of a label image (csrc/borders.hip, include/pcseg.h): the pairs of :func:`label_borders`
    with ``mean < below`` (``by`` = "mean": ``sum < rint(below * 2**32) * links`` in integers, strictly) or ``saddle <
    float32(below)`` (``by`` = "saddle") are joined, the groups are the connected components of the joined pairs over the
    labels 1 .. ``counts[b]`` (int32 (B,); default ``cap``) and are numbered 1 .. m in the order of their smallest member.
    One pass, as ``skimage.graph.cut_threshold``: weights are not updated after a union; a second call on the result is the
    exact second round.  Returns ``(merged, n_merged, map, flags)``: the merged image int32 (B, H, W) = ``map[b, labels]``,
    the groups per frame int32 (B,), ``map`` int32 (B, cap + 1) and ``flags`` int32 (B,) -- :func:`label_borders`'
    ``overflow`` bits, and 8 where the grouping met a corrupt parent entry.  A frame with bit 1 keeps the identity map: see
    :func:`check_border_flags`.  Fill, merge and relabel are enqueued one after the other: with ``cap`` given nothing is read
    back (the default reads the largest label once), and the call can be captured in a graph.  ``pair_cap``: as for
    :func:`label_borders`."""
    if by not in _BORDER_BY:
        raise ValueError('by must be "mean" or "saddle"')
    below = float(below)
    if not 0.0 <= below <= 1.0:
        raise ValueError("below must lie in [0, 1]")
    st = _border_fill(labels, strength, conn, cap, pair_cap, counts)
    B, cap, dev, counts = st["B"], st["cap"], st["labels"].device, st["counts"]
    label_map = torch.empty((B, cap + 1), dtype=torch.int32, device=dev)
    n_merged = torch.empty((B,), dtype=torch.int32, device=dev)
    _call("border_merge", st["pair_cap"], cap, counts, below, _BORDER_BY[by], st["overflow"], label_map, n_merged, B,
          ws=(st["ws"], st["nbytes"]))
    return relabel_map(st["labels"], label_map), n_merged, label_map, st["overflow"]


def check_border_flags(flags):
    """RuntimeError where a frame's merge is no result (``flags`` of :func:`merge_by_border`): its pair table was full (1), a
    label above the cap was dropped (2) or the grouping met a corrupt parent entry (8).  A clamped strength (4) is a defined
    reading and does not raise."""
    if flags is None:
        return
    bad = flags & (BORDER_TABLE_FULL | BORDER_ABOVE_CAP | BORDER_CORRUPT)
    if int((bad != 0).sum().item()):
        bad = bad.cpu()
        raise RuntimeError("the border merge of frame(s) %s is no result (flags %s: 1 = pair table full, raise pair_cap; 2 = a label "
                           "above cap; 8 = corrupt parent)" % ([int(b) for b in torch.nonzero(bad)[:, 0]], [int(v) for v in bad[bad != 0]]))


def refined_inputs(res, lp, rc, frame_ids, n_slots):
    """struct pcseg_refined_inputs of one batch: ``res`` (the pipeline's result), ``lp`` (:func:`label_parent` on it),
    ``rc`` (:func:`classify_regions` on the refined ROIs).  Returns (struct, tensors the pointers refer to)."""
    B, cap = res["stats"].shape[0], res["stats"].shape[1]
    ri = _lib.RefinedInputs()
    ri.B, ri.cap, ri.n_slots = B, cap, int(n_slots)
    keep = []
    ptr = functools.partial(_addr, keep, "refined")
    parent, parent_px, n_overlap, cls_r, overflow = lp[:5]
    ri.frame_ids = ptr(frame_ids, torch.int64, (B,))
    ri.counts = ptr(res["counts"], torch.int32, (B,))
    ri.kind = ptr(res["kind"], torch.uint8, (B, cap))
    ri.slot_of = ptr(res["slot_of"], torch.uint8, (B, cap))
    ri.cells = ptr(res["cells"], torch.int32, (B, cap))
    ri.n_markers = ptr(res["n_markers"], torch.int32, (B,))
    ri.ws_stats = ptr(res["ws_stats"], torch.int64, (B, cap, 8))
    ri.parent = ptr(parent, torch.int32, (B, cap))
    ri.parent_px = ptr(parent_px, torch.int32, (B, cap))
    ri.n_overlap = ptr(n_overlap, torch.int32, (B, cap))
    ri.cls_r = ptr(cls_r, torch.uint8, (B, cap))
    ri.kind_r = ptr(rc["kind"], torch.uint8, (B, cap))
    ri.slot_r = ptr(rc["slot_of"], torch.uint8, (B, cap))
    ri.cells_r = ptr(rc["cells"], torch.int32, (B, cap))
    ri.type_stats_r = ptr(rc["type_stats"], torch.int64, (B, 4, 4))
    ri.nan_flag_r = ptr(rc["nan_flag"], torch.int32, (B,))
    ri.parent_overflow = ptr(overflow, torch.int32, (B,))
    return ri, keep


def refined_tables(res, frame_ids, tables, table_ws, table_rows, check=False, points=False):
    """Goal 2 of refine_boundaries.py:1-12 for one batch whose dense tables :func:`build_tables` has just written
    (``table_ws``: its workspace, ``table_rows``: its (rois, cells) row counts): :func:`label_parent` of the refined
    ROIs, :func:`classify_regions` on them with their parent's class, then ``refined`` / ``cell_resolution`` /
    ``frames_refined`` (float64, see include/pcseg.h).  ``points``: also ``points`` = the refined rows of kind >= 1 as
    :class:`Points` for :func:`point_neighbours`.  ``check``: raise where a parent label exceeds cap."""
    B, cap = res["stats"].shape[0], res["stats"].shape[1]
    dev = res["stats"].device
    lp = label_parent(res["labels"], res["ws_labels"], res["n_markers"], cls_a=res["cls_out"], cap=cap, stats_r=res["ws_stats"])
    rc = classify_regions(res["ws_stats"], lp[3], res["n_markers"], tables)
    ri, keep = refined_inputs(res, lp, rc, frame_ids, len(tables.slot_names))
    ws = _workspace("refined_layout", dev, B, cap)
    totals = torch.empty((2,), dtype=torch.int64, device=dev)
    _call("refined_layout", ctypes.byref(ri), totals, ws=ws)
    n_pts, n_over = (int(v) for v in totals.cpu())
    if check and n_over:
        raise RuntimeError("refined ROI parent label above the region table capacity: raise FramePipeline(cap=...)")
    n_roi, n_cell = table_rows
    K = len(tables.slot_names)
    refined = torch.empty((n_roi + 1, 11), dtype=torch.float64, device=dev)
    resolution = torch.empty((n_cell + 1, 5), dtype=torch.float64, device=dev)
    frames = torch.empty((B, 2 + 5 * K), dtype=torch.float64, device=dev)
    pts = _alloc_points(n_pts, B, dev) if points else Points(None, None, None, None)
    _call("refined_table_write", ctypes.byref(ri), table_ws, table_ws.numel(), refined, resolution, frames, *pts, ws=ws)
    out = {"refined": refined[:n_roi], "cell_resolution": resolution[:n_cell], "frames_refined": frames,
           "parent_overflow": lp[4], "refined_nan_flag": rc["nan_flag"], "kind_r": rc["kind"], "slot_r": rc["slot_of"]}
    if points:
        out["points"] = _head(pts, n_pts)
    del keep
    return out


def point_neighbours(xy, slot, ids, frame_offsets, K, scale, edges=None):
    """Per-type nearest neighbours and pair-distance histograms, frame by frame (refine_boundaries.py:8-12, goal 3;
    csrc/neighbours.hip).  ``xy`` (n, 2) float64, ``slot`` (n,) int32 in 0..K-1, ``ids`` (n,) int32 and
    ``frame_offsets`` (B + 1,) int64 CUDA tensors, points of a frame contiguous.  Returns ``(dist, nn_id, pair_hist)``:
    (n, K) float64 distances ``sqrt(d2) / scale`` to the nearest OTHER point of each slot in the same frame (NaN: none),
    (n, K) int32 ids of those points (smallest id on ties, -1: none), and with ``edges`` (m + 1 increasing values from
    0) the (B, K (K + 1) / 2, m + 2) int64 histogram ``[n_pairs, bin_0 .. bin_m-1, over]`` of the unordered pairs of
    every slot pair ``a <= b`` (bin k: ``edges[k] <= d < edges[k + 1]``), else None."""
    xy = _req(xy, torch.float64, 2)
    slot = _req(slot, torch.int32, 1)
    ids = _req(ids, torch.int32, 1)
    frame_offsets = _req(frame_offsets, torch.int64, 1)
    n, B, K = xy.shape[0], frame_offsets.shape[0] - 1, int(K)
    if xy.shape[1] != 2 or slot.shape[0] != n or ids.shape[0] != n:
        raise ValueError("xy must be (n, 2) with n slots and ids")
    e, n_edges = _edges_arg(edges)
    dev = xy.device
    dist = torch.empty((n + 1, K), dtype=torch.float64, device=dev)  # (a spare row: never a null pointer)
    nn_id = torch.empty((n + 1, K), dtype=torch.int32, device=dev)
    P = K * (K + 1) // 2
    hist = None
    if e is not None:
        hist = torch.empty((max(B, 1), P, max(e.shape[0] + 1, 1)), dtype=torch.int64, device=dev)
    if B < 1:
        return dist[:n], nn_id[:n], (hist[:0] if hist is not None else None)
    _call("point_neighbours", xy, slot, ids, frame_offsets, n, B, K, float(scale), e, n_edges, dist, nn_id, hist,
          ws=(n, B, K, n_edges))
    return dist[:n], nn_id[:n], hist


MIXING_FIELDS = ("obs", "lo", "hi", "sum", "n_le", "n_ge", "cum_obs", "cum_lo", "cum_hi", "cum_sum", "cum_n_le", "cum_n_ge")


def mixing_tile():
    """The points of one LDS tile of :func:`pair_label_mixing`'s pair walk (larger frames: tile against tile)."""
    return int(_lib.load().pcseg_mixing_tile())  # (not through _call: what it returns is the answer, not a status)


def pair_label_mixing(xy, slot, frame_offsets, K, scale, edges, permutations, seed=0, frame_keys=None, counts=False):
    """Random-labelling envelopes of the pair-distance histograms of :func:`point_neighbours` (csrc/mixing.hip): the points
    stay where they are, the slots of a frame's typed points (``0 <= slot < K``) are shuffled ``permutations`` (P <= 65535)
    times by the counter-based rule of include/pcseg.h (``seed``, and per frame ``frame_keys``, (B,) int64, default 0 ..
    B - 1: a frame's result depends on its key, not on its place in the batch).  ``xy`` / ``slot`` / ``frame_offsets`` as
    for :func:`point_neighbours`, or ``xy`` a :class:`Points` and the other two None; ``edges`` m + 1 increasing values
    from 0.  Returns a dict of (B, Q, m) int64 CUDA tensors, Q = K (K + 1) / 2 slot pairs in (a <= b) order: ``obs`` (the
    histogram itself, without its n_pairs and overflow columns) and over the P shuffled histograms ``lo`` (minimum), ``hi``
    (maximum), ``sum``, ``n_le`` = #{p: N_p <= obs}, ``n_ge`` = #{p: N_p >= obs}; ``cum_*``: the same six of the counts
    summed over the bins 0 .. k (the K-function form).  With P = 0 only ``obs`` / ``cum_obs`` are meaningful (the rest 0).
    The one-sided Monte Carlo p-values are ``(1 + n_ge) / (1 + P)`` for attraction (more pairs than chance) and
    ``(1 + n_le) / (1 + P)`` for segregation.  ``counts=True``: also ``counts``, (B, P + 1, Q, m) int64, every labelling's
    histogram (p = 0 the observed one).  Exact integers, bit for bit reproducible."""
    if isinstance(xy, Points):
        if slot is not None or frame_offsets is not None:
            raise ValueError("with a Points as xy, slot and frame_offsets must be None")
        xy, slot, frame_offsets = xy.coords, xy.slot, xy.frame_offsets
    xy = _req(xy, torch.float64, 2)
    slot = _req(slot, torch.int32, 1)
    frame_offsets = _req(frame_offsets, torch.int64, 1)
    n, B, K, P = xy.shape[0], frame_offsets.shape[0] - 1, int(K), int(permutations)
    if xy.shape[1] != 2 or slot.shape[0] != n:
        raise ValueError("xy must be (n, 2) with n slots")
    e, n_edges = _edges_arg(edges)
    if e is None:
        raise ValueError("pair_label_mixing needs edges")
    dev = xy.device
    Q, m = K * (K + 1) // 2, max(n_edges - 1, 0)
    if frame_keys is None:
        frame_keys = torch.arange(max(B, 0), dtype=torch.int64, device=dev)
    frame_keys = _req(frame_keys, torch.int64, 1)
    if frame_keys.shape[0] != B:
        raise ValueError("frame_keys must have one entry per frame")
    if B < 1:
        out = {k: torch.zeros((0, Q, m), dtype=torch.int64, device=dev) for k in MIXING_FIELDS}
        if counts:
            out["counts"] = torch.zeros((0, max(P, 0) + 1, Q, m), dtype=torch.int64, device=dev)
        return out
    ws = _workspace("pair_label_mixing", dev, n, B, K, n_edges, P, 0 if counts else 1)
    env = torch.empty((len(MIXING_FIELDS), B, Q, m), dtype=torch.int64, device=dev)
    cnt = torch.empty((B, P + 1, Q, m), dtype=torch.int64, device=dev) if counts and ws[1] else None  # (0: a shape it refuses)
    spare = torch.empty((2,), dtype=torch.float64, device=dev)  # (an empty point set: never a null pointer)
    _call("pair_label_mixing", xy if n else spare, slot if n else spare, frame_offsets, frame_keys, n, B, K, float(scale), e, n_edges,
          P, int(seed) & 0xFFFFFFFFFFFFFFFF, cnt, env, ws=ws)
    out = dict(zip(MIXING_FIELDS, env))
    if counts:
        out["counts"] = cnt
    return out


def _edges_arg(edges):
    e = None if edges is None else np.ascontiguousarray(np.asarray(edges, dtype=np.float64).reshape(-1))  # checked by the library
    return e, (0 if e is None else int(e.shape[0]))


def surface_points(x, value_bits, want_points=True):
    """Surface of the mask ``(value_bits >> x) & 1`` of a (B, H, W) uint8 batch: its pixels with a 4-neighbour outside the
    mask, outside the image counting as outside (the point set of bwboundaries, .m:271-292; csrc/surface.hip).  Returns a
    dict: ``bits`` int32 (B, H, ceil(W / 32)) bit words (bit j of word w = column 32 w + j), ``counts`` int64 (B,),
    ``offsets`` int64 (B + 1,), ``area`` int64 (B,) = mask pixels per frame, ``shape`` and, with ``want_points`` (one
    host read of the total to size it), ``points`` int32 (n, 2) = (row, col) in raster order, frame by frame."""
    x = _req(x, torch.uint8, 3)
    B, H, W = x.shape
    dev = x.device
    out = {"bits": torch.empty((B, H, (W + 31) // 32), dtype=torch.int32, device=dev),
           "counts": torch.empty((B,), dtype=torch.int64, device=dev),
           "offsets": torch.empty((B + 1,), dtype=torch.int64, device=dev),
           "area": torch.empty((B,), dtype=torch.int64, device=dev), "shape": (B, H, W)}

    def call(points, cap, ws):
        return _call("surface_points", x, int(value_bits), out["bits"], out["counts"], out["offsets"], out["area"], points, cap,
                     B, H, W, ws=ws)

    ws = call(None, 0, (B, H, W))
    if want_points:
        n = int(out["offsets"][B].item())
        pts = torch.empty((n + 1, 2), dtype=torch.int32, device=dev)
        call(pts, n, ws)
        out["points"] = pts[:n]
    return out


def surface_distances(points_rc, frame_offsets, surface, scale, mask=None, slot=None, n_types=0, edges=None, rows_visited=False):
    """Distance of every query point to the surface of its frame (.m:271-309, without the script's (x, y) / (row, col)
    mix; csrc/surface.hip, an exact pruned search, one wave per query).  ``points_rc`` (n, 2) float64 (row, col),
    0-based, frame-contiguous, ``frame_offsets`` (B + 1,) int64, ``surface`` from :func:`surface_points`.  Returns
    ``(dist, nearest, inside, hist)``: (n,) float64 ``sqrt(min d2) / scale`` with d2 = drow*drow + dcol*dcol (each
    product and the sum rounded on their own), (n, 2) int32 surface pixel of minimal d2 (the smallest raster index on
    ties), (n,) uint8 ``mask`` at pixel (floor(row + 0.5), floor(col + 0.5)) (0 without ``mask``); NaN, -1, -1, 0 in a
    frame without surface.  With ``edges`` (m + 1 increasing values from 0; needs ``slot`` (n,) int32, ``n_types`` and
    ``mask``): ``hist`` int64 (B, 2, n_types, m + 2) = per frame, side (0 outside, 1 inside) and slot ``[n, bin_0 ..
    bin_m-1, over]``, else None.  ``rows_visited``: a fifth result, (n,) int32 image rows each search read."""
    rc = _req(points_rc, torch.float64, 2)
    foff = _req(frame_offsets, torch.int64, 1)
    B, H, W = surface["shape"]
    n = rc.shape[0]
    if rc.shape[1] != 2 or foff.shape[0] != B + 1:
        raise ValueError("points_rc must be (n, 2) and frame_offsets (B + 1,) for the surface's B frames")
    dev = rc.device
    if mask is not None:
        mask = _req(mask, torch.uint8, 3)
        if tuple(mask.shape) != (B, H, W):
            raise ValueError("mask must have the surface's shape")
    if slot is not None:
        slot = _req(slot, torch.int32, 1)
        if slot.shape[0] != n:
            raise ValueError("slot must be (n,)")
    e, n_edges = _edges_arg(edges)
    K = int(n_types)
    dist = torch.empty((n + 1,), dtype=torch.float64, device=dev)  # (a spare row: never a null pointer)
    nearest = torch.empty((n + 1, 2), dtype=torch.int32, device=dev)
    inside = torch.empty((n + 1,), dtype=torch.uint8, device=dev)
    hist = torch.empty((B, 2, max(K, 1), n_edges + 1), dtype=torch.int64, device=dev) if e is not None else None
    visited = torch.empty((n + 1,), dtype=torch.int32, device=dev) if rows_visited else None
    _call("surface_distances", rc, slot, foff, n, surface["bits"], surface["counts"], mask, B, H, W, float(scale), e, n_edges, K, dist,
          nearest, inside, hist, visited, ws=(B, H, W))
    out = (dist[:n], nearest[:n], inside[:n], hist)
    return out + (visited[:n],) if rows_visited else out


def surface_thresholds(edges, scale):
    """Host only: for every edge the smallest integer squared distance n with ``sqrt(n) / scale >= edge`` (numpy int64),
    so that ``searchsorted(edges, sqrt(D2) / scale, side="right") - 1 == searchsorted(thresholds, D2, side="right") - 1``."""
    e, n_edges = _edges_arg(edges)
    out = np.zeros(max(n_edges, 1), np.int64)
    _call("surface_thresholds", e, n_edges, float(scale), out)
    return out[:n_edges]


def surface_shells(surface, mask, edges, scale):
    """Pixels of every frame by their distance to the surface (the denominators of a colonisation profile, .m:271-309):
    int64 (B, 2, m + 2) = per frame and side (0 outside ``mask``, 1 inside) ``[n_px, bin_0 .. bin_m-1, over]``, bin k =
    ``edges[k] <= sqrt(D2) / scale < edges[k + 1]`` with D2 the exact squared distance to the nearest surface pixel;
    every pixel of a frame without surface is ``over``."""
    B, H, W = surface["shape"]
    mask = _req(mask, torch.uint8, 3)
    if tuple(mask.shape) != (B, H, W):
        raise ValueError("mask must have the surface's shape")
    e, n_edges = _edges_arg(edges)
    dev = mask.device
    shells = torch.empty((B, 2, n_edges + 1), dtype=torch.int64, device=dev)
    _call("surface_shells", surface["bits"], surface["counts"], mask, B, H, W, float(scale), e, n_edges, shells, ws=(B, H, W))
    return shells


def particle_mask(recreated, particle_value):
    """The surface mask of the tables: ``binary_fill_holes(recreated == particle_value)``, uint8 (B, H, W) (an empty mask
    without a particle class)."""
    recreated = _req(recreated, torch.uint8, 3)
    if particle_value is None:
        return torch.zeros_like(recreated)
    return fill_holes((recreated == int(particle_value)).view(torch.uint8))


def particle_surface(recreated, particle_value, mask=None):
    """:func:`particle_mask` (or ``mask``, if the caller has it already) and :func:`surface_points` of it (bit words only).
    Returns (mask uint8 (B, H, W), surface)."""
    if mask is None:
        mask = particle_mask(recreated, particle_value)
    return mask, surface_points(mask, 2, want_points=False)


def nearest_label(labels, sel=None, cap=None, want_site=False):
    """The exact nearest-label transform (Euclidean feature transform; csrc/voronoi.hip, include/pcseg.h): ``labels`` (B, H,
    W) int32 CUDA tensor of any width and alignment; a site is a pixel with a label in 1 .. ``cap`` (default: the width
    of ``sel``, else the largest label) that ``sel`` ((B, cap) uint8 / bool, optional) keeps.  Returns ``(d2, near, site)``,
    int32 (B, H, W): the squared distance to the nearest site, the SMALLEST label among the sites at that distance and,
    with ``want_site`` (else None), the raster index of the nearest site of that label (the smallest among equals) --
    ``scipy.ndimage.distance_transform_edt(labels == 0, return_indices=True)`` with the ties decided.  -1, 0, -1 in a frame
    without site.  Labels outside 1 .. cap are ignored."""
    labels = _label_batch(labels)
    B, H, W = labels.shape
    if sel is not None:
        sel = _req(sel, torch.uint8, 2)
        if cap is None:
            cap = sel.shape[1]
        if tuple(sel.shape) != (B, int(cap)):
            raise ValueError("sel must be (B, cap)")
    if cap is None:
        cap = _default_cap(labels)
    cap = int(cap)
    dev = labels.device
    d2 = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    near = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    site = torch.empty((B, H, W), dtype=torch.int32, device=dev) if want_site else None
    _call("nearest_label_i32", labels, sel, cap, d2, near, site, B, H, W, ws=(B, H, W))
    return d2, near, site


def _near_pair(near, d2):
    near, d2 = _label_batch(near, "near"), _label_batch(d2, "d2")
    if near.shape != d2.shape:
        raise ValueError("near and d2 must have one shape")
    return near, d2


def reach_r2(distance):
    """Host only: the largest integer n with ``np.sqrt(np.float64(n)) <= distance`` (a bisection over that very formula,
    which is non-decreasing in n); -1 = every n up to 2^53 (unbounded), None = none (``distance`` < 0 or NaN)."""
    ok = lambda n: bool(np.sqrt(np.float64(n)) <= distance)
    if not ok(0):
        return None
    lo, hi = 0, 1 << 53
    if ok(hi):
        return -1
    while hi - lo > 1:  # ok(lo) and not ok(hi)
        mid = (lo + hi) // 2
        if ok(mid):
            lo = mid
        else:
            hi = mid
    return lo


def reach_um_r2(reach, scale):
    """Host only: R2 of a reach in um at ``scale`` pixels per um, such that ``d2 <= R2`` iff ``sqrt(d2) / scale < reach``
    as numpy rounds it (:func:`surface_thresholds`); -1 (unbounded) for ``reach`` None."""
    if reach is None:
        return -1
    if not float(reach) > 0.0:
        raise ValueError("territory_reach must be a positive distance in um (None: unbounded)")
    t = int(surface_thresholds([0.0, float(reach)], scale)[1])
    return -1 if t >= (1 << 62) else t - 1


def territory_labels(near, d2, r2=-1):
    """``near`` where the pixel belongs to it (``0 <= d2 <= r2``; ``r2`` < 0: unbounded), else 0: int32, ``near``'s shape."""
    near, d2 = _near_pair(near, d2)
    out = torch.empty_like(near)
    _call("territory_labels", near, d2, int(r2), out, near.numel())
    return out


def expand_labels(labels, distance=1):
    """``skimage.segmentation.expand_labels(labels, distance)`` for an (H, W) or (B, H, W) int32 CUDA label image with labels
    >= 0: every background pixel within ``distance`` (``np.sqrt(d2) <= distance``) of a label takes the nearest one.  Where
    two labels are equally near -- skimage calls the choice undefined -- the smallest wins."""
    single = isinstance(labels, torch.Tensor) and labels.dim() == 2
    lab = _label_batch(labels[None] if single else labels)
    r2 = reach_r2(distance)
    if r2 is None:
        out = torch.zeros_like(lab)
    else:
        d2, near, _ = nearest_label(lab)
        out = territory_labels(near, d2, r2)
    return out[0] if single else out


TERRITORY_COLUMNS = ("territory_px", "territory_on_px", "reach2_max", "clipped")


def territory_reduce(near, d2, mask=None, r2=-1, cap=None):
    """The territory rows of :func:`nearest_label`'s result: int64 (B, cap, 4) in the order of ``TERRITORY_COLUMNS`` -- for
    label l (row l - 1) over the pixels with ``near == l`` and ``0 <= d2 <= r2`` (``r2`` < 0: unbounded) their count, the
    count of those on ``mask`` ((B, H, W) uint8 / bool, optional), the largest ``d2`` among them and whether one lies on
    the frame's outer row or column.  Zeros for a label that owns no pixel; ``near`` outside 1 .. ``cap`` (default: its
    maximum) is ignored."""
    near, d2 = _near_pair(near, d2)
    B, H, W = near.shape
    if mask is not None:
        mask = _req(mask, torch.uint8, 3)
        if tuple(mask.shape) != (B, H, W):
            raise ValueError("mask must have near's shape")
    if cap is None:
        cap = _default_cap(near)
    cap = int(cap)
    out = torch.empty((B, cap, 4), dtype=torch.int64, device=near.device)
    _call("territory_reduce", near, d2, mask, int(r2), cap, out, B, H, W)
    return out


def territory_pairs(near, d2, r2=-1, pair_cap=None, slot_of=None, n_types=0):
    """The adjacency graph of the territories of :func:`nearest_label`'s result.  A link is a pair of 4-neighbour pixels
    that belong (``0 <= d2 <= r2``) to different labels, counted once.  Returns a dict: ``frame`` int64 (n,) position in
    the batch, ``a`` / ``b`` int64 (n,) the labels (a < b), ``border`` / ``contact`` int64 (n,) the links between them and
    those with ``d2 == 0`` at both ends (the labels touch in the label image), rows sorted by (frame, a, b); ``overflow``
    int32 (B,) set where a frame has more than ``pair_cap`` pairs (default 8 x the largest label; its rows are then
    incomplete) and ``n_overflow``, their number (read back with the row total, the only host read).  With ``slot_of``
    ((B, cap) uint8, values >= ``n_types``: no type) also ``degree`` int32 (B, cap, 2 n_types): per label the number of
    distinct partners of every type slot, then of those with contact."""
    near, d2 = _near_pair(near, d2)
    B, H, W = near.shape
    dev = near.device
    degree, cap, K = None, 0, int(n_types)
    if slot_of is not None:  # (checked before anything is enqueued)
        slot_of = _req(slot_of, torch.uint8, 2)
        cap = slot_of.shape[1]
        if slot_of.shape[0] != B or not 1 <= K <= 4:
            raise ValueError("slot_of must be (B, cap), with 1 to 4 type slots")
    if pair_cap is None:
        pair_cap = 8 * (cap if slot_of is not None else _default_cap(near))
    pair_cap = int(pair_cap)
    st = _pair_fill("territory_pairs", (near, d2, int(r2), pair_cap), (B, H, W), dev, (B, pair_cap))
    if slot_of is not None:
        degree = torch.zeros((B, cap, 2 * K), dtype=torch.int32, device=dev)
    _, n_over, r = _pair_rows(st, (("counts", torch.int32, (2,)),), lambda offsets, out, ws, nbytes: _call(
        "territory_pairs_write", pair_cap, offsets, slot_of, cap, K, out["key"], out["frame"], out["counts"], degree, B,
        ws=(ws, nbytes)))
    a, b = _pair_ab(r["key"])
    counts = r["counts"].to(torch.int64)
    return {"frame": r["frame"], "a": a, "b": b, "border": counts[:, 0].contiguous(), "contact": counts[:, 1].contiguous(),
            "overflow": st["overflow"], "n_overflow": n_over, "degree": degree}


def territory_rows(labels, live, slot_of, frame_ids, scale, n_types, r2=-1, mask=None, check=False, pair_cap=None):
    """The ``territories`` and ``adjacency`` tables of one label batch whose sites are the labels ``live`` ((B, cap) bool):
    :func:`nearest_label`, :func:`territory_reduce` and :func:`territory_pairs` on the whole batch, then the rows ``live`` in
    (frame, label) order as ``[frame, label, slot, territory_px, territory_on_px, reach2_max, clipped, n_adj per type slot,
    n_contact per type slot, territory_um2, territory_on_um2]`` (areas / ``scale`` ^ 2, ONE correctly rounded division each)
    and the pairs as ``[frame, label_a, label_b, slot_a, slot_b, border_px, contact_px]`` sorted by (frame, a, b).  Returns
    (territories, adjacency, overflow int32 (B,)); ``check`` raises where a frame's pair table was full."""
    B, cap = live.shape
    K = max(int(n_types), 1)
    d2, near, _ = nearest_label(labels, live.view(torch.uint8) if live.dtype == torch.bool else live, cap)
    terr = territory_reduce(near, d2, mask, r2, cap)
    pairs = territory_pairs(near, d2, r2, pair_cap or 8 * cap, slot_of=slot_of, n_types=K)
    if check and pairs["n_overflow"]:
        raise RuntimeError("territory pair table capacity exceeded: raise FramePipeline(cap=...)")
    b, l, head = _row_head(live, slot_of, frame_ids)
    t = terr[b, l].to(torch.float64)
    deg = pairs["degree"][b, l].to(torch.float64)
    rows = torch.cat([torch.stack(head, dim=1), t, deg[:, :int(n_types)], deg[:, K:K + int(n_types)], _over(t[:, :2], scale * scale)],
                     dim=1)
    f, a, bb = pairs["frame"], pairs["a"], pairs["b"]
    inside = (a <= cap) & (bb <= cap)  # (every site label is: near only ever holds site labels)
    f, a, bb = f[inside], a[inside], bb[inside]
    adj = torch.stack([frame_ids[f].to(torch.float64), a.to(torch.float64), bb.to(torch.float64), _slot_column(slot_of, f, a - 1),
                       _slot_column(slot_of, f, bb - 1), pairs["border"][inside].to(torch.float64),
                       pairs["contact"][inside].to(torch.float64)], dim=1)
    return rows, adj, pairs["overflow"]


def remove_overlapping(dapi, other, threshold):
    """combine_cell_positions_and_clusters (tiff_analysis.py:252-287)."""
    dapi = _req(dapi, torch.uint8, 3)
    other = _req(other, torch.uint8, 3)
    if other.shape != dapi.shape:
        raise ValueError("dapi and other must have one shape")
    B, H, W = dapi.shape
    out = torch.empty_like(dapi)
    _call("remove_overlapping", dapi, other, float(threshold), out, B, H, W, ws=(B, H, W))
    return out


def otsu_hist(img):
    """256-bin histogram of each frame over its own [min, max] (north_star extension X1)."""
    img = _req(img, torch.float32, 3)
    B, H, W = img.shape
    hist = torch.zeros((B, 256), dtype=torch.int64, device=img.device)
    lohi = torch.zeros((B, 2), dtype=torch.float32, device=img.device)
    _call("otsu_hist_f32", img, hist, lohi, B, H, W)
    return hist, lohi


def morph3x3(mask, erode):
    """3x3 binary erosion / dilation (north_star extension X2)."""
    mask = _req(mask, torch.uint8, 3)
    B, H, W = mask.shape
    out = torch.empty_like(mask)
    _call("morph3x3", mask, out, int(bool(erode)), B, H, W)
    return out


def nearest_dist(a, b):
    """min over b of the Euclidean distance, for every row of a: (na,2), (nb,2) float64 CUDA tensors (.m:260-263)."""
    a = _req(a, torch.float64, 2)
    b = _req(b, torch.float64, 2)
    if a.shape[1] != 2 or b.shape[1] != 2:
        raise ValueError("a and b must be (n, 2)")
    out = torch.empty((a.shape[0],), dtype=torch.float64, device=a.device)
    if a.shape[0] == 0:
        return out
    if b.shape[0] == 0:
        return out.fill_(float("inf"))
    _call("nearest_dist_f64", a, a.shape[0], b, b.shape[0], out)
    return out


def threshold_otsu(img, return_hist=False):
    """skimage.filters.threshold_otsu per frame, entirely on the device (north_star extension X1; the library itself
    is the pin: tests/golden/extensions.npz): float64 (B,) CUDA tensor holding the float32 bin centre the
    library returns.  ``return_hist``: also the (B,256) histogram and the (B,2) [min, max] it was taken from."""
    img = _req(img, torch.float32, 3)
    B, H, W = img.shape
    thr = torch.empty((B,), dtype=torch.float64, device=img.device)
    hist = torch.empty((B, 256), dtype=torch.int64, device=img.device)
    lohi = torch.empty((B, 2), dtype=torch.float32, device=img.device)
    _call("otsu_f32", img, thr, hist, lohi, B, H, W)
    return (thr, hist, lohi) if return_hist else thr
