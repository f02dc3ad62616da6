"""CPU checks of the per-ROI shape table (csrc/shape.hip): the numpy / exact-rational RESTATEMENT of its definitions
(include/pcseg.h), pinned to scikit-image 0.18.3 by tests/golden/shape.npz for every fixture region; the table schemas, the
empty tables, the gather's sort keys and the workspace carve of the C entry point.  tests/test_gpu_shape.py and
tests/golden/make_golden_shape.py import the restatement from here.

The bound (derived, not tuned), with eps = 2^-52 and TOL = 64 eps = 1.4e-14:
  * relative TOL for the well-conditioned columns: the tensor entries relative to the largest of them, l1, the major axis,
    the equivalent diameter, the extent and the perimeter (each a handful of float64 roundings of exact integers);
  * TOL * l1 ABSOLUTE on l2: the backward error of any float64 evaluation of a symmetric 2 x 2 eigenproblem in about ten
    roundings -- l2 = ((P + Q) - root) / 2 cancels, nothing relative can be promised for it;
  * the minor axis and the eccentricity through the values that bound implies: minor^2 / 16 against l2 (within TOL * l1)
    and 1 - eccentricity^2 against l2 / l1 (within TOL);
  * the orientation as an AXIS (modulo pi: on a symmetric region the library lands on +pi/2 where the formula gives -pi/2):
    theta = atan2(y, x) / 2 with x = c - a, y = -2 b moves by at most (|dx| + |dy|) / (2 D), D = hypot(x, y); the tensor
    bound gives |dx|, |dy| <= 2 TOL T (T the largest entry), so |d theta| <= 2 TOL T / D + 8 eps; nothing when D == 0.
    The formula is DISCONTINUOUS on a == c: its a - c == 0 branch returns -pi/4 for b < 0, the limit of its other branch is
    +pi/4 -- the perpendicular axis.  An evaluation whose a - c is not exactly 0 where the integers say it is (scikit-image
    centres its moments in floating point: 13 of the 2 300 fixture regions) lands on the other branch, inside the tensor
    bound.  So where |c - a| <= 2 TOL T both branches count as right: the comparison there is modulo pi/2.  (The device
    forms a and c from the same exact integers and takes the formula's own branch; the GPU test asserts that exactly.)
Measured for func_256_s9/class_map (659 regions, areas 1 - 37 069), scikit-image against the exact evaluation: perimeter
2.5e-16 relative, tensor 4.8e-16 of its largest entry, eigenvalues 6.3e-16 l1, major axis 3.8e-16, eccentricity 2.2e-15
absolute, minor axis 5.7e-14 absolute."""
import ctypes
import math
import os
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.0 ** -52
TOL = 64 * EPS
COLUMNS = ("a", "b", "c", "l1", "l2", "major", "minor", "eccentricity", "orientation", "equivalent_diameter", "extent", "perimeter")
SHAPE_ROW = ["frame", "label", "slot", "n_border", "n_1", "n_sqrt2", "n_mid", "mu_rr", "mu_rc", "mu_cc", "major_um", "minor_um",
             "eccentricity", "orientation", "equivalent_diameter_um", "extent", "perimeter_um"]
# fixture regions on which scikit-image ITSELF leaves the bound: (image name, label, column) -> reason.  None is needed.
REFERENCE_OUTSIDE_BOUND = {}


# ---------------------------------------------------------------------------------------------------------------- restatement
def _bincount(lab, weights, n):
    tot = np.bincount(lab.ravel(), weights=None if weights is None else weights.ravel().astype(np.float64), minlength=n + 1)
    assert tot.max(initial=0) < 2.0 ** 53  # (integer sums below 2^53: float64 accumulation is exact)
    return tot[1:n + 1].astype(np.int64)


def region_table(lab, n=None):
    """int64 (n, 8) region rows of a 2-D label image: area, sum r, sum c, bbox (half open), first raster index."""
    lab = np.asarray(lab).astype(np.int64)
    n = int(lab.max(initial=0)) if n is None else n
    H, W = lab.shape
    r, c = np.indices(lab.shape)
    pos = np.where((lab > 0) & (lab <= n), lab, 0)
    out = np.zeros((n, 8), np.int64)
    out[:, 0], out[:, 1], out[:, 2] = _bincount(pos, None, n), _bincount(pos, r, n), _bincount(pos, c, n)
    big = np.iinfo(np.int64).max
    for col, src, red, init in ((3, r, np.minimum, H), (4, c, np.minimum, W), (5, r + 1, np.maximum, 0), (6, c + 1, np.maximum, 0),
                                (7, r * W + c, np.minimum, big)):
        acc = np.full(n + 1, init, np.int64)
        red.at(acc, pos.ravel(), src.ravel())
        out[:, col] = acc[1:]
    return out


def shape_table(lab, n=None):
    """int64 (n, 8): sum r^2, sum r c, sum c^2, n_1, n_sqrt2, n_mid, n_border, 0 per label 1..n (include/pcseg.h)."""
    lab = np.asarray(lab).astype(np.int64)
    n = int(lab.max(initial=0)) if n is None else n
    H, W = lab.shape
    r, c = np.indices(lab.shape)
    pos = np.where((lab > 0) & (lab <= n), lab, 0)
    out = np.zeros((n, 8), np.int64)
    out[:, 0], out[:, 1], out[:, 2] = _bincount(pos, r * r, n), _bincount(pos, r * c, n), _bincount(pos, c * c, n)
    pad = np.full((H + 2, W + 2), -1, np.int64)  # outside the image: never a label
    pad[1:-1, 1:-1] = lab
    win = lambda a, dr, dc: a[1 + dr:1 + dr + H, 1 + dc:1 + dc + W]
    four, diag = ((-1, 0), (1, 0), (0, -1), (0, 1)), ((-1, -1), (-1, 1), (1, -1), (1, 1))
    border = (lab > 0) & np.logical_or.reduce([win(pad, dr, dc) != lab for dr, dc in four])
    bpad = np.zeros((H + 2, W + 2), bool)
    bpad[1:-1, 1:-1] = border
    same = lambda dr, dc: (win(bpad, dr, dc) & (win(pad, dr, dc) == lab)).astype(np.int64)
    v = 1 + 2 * sum(same(dr, dc) for dr, dc in four) + 10 * sum(same(dr, dc) for dr, dc in diag)
    bl = np.where(border, pos, 0)
    for col, values in ((3, (5, 7, 15, 17, 25, 27)), (4, (21, 33)), (5, (13, 23))):
        out[:, col] = _bincount(np.where(np.isin(v, values), bl, 0), None, n)
    out[:, 6] = _bincount(bl, None, n)
    return out


def exact_properties(stats, shape):
    """float64 (n, 12) in COLUMNS order from the integer tables: rationals up to the square roots and the arc tangent;
    l2 as det / l1 (no cancellation).  NaN rows for labels without pixel."""
    out = np.full((len(stats), 12), np.nan)
    for i, (st, sh) in enumerate(zip(np.asarray(stats).tolist(), np.asarray(shape).tolist())):
        A, sr, sc = st[0], st[1], st[2]
        if A <= 0:
            continue
        P, Q, R = Fraction(A * sh[0] - sr * sr, A * A), Fraction(A * sh[2] - sc * sc, A * A), Fraction(A * sh[1] - sr * sc, A * A)
        root = math.sqrt((P - Q) ** 2 + 4 * R * R)
        l1 = (float(P + Q) + root) / 2
        l2 = max(float(P * Q - R * R) / l1, 0.0) if l1 > 0 else 0.0
        if Q - P == 0:
            theta = -math.pi / 4 if -R < 0 else math.pi / 4
        else:
            theta = 0.5 * math.atan2(float(2 * R), float(P - Q))
        out[i] = (float(Q), float(-R), float(P), l1, l2, 4 * math.sqrt(l1), 4 * math.sqrt(l2),
                  0.0 if l1 == 0 else math.sqrt(max(1 - l2 / l1, 0.0)), theta, math.sqrt(4 * A / math.pi),
                  A / ((st[5] - st[3]) * (st[6] - st[4])),
                  sh[3] + sh[4] * math.sqrt(2) + sh[5] * (1 + math.sqrt(2)) / 2)
    return out


def deviation(got, exact):
    """(n, 12) deviations of ``got`` from ``exact`` IN UNITS OF THE BOUND of the module docstring (<= 1: inside)."""
    got, exact = np.asarray(got, np.float64), np.asarray(exact, np.float64)
    dev = np.zeros(got.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        T = np.abs(exact[:, :3]).max(axis=1)
        l1 = exact[:, 3]
        rel = lambda k: np.where(exact[:, k] == 0, np.where(got[:, k] == 0, 0.0, np.inf), np.abs(got[:, k] - exact[:, k]) / (TOL * np.abs(exact[:, k])))
        for k in range(3):
            dev[:, k] = np.where(T == 0, np.where(got[:, k] == 0, 0.0, np.inf), np.abs(got[:, k] - exact[:, k]) / (TOL * T))
        for k in (3, 5, 9, 10, 11):
            dev[:, k] = rel(k)
        zero_l1 = lambda x, want0: np.where(l1 == 0, np.where(want0, 0.0, np.inf), x)
        dev[:, 4] = zero_l1(np.abs(got[:, 4] - exact[:, 4]) / (TOL * l1), got[:, 4] == 0)
        dev[:, 6] = zero_l1(np.abs(got[:, 6] ** 2 / 16 - exact[:, 4]) / (TOL * l1), got[:, 6] == 0)
        dev[:, 7] = zero_l1(np.abs((1 - got[:, 7] ** 2) - exact[:, 4] / l1) / TOL, got[:, 7] == 0)
        D = np.hypot(exact[:, 2] - exact[:, 0], 2 * exact[:, 1])
        d = np.abs(got[:, 8] - exact[:, 8]) % math.pi
        d = np.minimum(d, math.pi - d)
        q = d % (math.pi / 2)
        d = np.where(np.abs(exact[:, 2] - exact[:, 0]) <= 2 * TOL * T, np.minimum(q, math.pi / 2 - q), d)  # either branch at a == c
        dev[:, 8] = np.where(D == 0, 0.0, d / (2 * TOL * T / D + 8 * EPS))
    return dev


def load_fixture():
    """tests/golden/shape.npz -> [(name, label image int32, skimage values (n, 12), skimage central moments (n, 3))]."""
    z = np.load(os.path.join(HERE, "golden", "shape.npz"), allow_pickle=False)
    return [(str(name), z["lab_%02d" % i].astype(np.int32), z["val_%02d" % i], z["mu_%02d" % i]) for i, name in enumerate(z["names"])]


# ---------------------------------------------------------------------------------------------------------------------- tests
def test_restatement_matches_skimage_on_every_fixture_region():
    cases = load_fixture()
    names = [c[0] for c in cases]
    for want in ("single_pixel", "line_h", "line_v", "line_diag", "block_2x2", "ring", "on_border", "in_corner", "interleaved",
                 "full_frame", "frame_97x83"):
        assert want in names
    assert sum(n.endswith("/class_map") for n in names) == 7 and sum(n.endswith("/denoised") for n in names) == 7
    assert sum(n.endswith("/watershed") for n in names) >= 3
    assert set(k[0] for k in REFERENCE_OUTSIDE_BOUND) <= set(names)
    worst = np.zeros(12)
    for name, lab, val, mu in cases:
        n = int(lab.max())
        stats, shape = region_table(lab, n), shape_table(lab, n)
        live = stats[:, 0] > 0
        assert live.sum() == len(val), name  # scikit-image lists the labels that own a pixel, in label order
        ex = exact_properties(stats[live], shape[live])
        # the stored central moments are the integer sums themselves: mu20 = A P, mu11 = A R, mu02 = A Q
        A = stats[live, 0].astype(np.float64)
        for k, col in ((0, 2), (1, 1), (2, 0)):
            want = A * ex[:, col] * (-1.0 if k == 1 else 1.0)
            assert (np.abs(mu[:, k] - want) <= TOL * A * np.abs(ex[:, :3]).max(axis=1)).all(), (name, k)
        dev = deviation(val, ex)
        labels = np.nonzero(live)[0] + 1
        listed = [(i, k) for i in range(len(val)) for k in range(12) if (name, int(labels[i]), COLUMNS[k]) in REFERENCE_OUTSIDE_BOUND]
        assert len(set(i for i, _ in listed)) <= 0.01 * len(val), name
        for i, k in listed:
            dev[i, k] = 0.0
        print("%-28s %5d regions, worst deviation / bound per column: %s" % (name, len(val), np.array2string(dev.max(axis=0, initial=0), precision=3)))
        bad = np.argwhere(~(dev <= 1.0))
        assert len(bad) == 0, (name, [(int(labels[i]), COLUMNS[k], val[i, k], ex[i, k]) for i, k in bad[:5]])
        worst = np.maximum(worst, dev.max(axis=0, initial=0))
    print("worst over the fixture:", worst)


def test_restatement_on_hand_checked_shapes():
    one = np.zeros((5, 7), np.int32)
    one[2, 3] = 1
    assert shape_table(one).tolist() == [[4, 6, 9, 0, 0, 0, 1, 0]]  # v = 1: on the border, in no weight class
    ex = exact_properties(region_table(one), shape_table(one))[0]
    assert ex[:8].tolist() == [0.0] * 8 and ex[8] == math.pi / 4 and ex[10] == 1.0 and ex[11] == 0.0
    line = np.zeros((3, 9), np.int32)
    line[1, 2:7] = 1
    sh = shape_table(line)[0]
    assert sh[3:7].tolist() == [3, 0, 0, 5]  # the three inner pixels have v = 5, the two ends v = 3: in no weight class
    ex = exact_properties(region_table(line), shape_table(line))[0]
    assert ex[0] == 2.0 and ex[1] == 0.0 and ex[2] == 0.0 and ex[3] == 2.0 and ex[4] == 0.0 and ex[7] == 1.0
    assert abs(ex[8]) == math.pi / 2 and ex[11] == 3.0
    two = np.array([[1, 2, 1, 2], [2, 1, 2, 1], [1, 2, 1, 2]], np.int32)  # neighbours of the OTHER label never count
    sh = shape_table(two)
    # every pixel is on its label's border; of its own label it only ever sees diagonal neighbours: v = 11, 21 or 41
    assert sh[:, 3:7].tolist() == [[0, 3, 0, 6], [0, 3, 0, 6]]


def _pipe(ct=None):
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    return FramePipeline(ct)


def test_table_columns_with_shape():
    import pytest
    pytest.importorskip("torch")
    from particle_col_image_segmentation_amd.pipeline import OPTIONAL_TABLES, TableSwitches
    pipe = _pipe()
    assert TableSwitches._fields[-1] == "shape" and TableSwitches().shape is False
    base = pipe.table_columns(5)
    assert "shapes" not in base and "refined_shapes" not in base
    cols = pipe.table_columns(5, shape=True)
    assert set(cols) == set(base) | {"shapes"} and cols["shapes"] == SHAPE_ROW
    assert {k: v for k, v in cols.items() if k != "shapes"} == base
    cols = pipe.table_columns(5, shape=True, refined=True)
    ref = pipe.table_columns(5, refined=True)
    assert set(cols) == set(ref) | {"shapes", "refined_shapes"} and cols["refined_shapes"] == SHAPE_ROW
    assert {k: v for k, v in cols.items() if k not in ("shapes", "refined_shapes")} == ref
    assert [t.name for t in OPTIONAL_TABLES][-2:] == ["shapes", "refined_shapes"]
    every = dict(neighbours=True, pair_edges=[0.0, 1.0], refined=True, surface=True, surface_edges=[0.0, 1.0])
    with_all, without = pipe.table_columns(5, shape=True, **every), pipe.table_columns(5, **every)
    assert {k: v for k, v in with_all.items() if k not in ("shapes", "refined_shapes")} == without
    assert list(without) == list(with_all)[:len(without)]


def test_empty_and_host_tables_carry_the_shape_tables():
    import pytest
    torch = pytest.importorskip("torch")
    pipe = _pipe()
    dt = pipe.empty_device_tables(5, device="cpu", shape=True, refined=True)
    assert dt["shapes"].shape == (0, 17) and dt["refined_shapes"].shape == (0, 17)
    assert "refined_shapes" not in pipe.empty_device_tables(5, device="cpu", shape=True)
    assert set(pipe.empty_device_tables(5, device="cpu")) == {"rois", "cells", "groups", "frames_rec", "distances"}
    cols = pipe.table_columns(5, shape=True)
    z = lambda k, n: torch.zeros((n, len(cols[k])), dtype=torch.float64)
    base = {"rois": z("rois", 0), "cells": z("cells", 2), "groups": z("groups", 0),
            "frames_rec": torch.zeros((1, 18), dtype=torch.float64), "distances": torch.zeros((0, 3), dtype=torch.float64)}
    rows = torch.arange(34.0, dtype=torch.float64).reshape(2, 17)
    out = pipe.host_tables({**base, "shapes": rows}, 5, shape=True)
    np.testing.assert_array_equal(out["shapes"], rows.numpy())
    assert out["shapes_columns"] == SHAPE_ROW
    with pytest.raises(ValueError, match="shapes"):
        pipe.host_tables(base, 5, shape=True)
    assert "shapes" not in pipe.host_tables(base, 5)


def test_sort_keys_and_sharded_keywords_of_the_shape_tables():
    import pytest
    pytest.importorskip("torch")
    from particle_col_image_segmentation_amd.distributed import _SORT_COLS
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    assert _SORT_COLS["shapes"] == (0, 1) and _SORT_COLS["refined_shapes"] == (0, 1)
    for method in ("tables_device", "host_tables", "empty_device_tables"):
        assert FramePipeline.table_kwargs(method, {"shape": True, "refined": True}) == {"shape": True, "refined": True}


def test_region_shape_workspace_is_what_the_entry_point_carves():
    """one byte less than the size query's answer is refused before any device call (the pointers are never dereferenced)"""
    from particle_col_image_segmentation_amd import _lib, build
    build.build()
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    B, H, W, cap = 2, 96, 83, 16
    need = lib.pcseg_region_shape_workspace_bytes(B, H, W)
    assert need > 0 and need % 256 == 0
    assert "pcseg_region_shape" in _lib.SIGNATURES and "pcseg_shape_properties" in _lib.SIGNATURES
    rc = lib.pcseg_region_shape(p, p, p, p, B, H, W, cap, p, need - 1, None)
    assert rc == -3 and b"workspace too small" in lib.pcseg_last_error(), (rc, lib.pcseg_last_error())
    f = lib.pcseg_region_shape_workspace_bytes
    assert f(0, 8, 8) == 0 and f(1, 0, 8) == 0 and f(1, 8, 0) == 0
    null = ctypes.c_void_p(0)
    for bad in ((null, p, p, p, B, H, W, cap, p, need, None), (p, null, p, p, B, H, W, cap, p, need, None),
                (p, p, null, p, B, H, W, cap, p, need, None), (p, p, p, p, B, H, W, 0, p, need, None),
                (p, p, p, p, 0, H, W, cap, p, need, None), (p, p, p, p, B, H, W, cap, null, need, None)):
        assert lib.pcseg_region_shape(*bad) == -1 and lib.pcseg_last_error()
    for bad in ((null, p, p, p, B, cap, None), (p, null, p, p, B, cap, None), (p, p, null, p, B, cap, None), (p, p, p, null, B, cap, None),
                (p, p, p, p, 0, cap, None), (p, p, p, p, B, 0, None)):
        assert lib.pcseg_shape_properties(*bad) == -1 and lib.pcseg_last_error()


def test_region_attributes_are_lazy_and_others_still_raise():
    """without a device: a Region built from a table row has the nine names as class attributes, asks its holder only on
    access, and keeps raising AttributeError for anything else"""
    import pytest
    pytest.importorskip("torch")
    from particle_col_image_segmentation_amd.tiff_analysis import Region, _LabelImage
    holder = _LabelImage(None, stats=object(), n=2)
    holder._shape = np.arange(24.0).reshape(2, 12)  # as if the one device call had happened
    reg = Region(2, [4, 6, 6, 1, 1, 3, 3, 9], 8, holder)
    assert reg.major_axis_length == 17.0 and reg["perimeter"] == 23.0 and reg.orientation == 20.0 and reg.extent == 22.0
    assert reg.inertia_tensor.tolist() == [[12.0, 13.0], [13.0, 14.0]] and list(reg.inertia_tensor_eigvals) == [15.0, 16.0]
    assert reg.minor_axis_length == 18.0 and reg.eccentricity == 19.0 and reg.equivalent_diameter == 21.0
    for other in ("solidity", "convex_area", "euler_number", "feret_diameter_max", "moments_hu"):
        with pytest.raises(AttributeError):
            getattr(reg, other)
    with pytest.raises(AttributeError):
        Region(1, [4, 6, 6, 1, 1, 3, 3, 9], 8, None).perimeter
