"""CPU checks of the per-ROI skeletons (csrc/skeleton.hip): the numpy RESTATEMENT of its definitions (include/pcseg.h) --
the two deletion tables from their predicates, the peel image, links, degrees, the integer table and the two float columns --
pinned to scikit-image 0.18.3's ``morphology.thin`` by tests/golden/skeleton.npz; the table schemas, the empty tables, the
gather's sort keys, the argument and workspace checks of the C entry points and the drop-in helper.
tests/test_gpu_skeleton.py and tests/golden/make_golden_skeleton.py import the restatement from here.

Every comparison is EQUALITY: thinning is a table look-up over eight neighbours, the table holds counts, ``length_px`` is one
correctly rounded product and one correctly rounded sum, ``width_px`` one correctly rounded division.

The restatement is deliberately not the device's algorithm: whole frames, one sub-iteration at a time, neighbour codes from
shifted copies of the padded image; no tiles, no halo, no bit words, no list of active tiles."""
import ctypes
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SKELETON = 65535
SKELETON_COLUMNS = ("skel_px", "n_orth", "n_diag", "n_end", "n_junction", "passes", "length_px", "width_px")
SKELETON_ROW = ["frame", "label", "slot", "skel_px", "n_orth", "n_diag", "n_end", "n_junction", "passes", "length_um", "width_um"]
# neighbour i of a pixel: E, NE, N, NW, W, SW, S, SE (scikit-image's mask [[8, 4, 2], [16, 0, 1], [32, 64, 128]])
OFFSETS = ((0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1))


# ---------------------------------------------------------------------------------------------------------------- restatement
def thin_tables():
    """(2, 256) bool: is an alive pixel with neighbour code N deleted by the first / the second sub-iteration"""
    out = np.zeros((2, 256), bool)
    for code in range(256):
        b = [(code >> i) & 1 for i in range(8)]
        g1 = sum(1 for i in (0, 2, 4, 6) if not b[i] and (b[(i + 1) % 8] or b[(i + 2) % 8])) == 1
        n1 = sum(1 for k in (1, 3, 5, 7) if b[k] or b[k - 1])
        n2 = sum(1 for k in (1, 3, 5, 7) if b[k] or b[(k + 1) % 8])
        g2 = min(n1, n2) in (2, 3)
        g3 = not ((b[1] or b[2] or not b[7]) and b[0])
        g3p = not ((b[5] or b[6] or not b[3]) and b[4])
        out[0, code] = g1 and g2 and g3
        out[1, code] = g1 and g2 and g3p
    return out


def _same(key):
    """(8, H, W) bool: neighbour i lies in the frame and carries the pixel's own positive key"""
    H, W = key.shape
    p = np.zeros((H + 2, W + 2), key.dtype)
    p[1:-1, 1:-1] = key
    return np.stack([(p[1 + dr:1 + dr + H, 1 + dc:1 + dc + W] == key) & (key > 0) for dr, dc in OFFSETS])


def peel_image(lab, max_iter=None):
    """(peel uint16 (H, W), iters): 0 background, 65535 survives, else the 1-based sub-iteration that deleted the pixel;
    iters = the full iterations that deleted a pixel"""
    lab = np.asarray(lab).astype(np.int64)
    tables = thin_tables()
    weights = (1 << np.arange(8))[:, None, None]
    alive = lab > 0
    peel = np.where(alive, SKELETON, 0).astype(np.uint16)
    s = iters = 0
    while max_iter is None or iters < max_iter:
        any_deleted = False
        for second in (0, 1):
            s += 1
            code = (_same(np.where(alive, lab, 0)) * weights).sum(axis=0)
            gone = alive & tables[second][code]
            if gone.any():
                peel[gone] = s
                alive &= ~gone
                any_deleted = True
        if not any_deleted:
            break
        iters += 1
    return peel, iters


def pixel_links(lab, peel):
    """(orth (H, W), diag (H, W)): a skeleton pixel's orthogonal / diagonal links (to all sides)"""
    key = np.where(np.asarray(peel) == SKELETON, np.asarray(lab).astype(np.int64), 0)
    e, ne, n, nw, w, sw, s, se = _same(key)
    diag = (ne & ~(n | e)).astype(np.int64) + (nw & ~(n | w)) + (sw & ~(s | w)) + (se & ~(s | e))
    return e.astype(np.int64) + n + w + s, diag


def skeleton_table(lab, peel, n=None):
    """int64 (n, 6): skel_px, n_orth, n_diag, n_end, n_junction, passes per label 1..n; zeros for a label without pixel"""
    lab = np.asarray(lab).astype(np.int64)
    peel = np.asarray(peel).astype(np.int64)
    n = int(lab.max(initial=0)) if n is None else n
    orth, diag = pixel_links(lab, peel)
    deg = orth + diag
    on = (peel == SKELETON) & (lab > 0)
    sel = lambda m: np.where(m & (lab >= 1) & (lab <= n), lab, 0).ravel()
    count = lambda m, wgt=None: np.bincount(sel(m), weights=None if wgt is None else wgt.ravel(), minlength=n + 1)[1:n + 1]
    out = np.zeros((n, 6), np.int64)
    out[:, 0] = count(on)
    out[:, 1] = np.rint(count(on, orth.astype(np.float64))).astype(np.int64) // 2  # every link has two ends
    out[:, 2] = np.rint(count(on, diag.astype(np.float64))).astype(np.int64) // 2
    out[:, 3] = count(on & (deg == 1))
    out[:, 4] = count(on & (deg >= 3))
    gone = (lab > 0) & (peel != SKELETON)
    full = (peel + 1) // 2
    for l in np.unique(lab[gone & (lab <= n)]):
        out[l - 1, 5] = full[gone & (lab == l)].max()
    return out


def skeleton_properties(area, table):
    """float64 (n, 2): length_px, width_px; NaN rows for labels without pixel"""
    area, table = np.asarray(area, np.int64), np.asarray(table, np.int64)
    out = np.full((len(area), 2), np.nan)
    live = area > 0
    with np.errstate(divide="ignore"):
        length = table[live, 1].astype(np.float64) + table[live, 2].astype(np.float64) * np.sqrt(2.0)
        out[live, 0] = length
        out[live, 1] = area[live].astype(np.float64) / length
    return out


def areas(lab, n=None):
    lab = np.asarray(lab).astype(np.int64)
    n = int(lab.max(initial=0)) if n is None else n
    return np.bincount(np.where((lab >= 1) & (lab <= n), lab, 0).ravel(), minlength=n + 1)[1:n + 1].astype(np.int64)


def load_fixture():
    """tests/golden/skeleton.npz (+ the label images of shape.npz it refers to) -> (scikit-image's two tables (2, 256) bool,
    [(name, label image int32, skeleton bool, full-iteration image int64 -- 0 where nothing was deleted --, iters)])"""
    z = np.load(os.path.join(HERE, "golden", "skeleton.npz"), allow_pickle=False)
    s = np.load(os.path.join(HERE, "golden", "shape.npz"), allow_pickle=False)
    shape_names = [str(x) for x in s["names"]]
    out = []
    for i, name in enumerate(str(x) for x in z["names"]):
        lab = z["lab_%02d" % i] if "lab_%02d" % i in z.files else s["lab_%02d" % shape_names.index(name)]
        H, W = lab.shape
        skel = np.unpackbits(z["skel_%02d" % i])[:H * W].reshape(H, W).astype(bool)
        out.append((name, lab.astype(np.int32), skel, z["full_%02d" % i].astype(np.int64), int(z["iters"][i])))
    return np.stack([z["lut_first"], z["lut_second"]]).astype(bool), out


# ---------------------------------------------------------------------------------------------------------------------- tests
HAND_MADE = ("thin_bar_w1", "thin_bar_w2", "thin_bar_w3", "thin_L", "thin_T", "thin_ring", "thin_block_2x2", "thin_plus",
             "thin_touching_bent", "thin_on_edge_and_corner", "thin_full_9x13", "thin_square_41_in_48", "thin_disk_20_in_48")


def test_tables_equal_skimage():
    lut, _ = load_fixture()
    t = thin_tables()
    np.testing.assert_array_equal(t, lut)
    assert t[0].sum() > 20 and t[1].sum() > 20 and not t[:, 0].any() and not t[:, 255].any()
    assert (t[0] != t[1]).any()


def test_restatement_equals_skimage_on_every_fixture_image():
    _, cases = load_fixture()
    names = [c[0] for c in cases]
    shape_names = [str(x) for x in np.load(os.path.join(HERE, "golden", "shape.npz"), allow_pickle=False)["names"]]
    assert names == shape_names + list(HAND_MADE)
    for name, lab, skel, full, iters in cases:
        peel, it = peel_image(lab)
        np.testing.assert_array_equal(peel == SKELETON, skel, err_msg=name)
        gone = (lab > 0) & ~skel
        np.testing.assert_array_equal(((peel.astype(np.int64) + 1) // 2)[gone], full[gone], err_msg=name)
        assert (full[~gone] == 0).all() and (peel[lab <= 0] == 0).all() and it == iters, name
    by = {c[0]: c for c in cases}
    assert by["thin_full_9x13"][2].sum() == 5 and by["thin_square_41_in_48"][4] == 20 and by["thin_disk_20_in_48"][4] == 20
    assert by["thin_bar_w1"][4] == 0 and (by["thin_bar_w1"][2] == (by["thin_bar_w1"][1] > 0)).all()
    assert len({l for l in np.unique(by["thin_touching_bent"][1]) if l > 0}) == 2


def test_max_iter_stops_the_restatement_where_skimage_stops():
    _, cases = load_fixture()
    by = {c[0]: c for c in cases}
    for name in ("thin_square_41_in_48", "func_96x80_s5/denoised"):
        _, lab, skel, full, iters = by[name]
        for k in (1, 2):
            peel, it = peel_image(lab, max_iter=k)
            # thin(..., max_iter=k) keeps what the first k full iterations did not delete
            np.testing.assert_array_equal(peel == SKELETON, (lab > 0) & ((full == 0) | (full > k)), err_msg=name)
            assert it == min(k, iters) and peel[peel != SKELETON].max() <= 2 * k


def test_restatement_on_hand_checked_shapes():
    line = np.zeros((5, 9), np.int32)
    line[2, 1:8] = 3
    peel, it = peel_image(line)
    assert it == 0 and (peel[line > 0] == SKELETON).all()
    t = skeleton_table(line, peel)
    assert t[2].tolist() == [7, 6, 0, 2, 0, 0] and not t[:2].any()
    p = skeleton_properties(areas(line), t)
    assert p[2].tolist() == [6.0, 7.0 / 6.0] and np.isnan(p[:2]).all()
    corner = np.zeros((4, 4), np.int32)  # an L-corner of three pixels: two links, not three -- no loop
    corner[1, 1] = corner[1, 2] = corner[2, 2] = 1
    t = skeleton_table(corner, np.where(corner > 0, SKELETON, 0))
    assert t[0].tolist() == [3, 2, 0, 2, 0, 0]
    diag = np.zeros((4, 4), np.int32)
    diag[0, 0] = diag[1, 1] = diag[2, 2] = 1
    t = skeleton_table(diag, np.where(diag > 0, SKELETON, 0))
    assert t[0].tolist() == [3, 0, 2, 2, 0, 0]
    assert skeleton_properties([3], t)[0, 0] == 2.0 * math.sqrt(2.0)
    two = diag.copy()
    two[1, 1] = 2  # another label between them: no link across it
    t = skeleton_table(two, np.where(two > 0, SKELETON, 0))
    assert t.tolist() == [[2, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0]]
    assert skeleton_properties([2, 1], t)[1].tolist() == [0.0, math.inf]  # a one-pixel skeleton
    plus = np.zeros((7, 7), np.int32)
    plus[3, 1:6] = plus[1:6, 3] = 1
    t = skeleton_table(plus, np.where(plus > 0, SKELETON, 0))
    assert t[0].tolist() == [9, 8, 0, 4, 1, 0]
    square = np.zeros((8, 8), np.int32)
    square[1:7, 1:7] = 1
    peel, it = peel_image(square)
    t = skeleton_table(square, peel)
    assert it == t[0, 5] and t[0, 5] >= 2 and t[0, 0] == (peel == SKELETON).sum()
    cut = skeleton_table(square, peel, n=0)
    assert cut.shape == (0, 6)


def _pipe(ct=None):
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    return FramePipeline(ct)


def test_table_columns_with_skeleton():
    import pytest
    pytest.importorskip("torch")
    from particle_col_image_segmentation_amd import ops
    from particle_col_image_segmentation_amd.pipeline import OPTIONAL_TABLES, TableSwitches
    pipe = _pipe()
    assert TableSwitches().skeleton is False
    assert TableSwitches._fields.index("skeleton") == TableSwitches._fields.index("territory_reach") + 1
    assert ops.SKELETON_COLUMNS == SKELETON_COLUMNS
    names = [t.name for t in OPTIONAL_TABLES]
    at = names.index("skeletons")
    assert names[at - 1] == "refined_adjacency" and names[at:at + 3] == ["skeletons", "refined_skeletons", "convexity"]
    base = pipe.table_columns(5)
    assert "skeletons" not in base and "refined_skeletons" not in base
    cols = pipe.table_columns(5, skeleton=True)
    assert set(cols) == set(base) | {"skeletons"} and cols["skeletons"] == SKELETON_ROW
    assert {k: v for k, v in cols.items() if k != "skeletons"} == base
    cols = pipe.table_columns(5, skeleton=True, refined=True)
    ref = pipe.table_columns(5, refined=True)
    assert set(cols) == set(ref) | {"skeletons", "refined_skeletons"} and cols["refined_skeletons"] == SKELETON_ROW
    every = dict(neighbours=True, pair_edges=[0.0, 1.0], refined=True, surface=True, surface_edges=[0.0, 1.0], shape=True, convex=True,
                 territory=True, territory_reach=3.0)
    with_all, without = pipe.table_columns(5, skeleton=True, **every), pipe.table_columns(5, **every)
    assert {k: v for k, v in with_all.items() if k not in ("skeletons", "refined_skeletons")} == without
    assert [k for k in with_all if k not in ("skeletons", "refined_skeletons")] == list(without)
    keys = list(with_all)
    assert keys.index("refined_skeletons") + 1 == keys.index("convexity")


def test_empty_and_host_tables_carry_the_skeleton_tables():
    import pytest
    torch = pytest.importorskip("torch")
    pipe = _pipe()
    dt = pipe.empty_device_tables(5, device="cpu", skeleton=True, refined=True)
    assert dt["skeletons"].shape == (0, 11) and dt["refined_skeletons"].shape == (0, 11)
    assert "refined_skeletons" not in pipe.empty_device_tables(5, device="cpu", skeleton=True)
    assert set(pipe.empty_device_tables(5, device="cpu")) == {"rois", "cells", "groups", "frames_rec", "distances"}
    cols = pipe.table_columns(5, skeleton=True)
    z = lambda k, n: torch.zeros((n, len(cols[k])), dtype=torch.float64)
    base = {"rois": z("rois", 0), "cells": z("cells", 2), "groups": z("groups", 0),
            "frames_rec": torch.zeros((1, 18), dtype=torch.float64), "distances": torch.zeros((0, 3), dtype=torch.float64)}
    rows = torch.arange(22.0, dtype=torch.float64).reshape(2, 11)
    out = pipe.host_tables({**base, "skeletons": rows}, 5, skeleton=True)
    np.testing.assert_array_equal(out["skeletons"], rows.numpy())
    assert out["skeletons_columns"] == SKELETON_ROW
    with pytest.raises(ValueError, match="skeletons"):
        pipe.host_tables(base, 5, skeleton=True)
    assert "skeletons" not in pipe.host_tables(base, 5)


def test_sort_keys_and_sharded_keywords_of_the_skeleton_tables():
    import pytest
    pytest.importorskip("torch")
    from particle_col_image_segmentation_amd.distributed import _SORT_COLS
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    assert _SORT_COLS["skeletons"] == (0, 1) and _SORT_COLS["refined_skeletons"] == (0, 1)
    for method in ("tables_device", "host_tables", "empty_device_tables"):
        assert FramePipeline.table_kwargs(method, {"skeleton": True, "refined": True}) == {"skeleton": True, "refined": True}


def test_every_table_method_takes_the_same_switches():
    """the five table methods take the fields of TableSwitches and nothing else, and with every switch on the three that
    work without a device name the same tables"""
    import pytest
    torch = pytest.importorskip("torch")
    from particle_col_image_segmentation_amd.pipeline import OPTIONAL_TABLES, TableSwitches
    pipe = _pipe()
    res = {"shape": (1, 5, 8, 8)}  # (never read: the switches are looked at first)
    for call in (lambda **kw: pipe.table_columns(5, **kw), lambda **kw: pipe.empty_device_tables(5, device="cpu", **kw),
                 lambda **kw: pipe.host_tables({}, 5, **kw), lambda **kw: pipe.tables_device(res, **kw),
                 lambda **kw: pipe.tables(res, **kw)):
        with pytest.raises(TypeError, match="skeletons"):
            call(skeletons=True)
        with pytest.raises(TypeError, match="no_such_table"):
            call(refined=True, no_such_table=1)
    kw = dict(neighbours=True, pair_edges=[0.0, 1.0, 2.0], mixing=19, mixing_seed=3, refined=True, surface=True,
              surface_edges=[0.0, 1.0], territory=True, territory_reach=3.0, skeleton=True, convex=True, shape=True)
    assert set(kw) == set(TableSwitches._fields)
    cols = pipe.table_columns(5, **kw)
    always = {"rois", "cells", "groups", "frames", "distances"}
    assert set(cols) == always | {t.name for t in OPTIONAL_TABLES}
    dt = pipe.empty_device_tables(5, device="cpu", **kw)
    assert set(dt) == (set(cols) - {"frames"}) | {"frames_rec"}
    assert all(dt[k].shape == (0, len(cols[k])) for k in dt if k != "frames_rec")
    host = pipe.host_tables(dt, 5, **kw)
    assert {k for k in host if not k.endswith("_columns")} == set(cols)
    assert all(host[k + "_columns"] == cols[k] and host[k].shape == (0, len(cols[k])) for k in cols)


def test_skeleton_arguments_and_workspace():
    """argument checks and the workspace carve of the entry points, before any device call (the pointers are never
    dereferenced): one byte less than the size query's answer is refused"""
    from particle_col_image_segmentation_amd import _lib, build
    build.build()
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    null = ctypes.c_void_p(0)
    B, H, W, cap = 2, 96, 83, 16
    f = lib.pcseg_thin_labels_workspace_bytes
    need = f(B, H, W)
    # two copies of the alive bits, a link byte per pixel, two words per tile
    assert need % 256 == 0 and B * H * (W + 2 * 4 * 3) <= need < B * H * W * 2 + 8 * 256
    assert f(0, 8, 8) == 0 and f(1, 0, 8) == 0 and f(1, 8, 0) == 0 and f(-1, 8, 8) == 0
    assert f(64, 1024, 1024) < 100 << 20
    rc = lib.pcseg_thin_labels(p, p, p, B, H, W, -1, p, need - 1, None)
    assert rc == -3 and b"workspace too small" in lib.pcseg_last_error(), (rc, lib.pcseg_last_error())
    ok = [p, p, p, B, H, W, -1, p, need, None]
    for pos, bad in ((0, null), (1, null), (2, null), (3, 0), (3, -1), (3, 65536), (4, 0), (4, -2), (5, 0), (7, null)):
        args = list(ok)
        args[pos] = bad
        assert lib.pcseg_thin_labels(*args) == -1 and b"bad arguments" in lib.pcseg_last_error(), pos
    g = lib.pcseg_region_skeleton_workspace_bytes
    need = g(B, H, W, cap)
    assert need > 0 and need % 256 == 0
    assert g(0, 8, 8, 4) == 0 and g(1, 0, 8, 4) == 0 and g(1, 8, 0, 4) == 0 and g(1, 8, 8, 0) == 0
    rc = lib.pcseg_region_skeleton(p, p, p, p, B, H, W, cap, p, need - 1, None)
    assert rc == -3 and b"workspace too small" in lib.pcseg_last_error(), (rc, lib.pcseg_last_error())
    ok = [p, p, p, p, B, H, W, cap, p, need, None]
    for pos, bad in ((0, null), (1, null), (2, null), (3, null), (4, 0), (4, 65536), (5, 0), (6, -1), (7, 0), (8, null)):
        args = list(ok)
        args[pos] = bad
        assert lib.pcseg_region_skeleton(*args) == -1 and b"bad arguments" in lib.pcseg_last_error(), pos
    for bad in ((null, p, p, p, B, cap, None), (p, null, p, p, B, cap, None), (p, p, null, p, B, cap, None), (p, p, p, null, B, cap, None),
                (p, p, p, p, 0, cap, None), (p, p, p, p, 65536, cap, None), (p, p, p, p, B, 0, None)):
        assert lib.pcseg_skeleton_properties(*bad) == -1 and lib.pcseg_last_error()
    for name in ("pcseg_thin_labels_workspace_bytes", "pcseg_thin_labels", "pcseg_region_skeleton_workspace_bytes",
                 "pcseg_region_skeleton", "pcseg_skeleton_properties"):
        assert name in _lib.SIGNATURES


def test_get_cell_skeletons_reads_the_shared_holder():
    """without a device: the helper asks the regions' holder (pre-filled, as if the one device call had happened); a region
    without a holder raises with the wording of the shape attributes"""
    import pytest
    pytest.importorskip("torch")
    from particle_col_image_segmentation_amd import tiff_analysis as ta
    holder = ta._LabelImage(None, stats=object(), n=3)
    s2 = math.sqrt(2.0)
    holder._skeleton = np.array([[7.0, 6.0, 0.0, 2.0, 0.0, 0.0, 6.0, 7.0 / 6.0], [3.0, 0.0, 2.0, 2.0, 0.0, 3.0, 2.0 * s2, 20.0 / (2.0 * s2)],
                                 [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, math.inf]])
    row = [4, 6, 6, 1, 1, 3, 3, 9]
    regs = {"a": [ta.Region(3, row, 8, holder), ta.Region(1, row, 8, holder)], "b": [ta.Region(2, row, 8, holder)], "c": []}
    got = ta.get_cell_skeletons(regs, px_to_um=2.0)
    assert list(got) == ["a", "b", "c"]
    assert set(got["a"]) == {"labels", "skel_px", "n_orth", "n_diag", "n_end", "n_junction", "passes", "length_um", "width_um"}
    assert got["a"]["labels"].tolist() == [3, 1] and got["a"]["skel_px"].tolist() == [1.0, 7.0]
    assert got["a"]["length_um"].tolist() == [0.0, 3.0] and got["a"]["width_um"].tolist() == [math.inf, 7.0 / 6.0 / 2.0]
    assert got["b"]["n_diag"].tolist() == [2.0] and got["b"]["passes"].tolist() == [3.0] and got["b"]["length_um"].tolist() == [s2]
    assert got["c"]["labels"].shape == (0,) and got["c"]["width_um"].shape == (0,)
    assert ta.get_cell_skeletons(regs)["a"]["length_um"][1] == 6.0 / ta.PX_TO_UM_CONV
    with pytest.raises(AttributeError, match="carries no label image"):
        ta.get_cell_skeletons({"a": [ta.Region(1, row, 8, None)]})
    with pytest.raises(AttributeError, match="carries no label image"):
        ta._LabelImage(None).skeleton_columns
