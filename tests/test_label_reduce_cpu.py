"""The banded label images of tests/test_gpu_label_reduce.py and their numpy expectations, checked here WITHOUT a device
against the oracle's region_table: the inputs are ones the reference itself handles, and the restatements the GPU test
compares with (test_shape_cpu.shape_table / region_table, test_gpu_refined_cells.np_label_parent) agree with it on them.

The images aim at what the other inputs of the per-label reductions (csrc/label_reduce.h) do not reach: labels that collide
in the 256-slot table of a block, and columns that end many runs inside one 32-row block."""
import functools

import numpy as np

SHAPES = [(2, 64, 64), (2, 45, 67), (1, 5, 1030), (2, 33, 70)]
NEUTRAL = np.iinfo(np.int64).max


@functools.lru_cache(maxsize=None)
def banded(B, H, W):
    """(B, H, W) int32, read-only.  Bands 2 rows high (a column ends 16 runs per 32-row block); band k carries the labels
    1 + 256 (k % 3) + (c // 8) % 5, so l, l + 256 and l + 512 meet in one block and one slot, and runs of 8 equal columns
    span the 4-column lanes; band 1 is ONE label over the full width (a whole wave is one segment); about 10 % of the pixels
    are zeroed."""
    k = (np.arange(H) // 2)[:, None]
    c = np.arange(W)[None, :]
    one = 1 + 256 * (k % 3) + (c // 8) % 5
    one = np.where(k == 1, 257, one)
    rng = np.random.default_rng(1000 * H + W)
    lab = np.where(rng.random((B, H, W)) < 0.1, 0, np.broadcast_to(one, (B, H, W))).astype(np.int32)
    lab.setflags(write=False)
    return lab


def shifted(lab):
    """the same bands one row down and three columns to the right (zeros move in)"""
    out = np.zeros_like(lab)
    out[:, 1:, 3:] = lab[:, :-1, :-3]
    return out


def np_region_rows(lab, n):
    """int64 (n, 8) rows of the labels 1 .. n of ONE frame by np.add.at / np.minimum.at / np.maximum.at; a label that is
    absent keeps the neutral row: 0, 0, 0, H, W, 0, 0, INT64_MAX"""
    H, W = lab.shape
    r, c = np.indices(lab.shape)
    keep = (lab > 0) & (lab <= n)
    l, r, c = lab[keep].astype(np.int64), r[keep].astype(np.int64), c[keep].astype(np.int64)
    out = np.zeros((n + 1, 8), np.int64)
    out[:, 3], out[:, 4], out[:, 7] = H, W, NEUTRAL
    np.add.at(out[:, 0], l, 1)
    np.add.at(out[:, 1], l, r)
    np.add.at(out[:, 2], l, c)
    np.minimum.at(out[:, 3], l, r)
    np.minimum.at(out[:, 4], l, c)
    np.maximum.at(out[:, 5], l, r + 1)
    np.maximum.at(out[:, 6], l, c + 1)
    np.minimum.at(out[:, 7], l, r * W + c)
    return out[1:]


def class_bits_mask(cls, bits):
    """the pixels whose class byte v is selected: v < 64 and bit v of ``bits`` set"""
    return (cls < 64) & (((np.uint64(bits) >> np.minimum(cls, 63).astype(np.uint64)) & np.uint64(1)) == 1)


def np_plane_sums(lab, planes, n, cls=None, bits=0):
    """float64 (n, C): per label the sum of every float32 plane, accumulated in float64; with ``bits`` != 0 only over the
    pixels whose class byte in ``cls`` is selected (a label without such a pixel keeps 0)"""
    keep = (lab > 0) & (lab <= n)
    if bits:
        keep &= class_bits_mask(cls, bits)
    out = np.zeros((n + 1, planes.shape[0]), np.float64)
    for k, p in enumerate(planes):
        np.add.at(out[:, k], lab[keep], p[keep].astype(np.float64))
    return out[1:]


def test_banded_images_are_what_the_docstring_says():
    for B, H, W in SHAPES:
        lab = banded(B, H, W)
        assert lab.shape == (B, H, W) and lab.max() == 517 and 0.05 < (lab == 0).mean() < 0.15
        present = set(np.unique(lab).tolist())
        assert {1, 257, 513} <= present  # one slot, three labels, one block
        live = lab[0][:, 0][lab[0][:, 0] > 0]
        if H >= 32:
            assert (np.diff(lab[0][:32, 0]) != 0).sum() >= 15  # runs a column ends inside the first block
        assert set(lab[:, 2:4].ravel().tolist()) <= {0, 257} and len(live)


def test_class_selected_plane_sums_against_a_plain_loop():
    lab = banded(2, 33, 70)[0]
    n = int(lab.max())
    rng = np.random.default_rng(5)
    cls = rng.integers(0, 6, lab.shape).astype(np.uint8)
    cls[0, :4] = (63, 64, 200, 255)  # bit 63 is a class, bytes of 64 and above never are
    planes = (rng.random((3, 33, 70)) * 100).astype(np.float32)
    bits = (1 << 1) | (1 << 4) | (1 << 63)
    want = np.zeros((n, 3), np.float64)
    for r in range(33):
        for c in range(70):
            l, v = int(lab[r, c]), int(cls[r, c])
            if l > 0 and v < 64 and (bits >> v) & 1:
                for k in range(3):
                    want[l - 1, k] += float(planes[k, r, c])
    np.testing.assert_array_equal(np_plane_sums(lab, planes, n, cls, bits), want)
    assert class_bits_mask(cls[0, :4], bits).tolist() == [True, False, False, False]
    # no selection: every pixel, the class map is not looked at
    np.testing.assert_array_equal(np_plane_sums(lab, planes, n, cls, 0), np_plane_sums(lab, planes, n))
    assert (np_plane_sums(lab, planes, n, cls, 1 << 7) == 0).all()  # a class no pixel has


def test_expectations_and_restatements_agree_with_the_oracle_region_table():
    from oracle import oracle as orc
    from test_gpu_refined_cells import np_label_parent
    from test_shape_cpu import region_table, shape_table
    R = banded(2, 64, 64)
    A = shifted(R)
    n = int(R.max())
    parent, px, nov, _, over = np_label_parent(R, R, [n, n], n)  # every ROI against itself
    for b in range(2):
        tab = orc.region_table(R[b], n)
        live = tab[:, 0] > 0
        rows = np_region_rows(R[b], n)
        np.testing.assert_array_equal(rows[live], tab[live])
        assert (rows[~live] == [0, 0, 0, 64, 64, 0, 0, NEUTRAL]).all() and (~live).sum() == n - 15
        np.testing.assert_array_equal(region_table(R[b], n)[live], tab[live])
        sh = shape_table(R[b], n)
        # a band is 2 rows high: every pixel of a label has a 4-neighbour of another label -> n_border is the area
        np.testing.assert_array_equal(sh[:, 6], tab[:, 0])
        assert (sh[~live] == 0).all() and (sh[live, 0] >= tab[live, 1] ** 2 // tab[live, 0]).all()  # sum r^2 >= (sum r)^2 / A
        np.testing.assert_array_equal(px[b], tab[:, 0])
        np.testing.assert_array_equal(parent[b], np.where(live, np.arange(1, n + 1), 0))
        np.testing.assert_array_equal(nov[b], live.astype(np.int64))
    assert over.tolist() == [0, 0]
    # against the shifted image: an ROI's overlaps are part of its area, over fewer than the sixteen candidate slots
    parent, px, nov, _, _ = np_label_parent(A, R, [n, n], n)
    for b in range(2):
        area = orc.region_table(R[b], n)[:, 0]
        assert (px[b] <= area).all() and (px[b][area > 0] > 0).all() and nov[b].max() >= 2
    # the plane sums of a plane of ones are the areas
    ones = np.ones((1, 64, 64), np.float32)
    np.testing.assert_array_equal(np_plane_sums(R[0], ones, n)[:, 0], orc.region_table(R[0], n)[:, 0].astype(np.float64))
    np.testing.assert_array_equal(orc.channel_sums(R[0], ones, n), np_plane_sums(R[0], ones, n))
