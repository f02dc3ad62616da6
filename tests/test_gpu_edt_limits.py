"""The distance-transform family (csrc/edt.hip) on the device at the limits of its contract: squared distances of 2^30 and
more, the widths at which an LDS stage changes or ends, fill_particle over its radii, thresholds and labels, caps, class
bytes of 64 and more, non-finite thresholds.  Inputs and expectations: tests/edt_limit_cases.py, held against the oracle by
tests/test_edt_limits_cpu.py.  Every comparison is ``==``; a configuration the library refuses is asserted by its message."""
import numpy as np
import pytest

import edt_limit_cases as ec

torch = pytest.importorskip("torch")
from device_helpers import shifted  # noqa: E402  (needs torch)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")
    from particle_col_image_segmentation_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (np.array: a writable copy -- the shared expectations are read-only)


def same(got, want, what, names=None):
    """``got`` (device) == ``want`` (numpy), compared on the device; a failure names the first frame that differs, how many
    pixels do, the first of them, and how many of them lie where the expectation is 2^30 or more"""
    exp = dev(want)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, tuple(got.shape), exp.dtype, tuple(exp.shape))
    if torch.equal(got, exp):
        return
    g = got.cpu().numpy()
    if g.ndim == 1:
        pytest.fail("%s: got %s, expected %s" % (what, g, want))
    bad = [b for b in range(g.shape[0]) if (g[b] != want[b]).any()]
    b = bad[0]
    diff = g[b] != want[b]
    r, c = (int(v[0]) for v in np.nonzero(diff))
    pytest.fail("%s: %d of %d frames differ, first %s: %d pixels (%d of them where %d or more is expected), first at (%d, %d): "
                "got %d, expected %d" % (what, len(bad), g.shape[0], names[b] if names else b, diff.sum(),
                                         (diff & (want[b] >= ec.TWO_30)).sum(), ec.TWO_30, r, c, g[b][r, c], want[b][r, c]))


# ================================================================================================ A: distances of 2^30 and more
@pytest.mark.parametrize("names", ec.A_BATCHES, ids="+".join)
@pytest.mark.parametrize("shape", ec.A_SHAPES, ids=lambda s: "%dx%d" % s)
def test_distances_of_2_30_and_more(ops, shape, names):
    """edt_sq (exact, cap = 50, cap = 2^30), edt_sq_lt and nearest_label where the far corner lies 2^30 and more from the
    nearest zero pixel: a "no zero pixel" sentinel of 2^30 in the row search reported those pixels as 0"""
    mask = np.stack([ec.a_mask(shape, k) for k in names])
    d2 = np.stack([ec.a_expected(shape, k) for k in names])
    x = dev(mask)
    what = "%s %s: " % (shape, "+".join(names))
    same(ops.edt_sq(x), d2, what + "edt_sq", names)
    for cap in ec.A_CAPS:
        same(ops.edt_sq(x, cap=cap), ec.capped(d2, cap), what + "edt_sq cap=%d" % cap, names)
    img = torch.where(x != 0, 0.25, 0.75).to(torch.float32).contiguous()  # its < 0.5 set is the mask
    d2_lt, mask_lt = ops.edt_sq_lt(img, 0.5)
    del img
    same(d2_lt, d2, what + "edt_sq_lt", names)
    same(mask_lt, mask, what + "edt_sq_lt mask", names)
    del d2_lt, mask_lt
    # the nearest-label transform measures to the same targets when its sites are the zero pixels: label 1 on each
    vd2 = ops.nearest_label((x == 0).to(torch.int32), cap=1)[0]
    for b, k in enumerate(names):
        if k == "ones":  # no site: its own empty-frame rule
            assert bool((vd2[b] == -1).all()), what + "nearest_label d2 of the frame without a site"
        else:
            same(vd2[b:b + 1], d2[b:b + 1], what + "nearest_label d2", [k])


# ======================================================================================= B: width limits of the LDS stages
def test_row_block_pass_at_its_widest(ops):
    """dilate_disk radius 32 and fill_particle (20, 33) -- a reach of 32, the row-block pass -- at the largest width whose
    staged rows fit the LDS beside the kernel's own share, nine rows: a second row block with a single row"""
    W = ec.REACH_MAX_W
    x = dev(ec.b_class_frames(W))
    p, cell, overlap = ec.B_FILL
    r = ec.B_DILATE_REACH["row blocks"]
    same(ops.dilate_disk(x, 1 << p, r), ec.b_dilate_expected(W, r), "dilate_disk r=%d W=%d" % (r, W))
    pair = ec.B_FILL_REACH["row blocks"]
    out, area = ops.fill_particle(x, p, cell, overlap, *pair)
    want_out, want_area = ec.b_fill_expected(W, *pair)
    same(out, want_out, "fill_particle %s W=%d" % (pair, W))
    same(area, want_area, "fill_particle %s W=%d area" % (pair, W))


@pytest.mark.parametrize("W", ec.B_REFUSED_W)
def test_row_block_pass_refuses_wider_frames(ops, W):
    """one column more than fits, and a width that the guard admitted while it counted the staged rows alone: refused by
    message, nothing launched"""
    from particle_col_image_segmentation_amd._lib import PcsegError
    x = dev(ec.b_class_frames(6828)[:, :, :W])
    p, cell, overlap = ec.B_FILL
    with pytest.raises(PcsegError, match="too wide"):
        ops.dilate_disk(x, 1 << p, ec.B_DILATE_REACH["row blocks"])
    with pytest.raises(PcsegError, match="too wide"):
        ops.fill_particle(x, p, cell, overlap, *ec.B_FILL_REACH["row blocks"])


@pytest.mark.parametrize("W", ec.B_BIT_W)
def test_bit_word_pass_has_no_width_bound(ops, W):
    """dilate_disk radius 31 and fill_particle (20, 2) -- reaches of at most 31, the bit-word pass -- at widths the row-block
    pass refuses: 6828 (W % 4 == 0) and 12001 (ragged)"""
    x = dev(ec.b_class_frames(W))
    p, cell, overlap = ec.B_FILL
    r = ec.B_DILATE_REACH["bit words"]
    same(ops.dilate_disk(x, 1 << p, r), ec.b_dilate_expected(W, r), "dilate_disk r=%d W=%d" % (r, W))
    pair = ec.B_FILL_REACH["bit words"]
    out, area = ops.fill_particle(x, p, cell, overlap, *pair)
    want_out, want_area = ec.b_fill_expected(W, *pair)
    same(out, want_out, "fill_particle %s W=%d" % (pair, W))
    same(area, want_area, "fill_particle %s W=%d area" % (pair, W))


@pytest.mark.parametrize("W", ec.B_ROW_W)
def test_row_search_either_side_of_its_block_switch(ops, W):
    """edt_sq, exact and capped, at the last width with four staged rows per block (they fill the LDS exactly) and the
    first with one"""
    x = dev(ec.b_row_masks(W))
    d2 = ec.b_row_expected(W)
    names = ("sparse", "zero in column 0")
    same(ops.edt_sq(x), d2, "edt_sq W=%d" % W, names)
    same(ops.edt_sq(x, cap=ec.EDT_CAP), ec.capped(d2, ec.EDT_CAP), "edt_sq cap=%d W=%d" % (ec.EDT_CAP, W), names)


# ================================================================================================ C: fill_particle's parameters
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "one byte past"])
@pytest.mark.parametrize("shape", ec.C_SHAPES, ids=lambda s: "%dx%d" % s)
def test_fill_particle_over_its_parameters(ops, shape, aligned):
    """every (radius, threshold) pair with the default labels and every label triple at two pairs, four frames a call (a
    disk, single pixels at the seams and corners, no particle, a particle in the last column), from a 16-byte aligned base
    and from one byte past it: thresholds above the radius (R2 not a square), reaches of 31 and 32 either side of the
    switch between the two threshold kernels, labels with bit 7 set, cell == overlap, cell == particle"""
    place = (lambda t: t) if aligned else shifted
    for triple, pair in ec.c_cases():
        x = place(dev(ec.c_frames(shape, triple)))
        assert (x.data_ptr() % 16 == 0) == aligned
        out, area = ops.fill_particle(x, *triple, *pair)
        want_out, want_area = ec.c_expected(shape, triple, pair)
        what = "fill_particle %s labels %s (radius, threshold) %s" % (shape, triple, pair)
        same(out, want_out, what, ec.C_FRAMES)
        same(area, want_area, what + " area")


def test_fill_particle_adds_to_a_preset_area(ops):
    shape, triple, pair = ec.C_SHAPES[0], ec.C_DEFAULT, (2, 5)
    area = dev(ec.C_PRESET_AREA)
    out, got = ops.fill_particle(dev(ec.c_frames(shape, triple)), *triple, *pair, overlap_area=area)
    want_out, want_area = ec.c_expected(shape, triple, pair)
    assert got is area and want_area[0] > 0
    same(out, want_out, "fill_particle with a preset area", ec.C_FRAMES)
    same(area, ec.C_PRESET_AREA + want_area, "preset area + overlap area")


@pytest.mark.parametrize("pair", ec.C_REFUSED_PAIRS)
def test_fill_particle_refuses_radii_above_180(ops, pair):
    from particle_col_image_segmentation_amd._lib import PcsegError
    with pytest.raises(PcsegError, match="out of range"):
        ops.fill_particle(dev(ec.c_frames(ec.C_SHAPES[1], ec.C_DEFAULT)), *ec.C_DEFAULT, *pair)


# ================================================================================== D: caps, class bytes, non-finite thresholds
@pytest.mark.parametrize("shape", ec.D_CAP_SHAPES, ids=lambda s: "%dx%d" % s)
def test_edt_sq_caps(ops, shape):
    """cap = 0, perfect squares and their neighbours, a cap float32 cannot hold, 2^30, and the two largest: a distance above
    the cap comes back as cap + 1, one at or below it exactly (at 2^31 - 1 nothing exceeds it)"""
    x = dev(ec.d_cap_masks(shape))
    d2 = ec.d_cap_d2(shape)
    for cap in ec.D_CAPS:
        same(ops.edt_sq(x, cap=cap), ec.capped(d2, cap), "edt_sq %s cap=%d" % (shape, cap), ec.D_CAP_FRAMES)
    same(ops.edt_sq(x), d2, "edt_sq %s" % (shape,), ec.D_CAP_FRAMES)


@pytest.mark.parametrize("radius", ec.D_RADII)
def test_dilate_disk_value_bits_and_bytes_of_64_and_more(ops, radius):
    """only a byte below 64 is looked up in value_bits: 64 + v, 128 + v and 255 are never members, bit 63 is byte 63 alone,
    and the empty set dilates to the empty set -- on the bit words (radius 2) and on staged row blocks (radius 32)"""
    x = dev(ec.d_class_bytes())
    for bits in ec.D_VALUE_BITS:
        same(ops.dilate_disk(x, bits, radius), ec.d_dilate_expected(bits, radius), "dilate_disk value_bits=%#x r=%d" % (bits, radius))


@pytest.mark.parametrize("threshold", ec.D_THRESHOLDS, ids=repr)
def test_edt_sq_lt_non_finite(ops, threshold):
    """NaN, infinities, signed zeros and subnormals against thresholds of 0.0, -0.0, +inf, -inf and 0.5: the mask is
    numpy's float32 ``img < threshold``, the distances are the oracle's transform of it"""
    d2, mask = ops.edt_sq_lt(dev(ec.d_float_frames()), threshold)
    want_mask, want_d2 = ec.d_float_expected(threshold)
    same(mask, want_mask, "edt_sq_lt threshold %r: mask" % threshold)
    same(d2, want_d2, "edt_sq_lt threshold %r: d2" % threshold)
