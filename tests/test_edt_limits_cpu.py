"""The expectations of tests/edt_limit_cases.py against the CPU oracle and against each other, without a device: what
tests/test_gpu_edt_limits.py compares the device with is right before it is used, and the frames enter the parameter ranges
they were built for."""
import os

import numpy as np
import pytest

import edt_limit_cases as ec
from oracle import oracle as orc


# ================================================================================================ A: distances of 2^30 and more
@pytest.mark.parametrize("shape", ec.A_SHAPES)
def test_closed_forms_equal_the_oracle_past_2_30(shape):
    """r^2 + c^2 and its kin are what the oracle computes at the shapes whose far corner lies 2^30 and more from the zero
    pixel; every value fits int32; some 470 pixels of the single-zero frame are at or above 2^30"""
    H, W = shape
    for name in ec.A_FRAMES:
        d2 = ec.a_closed_form(shape, name)
        assert d2.dtype == np.int64 and d2.min() >= 0 and d2.max() < 2 ** 31, name
        exp = ec.a_expected(shape, name)
        assert exp.dtype == np.int32
        np.testing.assert_array_equal(exp, d2)
        np.testing.assert_array_equal(orc.edt_sq(ec.a_mask(shape, name)), exp, err_msg="%s %s" % (shape, name))
    far = ec.a_expected(shape, "one") >= ec.TWO_30
    assert 400 <= far.sum() <= 600
    assert ec.a_expected(shape, "one")[H - 1, W - 1] == (H - 1) ** 2 + (W - 1) ** 2 >= ec.TWO_30 + 1
    assert (ec.a_expected(shape, "ones") >= ec.TWO_30).any()        # the virtual pixel is that far away too
    assert not (ec.a_expected(shape, "two") >= ec.TWO_30).any()     # a zero pixel at either end halves the distance
    # cap = 2^30 cuts exactly those pixels down to 2^30 + 1
    c = ec.capped(ec.a_expected(shape, "one"), ec.TWO_30)
    assert (c[far] == ec.TWO_30 + 1).all() and (c[~far] == ec.a_expected(shape, "one")[~far]).all()


def test_smallest_frame_past_2_30():
    """(257, 32768) is the smallest frame with a distance of 2^30: one row less stays below"""
    assert 256 ** 2 + 32767 ** 2 == ec.TWO_30 + 1 and 255 ** 2 + 32767 ** 2 < ec.TWO_30
    assert all(H * W < 2 ** 30 and max(H, W) <= 32768 for H, W in ec.A_SHAPES)


# ======================================================================================= B: width limits of the LDS stages
def test_width_limits_are_the_stated_arithmetic():
    """include/pcseg.h: 24 bytes per column (rounded up to four) beside 1056 of the kernel's own in 163 840; four staged rows
    of uint32 with eight guard cells fill 163 840 bytes exactly at W = 10232"""
    lds = 160 * 1024
    need = lambda W: 24 * ((W + 3) & ~3) + 1056
    assert need(ec.REACH_MAX_W) <= lds < need(ec.REACH_MAX_W + 1)
    assert all(need(W) > lds for W in ec.B_REFUSED_W)
    assert 24 * 6828 > lds >= 24 * 6824  # 6828 is refused whatever the kernel's own share is
    assert 4 * 4 * (10232 + 8) == lds and ec.B_ROW_W == (10232, 10233)
    assert ec.reach_of(*ec.B_FILL_REACH["row blocks"]) == 32 == ec.B_DILATE_REACH["row blocks"]
    assert ec.reach_of(*ec.B_FILL_REACH["bit words"]) == 20 and ec.B_DILATE_REACH["bit words"] == 31
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "pcseg.h")) as f:
        assert "W <= %d" % ec.REACH_MAX_W in f.read()


@pytest.mark.parametrize("W", sorted({ec.REACH_MAX_W, *ec.B_BIT_W}))
def test_wide_class_frames(W):
    """the wide class maps: the dilation is a threshold of the oracle's distance, the particle fill at (20, 2) is the
    oracle's, and particle pixels sit in the first and last column"""
    x = ec.b_class_frames(W)
    p, cell, overlap = ec.B_FILL
    assert x.shape == (2, ec.B_ROWS, W) and (x[0] == p).sum() > 2 and (x == cell).mean() > 0.6
    assert x[1, 0, 0] == p and x[1, ec.B_ROWS - 1, W - 1] == p
    for radius in ec.B_DILATE_REACH.values():
        want = ec.b_dilate_expected(W, radius)
        for b in range(2):
            np.testing.assert_array_equal(want[b], orc.edt_sq(x[b] != p) <= radius * radius)
        assert 0 < want.mean() < 1
    out, area = ec.b_fill_expected(W, 20, 2)
    for b in range(2):
        o, a = orc.fill_particle_area(x[b], *ec.B_FILL)
        np.testing.assert_array_equal(out[b], o)
        assert area[b] == a > 0
    # the larger reach changes more pixels
    assert (ec.b_fill_expected(W, *ec.B_FILL_REACH["row blocks"])[1] > area).all()


@pytest.mark.parametrize("W", ec.B_ROW_W)
def test_wide_row_masks(W):
    """sparse zeros: row searches of hundreds of offsets; the single zero in column 0: r^2 + c^2 from (4, 0)"""
    m, d2 = ec.b_row_masks(W), ec.b_row_expected(W)
    assert d2[0].max() > 500 ** 2
    r, c = np.mgrid[:ec.B_ROWS, :W]
    np.testing.assert_array_equal(d2[1], (r - 4) ** 2 + c ** 2)
    assert (ec.capped(d2, ec.EDT_CAP) == np.minimum(d2, ec.EDT_CAP + 1)).all() and (d2 <= ec.EDT_CAP).any()
    assert (m[1] == 0).sum() == 1


# ================================================================================================ C: fill_particle's parameters
@pytest.mark.parametrize("shape", ec.C_SHAPES)
def test_fill_reference_is_the_oracle_at_its_parameters(shape):
    """fill_reference at (20, 2) equals orc.fill_particle_area on every frame used, whatever the labels"""
    for triple in ec.C_TRIPLES:
        frames = ec.c_frames(shape, triple)
        out, area = ec.c_expected(shape, triple, (20, 2))
        for b, name in enumerate(ec.C_FRAMES):
            o, a = orc.fill_particle_area(frames[b], *triple)
            np.testing.assert_array_equal(out[b], o, err_msg="%s %s %s" % (shape, triple, name))
            assert area[b] == a, (shape, triple, name)
            # without a precomputed distance it is the same function
            o2, a2 = ec.fill_reference(frames[b], *triple, 20, 2)
            assert a2 == a and (o2 == o).all()


@pytest.mark.parametrize("shape", ec.C_SHAPES)
def test_fill_reference_dilation_term(shape):
    """its dilation term is the oracle's disk dilation of the particle, for every radius used and every labelling: with a
    threshold of 0 the distance term is empty, so the changed pixels are the cell pixels inside the dilation"""
    radii = sorted({r for r, _ in ec.C_PAIRS + ec.C_TRIPLE_PAIRS})
    assert radii == [0, 1, 2, 3, 5, 20, 31, 32, 180]
    for triple in ec.C_TRIPLES:
        p, cell, overlap = triple
        frames, d2 = ec.c_frames(shape, triple), ec.c_d2(shape, triple)
        for b, name in enumerate(ec.C_FRAMES):
            particle = frames[b] == p
            for r in radii:
                dil = orc.binary_dilation_disk(particle, r)
                np.testing.assert_array_equal(particle.any() & (d2[b] <= r * r), dil, err_msg="%s %s %s r=%d" % (shape, triple, name, r))
                out, area = ec.fill_reference(frames[b], *triple, r, 0, d2=d2[b])
                hit = (frames[b] == cell) & dil
                assert area == hit.sum()
                np.testing.assert_array_equal(out, np.where(hit, overlap, frames[b]))


@pytest.mark.parametrize("shape", ec.C_SHAPES)
def test_fill_frames_enter_the_ranges(shape):
    H, W = shape
    assert ec.C_DEFAULT in ec.C_TRIPLES and len(ec.c_cases()) == len(ec.C_PAIRS) + (len(ec.C_TRIPLES) - 1) * len(ec.C_TRIPLE_PAIRS)
    reach = {pair: ec.reach_of(*pair) for pair in ec.C_PAIRS}
    assert reach[(20, 32)] == 31 and reach[(31, 32)] == 31 and reach[(20, 33)] == 32 and reach[(2, 5)] == 4 and reach[(5, 40)] == 39
    assert max(20 * 20, 32 * 32 - 1) == 1023 and max(20 * 20, 33 * 33 - 1) == 1088 and max(5 * 5, 40 * 40 - 1) == 1599
    for triple in ec.C_TRIPLES:
        p, cell, overlap = triple
        x = ec.c_frames(shape, triple)
        particle = x == p
        assert particle[0].sum() > 100 and particle[1].sum() == 8 and not particle[2].any() and particle[3].sum() == H // 2 - H // 4
        assert particle[1, 0, 0] and particle[1, 0, W - 1] and particle[1, H - 1, 0] and particle[1, H - 1, W - 1]
        assert particle[1, 31 % H].any() and particle[1, 32 % H].any() and particle[1, :, 447 % W].any() and particle[1, :, 448 % W].any()
        for v in (64 + p, 128 + p, 255, cell ^ 128):  # bytes that must never count as particle; the last never as cell
            assert (x == v).any(axis=(1, 2)).all(), (triple, v)
        if cell != p:
            assert 0.6 < (x == cell).mean() < 0.8
        else:
            assert ((x == cell) == particle).all()
    # the pairs tell each other apart on the default labels: neighbouring reaches give different areas
    area = {pair: ec.c_expected(shape, ec.C_DEFAULT, pair)[1] for pair in ec.C_PAIRS}
    assert (area[(0, 0)] == 0).all()
    assert area[(20, 2)][0] < area[(20, 32)][0] < area[(20, 33)][0] < area[(5, 40)][0]  # (the disk)
    assert area[(20, 2)][2] < area[(20, 32)][2] < area[(20, 33)][2]  # (no particle: the virtual pixel, by the threshold alone)
    assert (area[(0, 1)] == 0).all() and area[(0, 2)][0] > 0  # cell != particle: distance 0 is never a cell pixel
    # labels (63, 128, 128): the output is the input, the area is not zero
    out, a = ec.c_expected(shape, (63, 128, 128), (20, 2))
    assert (out == ec.c_frames(shape, (63, 128, 128))).all() and a[0] > 0
    # labels (2, 2, 7): every particle pixel is a cell pixel at distance 0
    out, a = ec.c_expected(shape, (2, 2, 7), (20, 2))
    assert (a == (ec.c_frames(shape, (2, 2, 7)) == 2).sum(axis=(1, 2))).all()


# ================================================================================== D: caps, class bytes, non-finite thresholds
@pytest.mark.parametrize("shape", ec.D_CAP_SHAPES)
def test_cap_frames_straddle_every_small_cap(shape):
    H, W = shape
    m, d2 = ec.d_cap_masks(shape), ec.d_cap_d2(shape)
    assert (m[0] == 0).sum() >= 2 and (m[1] == 0).sum() == 1 and m[2].all()
    r, c = np.mgrid[:H, :W]
    np.testing.assert_array_equal(d2[1], (H - 1 - r) ** 2 + c ** 2)
    np.testing.assert_array_equal(d2[2], (r + 1) ** 2 + c ** 2)
    for cap in ec.D_SMALL_CAPS:
        for b, name in enumerate(ec.D_CAP_FRAMES):
            assert (d2[b] <= cap).any() == (name != "none" or cap >= 1) and (d2[b] > cap).any(), (cap, name)
        assert (ec.capped(d2, cap) == cap + 1).all(axis=(1, 2)).sum() == (cap == 0)  # (only the frame without a zero, at cap 0)
    for cap in ec.D_CAPS:
        got = ec.capped(d2, cap)
        assert got.dtype == np.int32 and got.max() <= min(cap + 1, d2.max())
        assert ((got == d2) | ((d2 > cap) & (got == cap + 1))).all()
    np.testing.assert_array_equal(ec.capped(d2, 2 ** 31 - 1), d2)  # nothing exceeds it
    # perfect squares and their neighbours are among the caps
    assert {3, 4, 5, 8, 9, 10, 15, 16, 17, 48, 49, 50} <= set(ec.D_SMALL_CAPS)
    assert np.float32(2 ** 24 + 1) == 2 ** 24  # a cap that float32 cannot hold


def test_class_bytes_and_value_sets():
    x = ec.d_class_bytes()
    assert x.shape == (4,) + ec.D_SHAPE and x.dtype == np.uint8
    for v in ec.D_RARE_BYTES + ec.D_COMMON_BYTES:
        assert (x == v).any(), v
    assert {0, 1, 2, 3, 4, 5, 64, 65, 66, 67, 68, 69, 255} <= set(np.unique(x)) and (x >= 128).any()
    for v in ec.D_RARE_BYTES:
        assert (x[3] == v).sum() == 1
    for bits, members in zip(ec.D_VALUE_BITS, ([1], [1, 5], [63], [])):
        np.testing.assert_array_equal(ec.in_value_set(x, bits), np.isin(x, members))
        for radius in ec.D_RADII:
            want = ec.d_dilate_expected(bits, radius)
            if members:
                assert (0 < want.mean(axis=(1, 2))).all() and want.mean() < 1, (bits, radius)
                for b in range(4):
                    np.testing.assert_array_equal(want[b], orc.edt_sq(~np.isin(x[b], members)) <= radius * radius)
            else:
                assert not want.any()  # the empty set dilates to the empty set
    # a byte of 64 and more, shifted without the guard, would wrap to v % 64
    assert (x % 64 == 1).sum() > (x == 1).sum() and (x % 64 == 63).sum() > (x == 63).sum()


def test_non_finite_frames_and_thresholds():
    x = ec.d_float_frames()
    assert x.dtype == np.float32
    sub = (x != 0) & (np.abs(x) < np.finfo(np.float32).tiny)
    for what, sel in (("nan", np.isnan(x)), ("+inf", np.isposinf(x)), ("-inf", np.isneginf(x)), ("-0.0", (x == 0) & np.signbit(x)),
                      ("0.0", (x == 0) & ~np.signbit(x)), ("subnormal > 0", sub & (x > 0)), ("subnormal < 0", sub & (x < 0))):
        assert sel.sum() >= 20, what
    masks = {t: ec.d_float_expected(t)[0] for t in ec.D_THRESHOLDS}
    # neither zero is below either zero, a negative subnormal is; NaN is below nothing, not even +inf
    zero = masks[0.0]
    assert not zero[x == 0].any() and zero[sub & (x < 0)].all() and not zero[sub & (x > 0)].any()
    np.testing.assert_array_equal(ec.d_float_expected(-0.0)[0], zero)
    inf = masks[float("inf")]
    assert not inf[np.isnan(x)].any() and not inf[np.isposinf(x)].any() and inf[np.isneginf(x)].all() and inf[np.isfinite(x)].all()
    assert not masks[float("-inf")].any() and (ec.d_float_expected(float("-inf"))[1] == 0).all()
    half = masks[0.5]
    assert 0.5 < half.mean() < 0.9 and not half[np.isnan(x)].any()
    for t in ec.D_THRESHOLDS:
        m, d2 = ec.d_float_expected(t)
        assert ((d2 == 0) == (m == 0)).all()
