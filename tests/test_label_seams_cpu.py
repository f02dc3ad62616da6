"""The host side of the seam tests (tests/seam_patterns.py) on its own, and the oracle -- the judge of every labelling
test -- against scipy where scipy is installed.  Needs no GPU; every comparison is equality."""
import numpy as np
import pytest

import seam_patterns as sp
from oracle import oracle as orc


# ------------------------------------------------------------------------------------------------ the pattern helper
@pytest.mark.parametrize("connectivity", [1, 2])
def test_window_frames_padding_equals_oracle_on_whole_frame(connectivity):
    """Labelling a window alone and padding the labels is labelling the padded frame: 512 seeded binary windows per
    connectivity at the tile corner of a 34 x 66 frame, and the mosaic labelling against one oracle call per window."""
    rng = np.random.default_rng(11 + connectivity)
    wins = sp.all_binary_windows()[rng.choice(65536, 512, replace=False)]
    labs = sp.window_labels(wins, connectivity=connectivity)
    frames = sp.window_frames((34, 66), (30, 62), wins)
    expect = sp.window_frames((34, 66), (30, 62), labs)
    assert frames.shape == (512, 34, 66) and frames.dtype == np.uint8 and frames[:, :30].sum() == 0 and frames[:, :, :62].sum() == 0
    for k in range(512):
        np.testing.assert_array_equal(labs[k], orc.label(wins[k] > 0, connectivity=connectivity))
        np.testing.assert_array_equal(expect[k], orc.label(frames[k] > 0, connectivity=connectivity))


def test_window_labels_equal_values_and_dilated_windows():
    """The other two forms of window_labels: equal-valued components of windows over {0 .. 3}, and windows dilated by a
    disk of radius 2 and cut off by the frame's edge before they are labelled."""
    wins = sp.random_windows(512, 4, seed=5)
    labs = sp.window_labels(wins, equal=True)
    frames = sp.window_frames((35, 67), (30, 62), wins)
    expect = sp.window_frames((35, 67), (30, 62), labs)
    for k in range(512):
        np.testing.assert_array_equal(labs[k], orc.label(wins[k].astype(np.int32)))
        np.testing.assert_array_equal(expect[k], orc.label(frames[k].astype(np.int32)))
    wins = sp.all_binary_windows()[np.random.default_rng(6).choice(65536, 512, replace=False)]
    # window at rows 126 .. 129, columns 62 .. 65 of a 131 x 67 frame: dilated it covers rows 124 .. 131 and columns
    # 60 .. 67, of which 7 rows and 7 columns lie inside the frame
    labs = sp.window_labels(wins, radius=2, room=(7, 7))
    frames = sp.window_frames((131, 67), (126, 62), wins)
    expect = sp.window_frames((131, 67), (124, 60), labs)
    for k in range(512):
        np.testing.assert_array_equal(expect[k], orc.label(orc.binary_dilation_disk(frames[k] > 0, 2)))


def test_window_frames_cuts_what_hangs_over():
    wins = np.arange(1, 33, dtype=np.int32).reshape(2, 4, 4)
    out = sp.window_frames((5, 6), (3, 4), wins)
    assert out.shape == (2, 5, 6) and out.dtype == np.int32
    np.testing.assert_array_equal(out[1, 3:, 4:], wins[1, :2, :2])
    assert out[:, :3].sum() == 0 and out[:, :, :4].sum() == 0
    with pytest.raises(ValueError):
        sp.window_frames((5, 6), (5, 0), wins)


def _words(cols, H):
    """Column bit words (ceil(H / 32), W) from a list of per-column row lists."""
    W = len(cols)
    bits = np.zeros(((H + 31) // 32, W), np.uint32)
    for c, rows in enumerate(cols):
        for r in rows:
            bits[r // 32, c] |= np.uint32(1) << np.uint32(r % 32)
    return bits.view(np.int32)


def test_run_partition_on_hand_made_words():
    """Runs that end at bit 31, runs that start at bit 0 of the next word, a run cut in two by the word seam, a
    diagonal-only contact across the word seam -- with the parent entries written by hand at the run heads only
    (every other entry holds a poison value that a wrong node choice would trip over)."""
    H, W = 70, 4
    POISON = 10 ** 9
    # column 0: rows 29 .. 34 (one vertical line = two runs: 29 .. 31 and 32 .. 34); column 1: rows 30 .. 31 (ends at bit
    # 31); column 2: rows 32 .. 33 (starts at bit 0 of word 1: touches column 1 only diagonally, (31, 1) - (32, 2));
    # column 3: rows 0 .. 1 and 66 .. 69 (apart from everything)
    cols = [list(range(29, 35)), [30, 31], [32, 33], [0, 1, 66, 67, 68, 69]]
    bits = _words(cols, H)
    par = np.full((H, W), POISON, np.int32)
    head = lambda r, c: r * W + c
    par[29, 0] = head(29, 0)                # root of the big component
    par[32, 0] = head(29, 0)                # the lower half of the line -> its upper half (vertical link across the seam)
    par[30, 1] = head(29, 0)                # left link
    par[32, 2] = head(30, 1)                # diagonal link across the word seam, two steps from the root
    par[0, 3] = head(0, 3)
    par[66, 3] = head(66, 3)
    roots = sp.run_partition(bits, par, H)
    mask, tail = sp.unpack_bits(bits, H)
    assert not tail
    exp_mask = np.zeros((H, W), bool)
    for c, rows in enumerate(cols):
        exp_mask[rows, c] = True
    np.testing.assert_array_equal(mask, exp_mask)
    np.testing.assert_array_equal(roots > 0, exp_mask)
    assert set(roots[exp_mask]) == {head(29, 0) + 1, head(0, 3) + 1, head(66, 3) + 1}
    assert roots[33, 2] == head(29, 0) + 1 and roots[34, 0] == head(29, 0) + 1 and roots[31, 1] == head(29, 0) + 1
    assert roots[1, 3] == head(0, 3) + 1 and roots[69, 3] == head(66, 3) + 1
    assert sp.same_partition(roots, orc.label(exp_mask))
    # the batched form, frame 1 = the same words with the diagonal contact left unlinked: one component more
    par2 = par.copy()
    par2[32, 2] = head(32, 2)
    both = sp.run_partition(np.stack([bits, bits]), np.stack([par, par2]), H)
    np.testing.assert_array_equal(both[0], roots)
    assert sp.same_partition(both[0], orc.label(exp_mask)) and not sp.same_partition(both[1], orc.label(exp_mask))
    assert not sp.same_partition(both, np.stack([orc.label(exp_mask)] * 2))
    # an entry above its own index, and a bit below the frame's last row, are refused
    bad = par.copy()
    bad[29, 0] = head(32, 0)
    with pytest.raises(ValueError):
        sp.run_partition(bits, bad, H)
    with pytest.raises(ValueError):
        sp.run_partition(_words([[71]], 96)[:3], np.zeros((70, 1), np.int32), 70)


def test_same_partition():
    a = np.array([[1, 1, 0], [0, 2, 2], [3, 0, 0]])
    assert sp.same_partition(a, np.array([[7, 7, 0], [0, 1, 1], [4, 0, 0]]))
    assert not sp.same_partition(a, np.array([[7, 7, 0], [0, 7, 7], [4, 0, 0]]))   # two components joined
    assert not sp.same_partition(a, np.array([[7, 5, 0], [0, 1, 1], [4, 0, 0]]))   # one component split
    assert not sp.same_partition(a, np.array([[7, 7, 1], [0, 1, 1], [4, 0, 0]]))   # another foreground
    assert sp.same_partition(np.zeros((2, 2), int), np.zeros((2, 2), int))
    # batched: the same number may name different components in different frames
    b = np.stack([a, a])
    c = np.stack([a, np.where(a > 0, 4 - a, 0)])
    assert sp.same_partition(b, c)
    c[1, 0, 0] = c[1, 1, 1]
    assert not sp.same_partition(b, c)


def test_structured_frames_are_what_they_claim():
    for shape in [(1, 64), (3, 65), (35, 67), (65, 129)]:
        f = sp.structured_frames(shape)
        H, W = shape
        assert all(v.shape == shape and v.dtype == np.uint8 for v in f.values())
        assert orc.label(f["serpentine"] > 0, connectivity=1, return_num=True)[1] == 1
        assert f["serpentine"].sum() == ((H + 1) // 2) * W + H // 2
        assert orc.label(f["comb"] > 0, connectivity=1, return_num=True)[1] == 1
        assert orc.label(f["checker"], return_num=True)[1] == (2 if H > 1 else W)
        assert orc.label(f["diag2"] > 0, connectivity=1, return_num=True)[1] == (H * W + 1) // 2
        assert orc.label(f["diag2"] > 0, return_num=True)[1] == (1 if H > 1 else (W + 1) // 2)
        assert orc.label(f["lattice"] > 0, return_num=True)[1] == ((H + 1) // 2) * ((W + 1) // 2)
        assert f["full"].all() and not f["empty"].any()
        assert f["vline"].sum() == H and f["hline"].sum() == W
        if H >= 3:
            assert orc.label(f["rings10"] > 0, return_num=True)[1] == (min(H, W) + 3) // 4
            assert orc.label(f["diag3"] > 0, connectivity=1, return_num=True)[1] == f["diag3"].sum()
    for off in range(6):
        bn = sp.block_noise((35, 67), 5, off, seed=3)
        assert bn.shape == (35, 67) and bn.min() >= 1 and bn.max() <= 5
        edge = 6 - off if off else 6  # the first block edge
        assert (bn[:edge] == bn[:1]).all() and (bn[:, :edge] == bn[:, :1]).all()
        assert (bn[edge] != bn[edge - 1]).any()
    np.testing.assert_array_equal(sp.block_noise((35, 67), 5, 2, seed=3), sp.block_noise((35, 67), 5, 2, seed=3))


# ------------------------------------------------------------------------------------------------ the oracle vs scipy
def _cases():
    """name -> uint8 class image: every structured frame at two shapes, block noise, and 4096 seeded 4 x 4 windows set
    side by side with an empty rim (one image per 1024 windows)."""
    cases = {}
    for shape in [(35, 67), (65, 129)]:
        for name, img in sp.structured_frames(shape).items():
            cases["%s_%dx%d" % ((name,) + shape)] = img
        for off in (0, 1, 5):
            cases["blocks%d_%dx%d" % ((off,) + shape)] = sp.block_noise(shape, 5, off, seed=off)
    wins = sp.random_windows(4096, 4, seed=17)
    for k in range(4):
        cells = np.zeros((1024, 5, 5), np.uint8)
        cells[:, :4, :4] = wins[1024 * k:1024 * (k + 1)]
        cases["windows%d" % k] = np.ascontiguousarray(cells.reshape(32, 32, 5, 5).transpose(0, 2, 1, 3).reshape(160, 160))
    return cases


def _raster_renumber(lab):
    """Renumber a label image 1 .. N by the raster position of each label's first pixel."""
    flat = lab.ravel()
    vals, first = np.unique(flat, return_index=True)
    keep = vals != 0
    vals, first = vals[keep], first[keep]
    lut = np.zeros(int(flat.max()) + 1, np.int32)
    lut[vals[np.argsort(first)]] = np.arange(1, vals.size + 1)
    return lut[lab]


def test_oracle_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    full, cross = np.ones((3, 3), int), ndi.generate_binary_structure(2, 1)
    yy, xx = np.mgrid[-5:6, -5:6]
    for name, img in _cases().items():
        m = img > 0
        # boolean labellings: scipy numbers components in raster order of their first pixel too
        for conn, st in ((2, full), (1, cross)):
            exp, n = ndi.label(m, structure=st)
            got, gn = orc.label(m, connectivity=conn, return_num=True)
            np.testing.assert_array_equal(got, exp, err_msg="%s conn %d" % (name, conn))
            assert gn == n
        # equal-valued components: per-value scipy labellings, offset and renumbered by first pixel
        comb = np.zeros(img.shape, np.int64)
        total = 0
        for v in np.unique(img[img > 0]):
            lv, nv = ndi.label(img == v, structure=full)
            comb[lv > 0] = lv[lv > 0] + total
            total += nv
        got, gn = orc.label(img.astype(np.int32), return_num=True)
        np.testing.assert_array_equal(got, _raster_renumber(comb), err_msg=name)
        assert gn == total
        np.testing.assert_array_equal(orc.binary_fill_holes(m), ndi.binary_fill_holes(m), err_msg=name)
        np.testing.assert_array_equal(orc.median_filter(img), ndi.median_filter(img, size=5, mode="reflect"), err_msg=name)
        for rad in (1, 2, 5):
            disk = (xx * xx + yy * yy <= rad * rad)[5 - rad:6 + rad, 5 - rad:6 + rad]
            np.testing.assert_array_equal(orc.binary_dilation_disk(m, rad), ndi.binary_dilation(m, structure=disk),
                                          err_msg="%s r %d" % (name, rad))
        if not m.all():  # (the frame without a zero pixel is scipy's degenerate case: below)
            np.testing.assert_array_equal(np.sqrt(orc.edt_sq(m).astype(np.float64)), ndi.distance_transform_edt(m), err_msg=name)


@pytest.mark.parametrize("shape", [(35, 67), (65, 129), (32768, 3), (3, 32768)])
def test_oracle_edt_degenerate_and_limit_shapes_against_scipy(shape):
    """What the GPU limit test expects of ``edt_sq`` comes from the oracle; here the oracle itself is held against scipy
    on the same masks: a zero pixel at one end, one at each end, and the frame without any zero pixel -- which scipy
    answers as if one zero pixel sat at (-1, 0), d^2 = (r + 1)^2 + c^2."""
    ndi = pytest.importorskip("scipy.ndimage")
    H, W = shape
    one = np.ones(shape, bool)
    one[0, 0] = False
    two = one.copy()
    two[H - 1, W - 1] = False
    for m in (one, two):
        d2 = orc.edt_sq(m)
        np.testing.assert_array_equal(np.sqrt(d2.astype(np.float64)), ndi.distance_transform_edt(m))
    r, c = np.mgrid[:H, :W].astype(np.int64)
    d2 = orc.edt_sq(np.ones(shape, bool))
    np.testing.assert_array_equal(d2, (r + 1) ** 2 + c ** 2)
    np.testing.assert_array_equal(np.sqrt(d2.astype(np.float64)), ndi.distance_transform_edt(np.ones(shape, bool)))
