"""The host side of the local-maxima seam tests (tests/maxima_windows.py) on its own, and the oracle's local_maxima -- the
judge of tests/test_gpu_maxima_seams.py -- against a plain restatement of the definition.  Needs no GPU; every
comparison is equality."""
import numpy as np
import pytest

import maxima_windows as mw
import seam_patterns as sp
from oracle import oracle as orc

SHAPE = (34, 66)                                    # 2 x 2 tiles, the corner at (32, 64)
ORIGINS = [(30, 62), (30, 63), (31, 62), (31, 63)]  # the corner at each interior grid point of a 3 x 3 window
ROLES = [mw.LOW, mw.MIDDLE, mw.HIGH]


# ------------------------------------------------------------------------------------- the oracle vs the definition
def restated(ndi, img, cells=None):
    """Local maxima by the definition: plateaus are the 8-connected components of equal value; a plateau is a maximum iff
    no pixel of it has a strictly higher 8-neighbour; neighbours outside the frame never count; a constant frame has
    none.  ``cells`` = (rows, columns): ``img`` is a mosaic of independent frames of that shape, each followed by one row
    and one column of a value below every frame's (a neighbour that is never higher and belongs to no plateau, which is
    what the outside of a frame is), and "constant" is judged per frame."""
    img = np.asarray(img, np.int64)
    floor = img.min() - 1
    higher = ndi.maximum_filter(img, size=3, mode="constant", cval=floor) > img
    out = np.zeros(img.shape, bool)
    sep = np.zeros(img.shape, bool)
    if cells is not None:
        sep[cells[0]::cells[0] + 1, :] = True
        sep[:, cells[1]::cells[1] + 1] = True
    for v in np.unique(img[~sep]):
        lab, n = ndi.label((img == v) & ~sep, structure=np.ones((3, 3), int))
        spoilt = np.zeros(n + 1, bool)
        spoilt[np.unique(lab[higher])] = True
        spoilt[0] = True
        out |= ~spoilt[lab]
    if cells is None:
        return out & bool((img != img.flat[0]).any())
    ch, cw = cells[0] + 1, cells[1] + 1
    gh, gw = img.shape[0] // ch, img.shape[1] // cw
    per = img.reshape(gh, ch, gw, cw)[:, :cells[0], :, :cells[1]]
    const = (per == per[:, :1, :, :1]).all(axis=(1, 3))  # (gh, gw)
    return out & ~np.repeat(np.repeat(const, ch, axis=0), cw, axis=1)


def mosaic(frames, floor):
    """(n, h, w) -> one image of the frames side by side, each followed by a row and a column of ``floor``; n must be a
    multiple of the 64 frames of a mosaic row."""
    n, h, w = frames.shape
    cells = np.full((n, h + 1, w + 1), floor, frames.dtype)
    cells[:, :h, :w] = frames
    return np.ascontiguousarray(cells.reshape(n // 64, 64, h + 1, w + 1).transpose(0, 2, 1, 3).reshape(n // 64 * (h + 1), 64 * (w + 1)))


def unmosaic(img, n, h, w):
    return img.reshape(n // 64, h + 1, 64, w + 1).transpose(0, 2, 1, 3).reshape(n, h + 1, w + 1)[:, :h, :w]


@pytest.mark.parametrize("background", ROLES)
@pytest.mark.parametrize("origin", [(30, 62), (31, 63)])
def test_oracle_against_the_definition(origin, background):
    """Every crop the GPU test's expectations come from -- all 19 683 windows in a background of each role, in the frame's
    interior (7 x 6 crop) and in its last rows and columns (5 x 5 crop with the frame's own edges) -- through the oracle
    and through ``restated`` (scipy.ndimage.label + maximum_filter).  The restatement runs on mosaics of crops; that a
    mosaic cell is judged like the crop alone is checked on every 37th crop."""
    ndi = pytest.importorskip("scipy.ndimage")
    wins = mw.all_ternary_windows()
    exp = mw.expected("ternary", SHAPE, origin, background)
    rlo, rhi, clo, chi = exp.box
    crops = mw.value_frames((rhi - rlo, chi - clo), (origin[0] - rlo, origin[1] - clo), wins, background, (0, 1, 2))
    n, h, w = crops.shape
    pad = (-n) % 64
    padded = np.concatenate([crops, np.repeat(crops[:1], pad, axis=0)])
    got = unmosaic(restated(ndi, mosaic(padded, -1), cells=(h, w)), n + pad, h, w)[:n]
    differ = np.flatnonzero((got != exp.is_max.astype(bool)).reshape(n, -1).any(axis=1))
    assert differ.size == 0, "%d crops differ, first: window %d\n%s\n oracle:\n%s\n definition:\n%s" % (
        differ.size, differ[0], crops[differ[0]], exp.is_max[differ[0]], got[differ[0]].astype(np.uint8))
    for k in range(0, n, 37):
        np.testing.assert_array_equal(restated(ndi, crops[k]), got[k], err_msg="window %d alone" % k)


def test_oracle_against_the_definition_on_whole_frames():
    """The same on the whole frames of the GPU test: the structured frames as they are and spoilt at the far end, their
    distance maps, constant frames with one pixel changed, the peak frames and the dense ones."""
    ndi = pytest.importorskip("scipy.ndimage")
    frames = []
    for shape in [(33, 65), (35, 67)]:
        for name, f in sp.structured_frames(shape).items():
            frames += [(name, f.astype(np.int32)), (name + " edt", orc.edt_sq(f > 0))]
            spoilt = mw.spoilt_at_the_far_end(f)
            assert (spoilt is None) == (name in ("full", "empty"))
            if spoilt is not None:
                g, (r, c) = spoilt
                assert (g != f).sum() == 1 and g.max() == f.max() + 1 and g[r, c] == f.max() and not orc.local_maxima(g)[r, c]
                frames.append((name + " spoilt", g))
        frames += list(zip(*mw.one_pixel_frames(shape, [(0, 0), (shape[0] - 1, shape[1] - 1), (32, 64), (20, 30)])))
        frames += list(mw.peak_frames(shape).items()) + list(mw.dense_frames(shape).items())
    for name, f in frames:
        np.testing.assert_array_equal(orc.local_maxima(f), restated(ndi, f), err_msg="%s %s" % (name, f.shape))


def test_dense_frames_fill_the_counting_blocks():
    f = mw.dense_frames((35, 67))
    assert f["peaks"].sum() == 18 * 34 and f["peaks"].ravel()[:1024].sum() == 8 * 34  # a marker in every fourth pixel
    assert f["squares"][:5, :5].tolist() == [[1, 1, 0, 1, 1], [1, 1, 0, 1, 1], [0, 0, 0, 0, 0], [1, 1, 0, 1, 1], [1, 1, 0, 1, 1]]
    assert f["tail"].ravel()[:2048].sum() == 0 and f["tail"].sum() > 0 and (f["tail"].ravel()[2048:] == f["peaks"].ravel()[2048:]).all()
    for g in f.values():
        assert g.dtype == np.int32 and mw.frame_answer(g)[2] > 0
    assert mw.frame_answer(f["peaks"])[2] == 18 * 34 and mw.frame_answer(mw.peak_frames((3, 65))["constant"])[2] == 0


# --------------------------------------------------------------------------------------------------------- the helper
def test_all_ternary_windows():
    wins = mw.all_ternary_windows()
    assert wins.shape == (19683, 3, 3) and wins.dtype == np.uint8 and wins.max() == 2
    assert len({w.tobytes() for w in wins}) == 19683
    k = 2 + 1 * 3 + 2 * 3 ** 5  # pixel (0, 0) high, (0, 1) middle, (1, 2) high
    assert wins[k, 0, 0] == 2 and wins[k, 0, 1] == 1 and wins[k, 1, 2] == 2 and wins[k].sum() == 5
    np.testing.assert_array_equal(wins[k].ravel(), [(k // 3 ** j) % 3 for j in range(9)])
    f = mw.value_frames(SHAPE, (31, 63), wins[[19682]], mw.MIDDLE, (-1, 0, 1))
    assert f.dtype == np.int32 and f.shape == (1, 34, 66) and (f[0, 31:, 63:] == 1).all() and f.sum() == 9
    f = mw.value_frames(SHAPE, (33, 65), wins[[0]], mw.HIGH, mw.MAPS["range_ends"])  # all but one pixel hangs over
    assert f[0, 33, 65] == mw.INT_MIN + 1 and (f == mw.INT_MAX).sum() == 34 * 66 - 1
    with pytest.raises(ValueError):
        mw.value_frames(SHAPE, (0, 0), wins[:1], 0, (0, 0, 1))
    with pytest.raises(ValueError):
        mw.value_frames(SHAPE, (0, 0), wins[:1], 0, (mw.INT_MIN, 0, 1))


def test_crop_box_keeps_the_frames_own_edge():
    assert mw.crop_box(SHAPE, (30, 62), (3, 3)) == (28, 34, 60, 66)   # one background row / column, then the edge
    assert mw.crop_box(SHAPE, (31, 63), (3, 3)) == (29, 34, 61, 66)   # the window on the edge: no ring added there
    assert mw.crop_box((35, 67), (30, 62), (4, 4)) == (28, 35, 60, 67)
    assert mw.crop_box((97, 200), (40, 90), (3, 3)) == (38, 45, 88, 95)
    assert mw.crop_box(SHAPE, (0, 0), (3, 3)) == (0, 5, 0, 5)
    with pytest.raises(ValueError):
        mw.crop_box((3, 65), (0, 30), (3, 3))  # the window cuts the background in two


def test_the_window_on_the_last_row_is_not_the_window_in_a_ring():
    """A high pixel at the bottom middle of a window on the frame's last row, low pixels around it: no background pixel
    touches it, so the background stays a maximum -- with one more ring of background below it would not."""
    win = np.array([[1, 1, 1], [0, 0, 0], [0, 2, 0]], np.uint8)
    exp = mw.window_expected(SHAPE, (31, 62), win[None], mw.MIDDLE)
    assert exp.outside_max[0] == 1 and exp.counts[0] == 2 and exp.outside_marker[0] == 1
    inner = mw.window_expected((40, 70), (31, 62), win[None], mw.MIDDLE)
    assert inner.outside_max[0] == 0 and inner.counts[0] == 1


def frames_of(exp, field, ks):
    return np.concatenate([mw.spread(exp, field, k, k + 1) for k in ks])


@pytest.mark.parametrize("case", [("ternary", SHAPE, o, mw.MIDDLE) for o in ORIGINS] +
                         [("ternary", SHAPE, (30, 62), mw.LOW), ("ternary", SHAPE, (30, 62), mw.HIGH),
                          ("ternary", (34, 128), (31, 63), mw.MIDDLE), ("ternary", (5, 6), (0, 1), mw.MIDDLE), ("ternary", SHAPE, (0, 0), mw.MIDDLE),
                          ("ternary", SHAPE, (0, 63), mw.LOW),
                          (("random4", 40000, 40034), (34, 66), (30, 62), mw.MIDDLE),
                          (("random4", 40000, 40035), (35, 67), (30, 62), mw.MIDDLE)], ids=str)
def test_crop_expectation_equals_oracle_on_whole_frame(case):
    """512 seeded windows per placement the GPU test uses, and three with the window in the frame's first row -- where
    window pixels precede the background's first pixel: is_max, markers in the frame's raster order and counts from the
    crop equal orc.local_maxima / orc.label of the whole frame."""
    family, shape, origin, background = case
    exp = mw.expected(family, shape, origin, background)
    wins = mw.windows(family)
    pick = np.sort(np.random.default_rng(512).choice(wins.shape[0], 512, replace=False))
    frames = mw.value_frames(shape, origin, wins[pick], background, (0, 1, 2))
    is_max, markers, counts = mw.frames_answer(frames)
    np.testing.assert_array_equal(frames_of(exp, "is_max", pick), is_max)
    np.testing.assert_array_equal(frames_of(exp, "markers", pick), markers)
    np.testing.assert_array_equal(exp.counts[pick], counts)
    assert exp.is_max.dtype == np.uint8 and exp.markers.dtype == np.int32 and exp.counts.dtype == np.int32


def test_expectation_does_not_depend_on_the_map():
    """Every 7th window at every origin: the crop expectation under the three maps, and the oracle on whole frames under
    the extreme map for every 290th."""
    wins = mw.all_ternary_windows()[::7]
    for origin in ORIGINS:
        for background in ROLES:
            base = mw.window_expected(SHAPE, origin, wins, background)
            for name, values in mw.MAPS.items():
                other = mw.window_expected(SHAPE, origin, wins, background, values)
                for a, b in zip(base[2:], other[2:]):
                    np.testing.assert_array_equal(a, b, err_msg="%s %s" % (name, origin))
            frames = mw.value_frames(SHAPE, origin, wins[::290], background, mw.MAPS["range_ends"])
            is_max, markers, counts = mw.frames_answer(frames)
            np.testing.assert_array_equal(mw.spread(base, "markers")[::290], markers)
            np.testing.assert_array_equal(mw.spread(base, "is_max")[::290], is_max)
            np.testing.assert_array_equal(base.counts[::290], counts)


# ------------------------------------------------------------------------------------------- what the windows reach
def test_background_plateau_is_a_maximum_often_enough():
    """The middle background survives exactly where no background pixel touches a high pixel.  In the frame's interior:
    the 2^9 - 1 windows over {low, middle} that are not the constant frame, and the one with a high centre in a ring of
    low pixels; more on the frame's last row and column."""
    for origin in ORIGINS:
        exp = mw.expected("ternary", SHAPE, origin, mw.MIDDLE)
        assert exp.outside_max.sum() >= 500, origin
        assert exp.outside_max[(3 ** 9 - 1) // 2] == 0 and exp.counts[(3 ** 9 - 1) // 2] == 0  # the constant frame
    assert mw.expected("ternary", SHAPE, (30, 62), mw.MIDDLE).outside_max.sum() == 512
    assert mw.expected("ternary", SHAPE, (31, 63), mw.MIDDLE).outside_max.sum() > 512
    assert mw.expected("ternary", SHAPE, (30, 62), mw.HIGH).outside_max.sum() == 19682
    assert mw.expected("ternary", SHAPE, (30, 62), mw.LOW).outside_max.sum() == 0


@pytest.mark.parametrize("origin", ORIGINS)
def test_windows_reach_the_seam_rules(origin):
    """Among 768 seeded windows at each origin there are: a background spoilt only from another tile than its root's, a
    window plateau joined to a maximal background across a seam, and a maximal plateau of the window's own across a
    seam (maxima_windows.window_classes)."""
    wins = mw.all_ternary_windows()
    pick = np.random.default_rng(768).choice(wins.shape[0], 768, replace=False)
    seen = {"spoilt_from_another_tile": 0, "joined_across_a_seam": 0, "own_plateau_across_a_seam": 0, "background_max": 0}
    for k in pick:
        for name, hit in mw.window_classes(SHAPE, origin, wins[k], mw.MIDDLE).items():
            seen[name] += bool(hit)
    assert all(v >= 1 for v in seen.values()), (origin, seen)
