"""ops.local_maxima (pcseg_local_maxima_i32) at its tile seams, against the CPU oracle; every comparison is integer equality
of is_max, markers and counts, with markers = orc.label(orc.local_maxima(frame)).

The kernel decides candidates on a tile and a ring around it, flags plateaus from equal-valued non-candidates that may
lie in another tile, links candidates inside a tile and leaves the links across tiles to the border pass, hands the flag to
a root that may lie tiles away, keeps the candidates as one flat bit array over all frames of a batch, and numbers the
markers with a 16-lane scan per 1024 pixels.  Here all 19 683 ternary 3 x 3 windows lie over the tile corner at each of
its four positions inside the window (tests/maxima_windows.py; that the expectations are what the oracle says of the
whole frames, and that the oracle follows the definition, is tests/test_maxima_windows_cpu.py), plateaus are spoilt at
the far end from their roots, frames of a batch share words of the bit array, and the counting blocks are filled to the
densest.

INT_MIN as an image value is out of scope: the kernel's contract excludes it (it is the value of the cells outside the
frame and the key of a candidate of value 0), and no caller produces it.
"""
import functools

import numpy as np
import pytest

import maxima_windows as mw
import seam_patterns as sp
from oracle import oracle as orc

torch = pytest.importorskip("torch")
from device_helpers import shifted  # noqa: E402  (needs torch)

pytestmark = pytest.mark.gpu

FIELDS = ("is_max", "markers", "counts")
CORNER_SHAPE = (34, 66)  # 2 x 2 tiles, the corner at (32, 64); W % 4 != 0: one pixel per load
CORNER_ORIGINS = [(30, 62), (30, 63), (31, 62), (31, 63)]  # the corner at each interior grid point of a 3 x 3 window
MAX_PIXELS = 20_000_000  # per call


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")
    from particle_col_image_segmentation_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_frames_equal(got, exp, what, names=None, show=None, first=0):
    """torch.equal of two (B, ...) device tensors, naming the first frame that differs (``show``: the (row slice, column
    slice) of it that the message prints; the comparison is always of whole frames)."""
    if got.dim() == 1:
        got, exp = got[:, None], exp[:, None]
    if torch.equal(got, exp):
        return
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, tuple(got.shape), got.dtype, tuple(exp.shape), exp.dtype)
    bad = torch.nonzero((got != exp).flatten(1).any(1)).flatten()
    k = int(bad[0])
    g, e = got[k].cpu().numpy(), exp[k].cpu().numpy()
    where = ""
    if show is not None and g.ndim == 2 and (g != e).sum() == (g[show] != e[show]).sum():  # (else they also differ outside it)
        where = " (rows %d.., columns %d..)" % (show[0].start, show[1].start)
        g, e = g[show], e[show]
    with np.printoptions(linewidth=250, threshold=5000):
        pytest.fail("%s: %d of %d frames differ, first %s%s\n got:\n%s\n expected:\n%s" % (
            what, bad.numel(), got.shape[0], names[k] if names else first + k, where, g, e))


def compare(got, exp, what, names=None, show=None, first=0):
    """(is_max, markers, counts) against (is_max, markers, counts); a None on the left is an output that was not asked for."""
    for g, e, field in zip(got, exp, FIELDS):
        if g is not None:
            assert_frames_equal(g, e if torch.is_tensor(e) else dev(e), "%s %s" % (what, field), names, show, first)


def check_frames(ops, frames, what, names=None, also_shifted=False):
    """Whole frames (n, H, W) int32 in one call against the oracle on each; returns the device results."""
    x = dev(frames)
    got = ops.local_maxima(x)
    compare(got, mw.frames_answer(frames), what, names)
    if also_shifted:
        compare(ops.local_maxima(shifted(x)), got, what + " from a shifted base pointer", names)
    return got


# ============================================================================================================== windows
def check_windows(ops, family, shape, origin, background, values, also_shifted=False):
    """Every window of ``family`` at ``origin`` of a frame of ``shape`` and the role ``background``, under the map ``values``:
    is_max, markers and counts equal maxima_windows.expected.  Chunks of at most 20 Mpixels, compared on the device."""
    exp = mw.expected(family, shape, origin, background)
    wins = mw.windows(family)
    rlo, rhi, clo, chi = exp.box
    show = (slice(rlo, rhi), slice(clo, chi))
    chunk = min(8192, MAX_PIXELS // (shape[0] * shape[1]))
    for k0 in range(0, wins.shape[0], chunk):
        k1 = min(k0 + chunk, wins.shape[0])
        what = "%s %s at %s, background %d, values %s" % (family, shape, origin, background, values)
        x = dev(mw.value_frames(shape, origin, wins[k0:k1], background, values))
        got = ops.local_maxima(x)
        compare(got, (mw.spread(exp, "is_max", k0, k1), mw.spread(exp, "markers", k0, k1), exp.counts[k0:k1]), what, None, show, k0)
        if also_shifted:
            compare(ops.local_maxima(shifted(x)), got, what + " from a shifted base pointer", None, show, k0)


@pytest.mark.parametrize("origin", CORNER_ORIGINS, ids=str)
def test_ternary_windows_over_the_tile_corner(ops, origin):
    """All 19 683 windows over the corner of the 2 x 2 tiles of a 34 x 66 frame (the scalar load path), the background
    the middle role at value 0 -- the value whose key is INT_MIN.  At (31, 63) the window lies on the frame's last row
    and column.  44 Mpixels per origin, in 3 calls."""
    check_windows(ops, "ternary", CORNER_SHAPE, origin, mw.MIDDLE, mw.MAPS["zero_middle"])


@pytest.mark.parametrize("values", ["from_zero", "range_ends"])
def test_ternary_windows_under_other_maps(ops, values):
    """The same windows at (30, 62) with the low role at 0, and at the two ends of the int32 range the kernel admits."""
    check_windows(ops, "ternary", CORNER_SHAPE, (30, 62), mw.MIDDLE, mw.MAPS[values])


@pytest.mark.parametrize("background", [mw.LOW, mw.HIGH])
def test_ternary_windows_in_other_backgrounds(ops, background):
    """... and in a low background (never a maximum: the window's plateaus alone) and in a high one: the whole frame is
    one maximal plateau over all four tiles, with the window's holes in it."""
    check_windows(ops, "ternary", CORNER_SHAPE, (30, 62), background, mw.MAPS["zero_middle"])


def test_ternary_windows_through_the_16_byte_loads(ops):
    """All windows on the last row of a 34 x 128 frame, over the corner at (32, 64): full-width tiles of a frame whose
    width is a multiple of 4, the 16-byte load path from an aligned base pointer and the scalar one from a shifted one.
    The two results equal each other and the oracle."""
    check_windows(ops, "ternary", (34, 128), (31, 63), mw.MIDDLE, mw.MAPS["zero_middle"], also_shifted=True)


@pytest.mark.parametrize("shape", [(34, 66), (35, 67)])
def test_four_by_four_windows(ops, shape):
    """40 000 seeded 4 x 4 windows over the three roles at (30, 62): two pixels on either side of both seams.  35 x 67: an
    odd pixel count (the last word of the candidate bits and the last counting block are partial) and ragged last tiles."""
    check_windows(ops, ("random4", 40000, 40000 + shape[0]), shape, (30, 62), mw.MIDDLE, mw.MAPS["zero_middle"])


def test_output_switches(ops):
    """is_max alone, markers alone (each skips a pass: the mask kernel, the zero fill and the numbering) and both, on 4096
    of the 4 x 4 windows in the 35 x 67 frame: every output equals the one of the call that asked for both.  The counts
    come out of the numbering: without markers there are none, and none are handed back."""
    wins = mw.windows(("random4", 40000, 40035))[:4096]
    exp = mw.expected(("random4", 40000, 40035), (35, 67), (30, 62), mw.MIDDLE)
    x = dev(mw.value_frames((35, 67), (30, 62), wins, mw.MIDDLE, mw.MAPS["zero_middle"]))
    both = ops.local_maxima(x)
    compare(both, (mw.spread(exp, "is_max", 0, 4096), mw.spread(exp, "markers", 0, 4096), exp.counts[:4096]), "both")
    only_mask = ops.local_maxima(x, want_markers=False)
    assert only_mask[0] is not None and only_mask[1] is None and only_mask[2] is None
    compare(only_mask, both, "want_mask only")
    only_markers = ops.local_maxima(x, want_mask=False)
    assert only_markers[0] is None
    compare(only_markers, both, "want_markers only")
    compare(ops.local_maxima(x), both, "both, again")


def test_every_output_element_is_written(ops):
    """The entry with outputs that hold a poison pattern before the call (ops.local_maxima hands over fresh memory, which
    may happen to hold an earlier call's result): is_max and markers are written at every pixel -- the markers' zeros are
    written by the candidates pass, their numbers by the relabel pass -- and counts in every frame, whichever outputs are
    asked for.  On 4096 of the 4 x 4 windows and on the constant and the dense frames of 35 x 67."""
    shape = (35, 67)
    family = ("random4", 40000, 40035)
    exp = mw.expected(family, shape, (30, 62), mw.MIDDLE)
    whole = np.stack([mw.peak_frames(shape)["constant"]] + list(mw.dense_frames(shape).values()))
    cases = [("windows", mw.value_frames(shape, (30, 62), mw.windows(family)[:4096], mw.MIDDLE, mw.MAPS["zero_middle"]),
              (mw.spread(exp, "is_max", 0, 4096), mw.spread(exp, "markers", 0, 4096), exp.counts[:4096])),
             ("whole frames", whole, mw.frames_answer(whole))]
    for name, frames, want in cases:
        x = dev(frames)
        B, H, W = x.shape
        for want_mask, want_markers in ((True, True), (True, False), (False, True)):
            is_max = torch.full((B, H, W), 0xA5, dtype=torch.uint8, device="cuda") if want_mask else None
            markers = torch.full((B, H, W), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if want_markers else None
            counts = torch.full((B,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if want_markers else None
            ops._call("local_maxima_i32", x, is_max, markers, counts, B, H, W, ws=(B, H, W))
            compare((is_max, markers, counts), want, "%s into poisoned outputs (mask %s, markers %s)" % (name, want_mask, want_markers))


# ========================================================================================================= whole frames
@functools.lru_cache(None)
def spoilt_batch(shape):
    names, frames, last = [], [], []
    for name, f in sp.structured_frames(shape).items():
        res = mw.spoilt_at_the_far_end(f)
        if res is not None:
            names.append(name)
            frames.append(res[0])
            last.append(res[1])
    return names, np.stack(frames), last


@pytest.mark.parametrize("shape", [(33, 65), (65, 129), (97, 200)])
def test_plateaus_spoilt_at_the_far_end(ops, shape):
    """Every structured frame with one pixel beside the raster-last pixel of its highest class raised above it: the
    plateau that crossed every seam is no maximum any more, its root lies many tiles before the only pixel that can
    tell.  (All frames but the two constant ones, which have no such neighbour.)"""
    names, frames, last = spoilt_batch(shape)
    assert len(names) == 12 and "serpentine" in names and "checker" in names
    is_max = check_frames(ops, frames, "spoilt at the far end %s" % (shape,), names, also_shifted=True)[0]
    for k, (r, c) in enumerate(last):
        assert int(is_max[k, r, c]) == 0, names[k]


def test_constant_frames_with_one_pixel_changed(ops):
    """A constant 97 x 200 frame (4 x 4 tiles) with one pixel raised -- the only maximum -- and with one pixel lowered --
    everything else is one maximal plateau over all tiles: the pixel at the first and the last pixel, on a tile corner and
    inside a tile."""
    names, frames = mw.one_pixel_frames((97, 200), [(0, 0), (96, 199), (32, 64), (50, 100)])
    got = check_frames(ops, frames, "one pixel changed", names, also_shifted=True)
    assert got[2].tolist() == [1] * 8 and int(got[0][:4].sum()) == 4 and int(got[0][4:].sum()) == 4 * (97 * 200 - 1)


@pytest.mark.parametrize("shape", [(3, 65), (35, 67), (33, 65)])
def test_frames_that_share_candidate_words(ops, shape):
    """B = 6 frames of an odd pixel count: every word of the candidate bits at a frame boundary holds the end of one frame
    and the start of the next.  The frames alternate between a peak at the first pixel, one at the last pixel, both, and
    the constant frame, whose pixels are all candidates and none a maximum; in two orders.  Every frame equals the oracle
    and the same frame sent alone."""
    f = mw.peak_frames(shape)
    keys = list(f)
    alone = {k: ops.local_maxima(dev(f[k][None])) for k in keys}
    for start in (0, 3):
        names = [keys[(start + k) % 4] for k in range(6)]
        got = check_frames(ops, np.stack([f[k] for k in names]), "shared words %s" % (shape,), names)
        for j, k in enumerate(names):
            compare([g[j:j + 1] for g in got], alone[k], "shared words %s: frame %d (%s) against the frame alone" % (shape, j, k))


@pytest.mark.parametrize("shape", [(97, 200), (35, 67)])
def test_marker_numbering_at_full_density(ops, shape):
    """Single-pixel peaks at every (2 i, 2 j) -- a marker in every fourth pixel, some 256 in a 1024-pixel counting block
    and up to 32 in a thread's 64-pixel word; 2 x 2 plateaus at every (3 i, 3 j); peaks in the last, partial block only.
    B = 2 with differing frames, in three pairs."""
    f = mw.dense_frames(shape)
    for pair in (("peaks", "squares"), ("tail", "peaks"), ("squares", "tail")):
        got = check_frames(ops, np.stack([f[k] for k in pair]), "density %s" % (shape,), list(pair), also_shifted=True)
        for j, k in enumerate(pair):
            if k == "peaks":
                assert int(got[2][j]) == ((shape[0] + 1) // 2) * ((shape[1] + 1) // 2)


@pytest.mark.parametrize("shape", [(33, 65), (65, 129)])
def test_distance_maps_of_the_structured_masks(ops, shape):
    """The squared distance maps of the structured masks: the plateaus and ridges that the pipeline feeds in."""
    masks = sp.structured_frames(shape)
    frames = np.stack([orc.edt_sq(m > 0) for m in masks.values()])
    check_frames(ops, frames, "distance maps %s" % (shape,), list(masks), also_shifted=True)
