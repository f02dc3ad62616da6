"""Small plateau windows for the tile seams of the local maxima, and the host side of their checks (the seam_patterns.py
of pcseg_local_maxima_i32, csrc/ccl.hip; no tests in here).

The kernel works in 64 x 32 pixel tiles.  Whether a pixel is a candidate (no higher 8-neighbour) is decided for the tile and
a one-pixel ring around it; a candidate beside an equal-valued non-candidate flags its plateau; links between candidates
are made inside the tile only and across tiles by the border pass; the flag reaches the plateau's root, which may lie in
another tile, in a pass of its own.  A frame made here holds ONE small window over the three roles low / middle / high
(0 / 1 / 2) in a frame that is otherwise of one role, the background: with the window over a tile corner, every plateau
configuration of the window meets the seams, and the background plateau -- rooted at the frame's first pixel -- is
spoilt, or not, by pixels of another tile.

Roles become values under a strictly increasing map (lo, mid, hi); a local maximum only depends on the order of the
values, so the expectation of a frame is the same under every map (tests/test_maxima_windows_cpu.py checks it) and is
computed once per (windows, shape, origin, background), on a crop around the window: the frame outside the crop is
background, one plateau with the crop's margin, and carries that plateau's verdict and marker.
"""
import collections
import functools

import numpy as np

import seam_patterns as sp
from oracle import oracle as orc

LOW, MIDDLE, HIGH = 0, 1, 2
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
# the value maps: the background (middle) is 0, the value whose key inside the kernel is INT_MIN; plain small values; and the
# ends of the range the kernel admits (INT_MIN itself is the kernel's out-of-frame value: not an image value)
MAPS = collections.OrderedDict([("zero_middle", (-1, 0, 1)), ("from_zero", (0, 1, 2)),
                                ("range_ends", (INT_MIN + 1, INT_MAX - 1, INT_MAX))])
TILE = (32, 64)  # rows, columns of a tile
MARGIN = 2       # background pixels the crop keeps around the window, where the frame has them


@functools.lru_cache(None)
def all_ternary_windows():
    """All 3^9 = 19 683 windows of 3 x 3 pixels over the roles {0, 1, 2}, uint8 (19 683, 3, 3); digit k (base 3) of the
    index is pixel k in raster order.  Do not write to it."""
    codes = np.arange(3 ** 9, dtype=np.int64)
    wins = ((codes[:, None] // 3 ** np.arange(9, dtype=np.int64)[None, :]) % 3).astype(np.uint8).reshape(-1, 3, 3)
    wins.setflags(write=False)
    return wins


@functools.lru_cache(None)
def windows(family):
    """The windows of a family: "ternary" (all_ternary_windows) or ("random4", n, seed): ``n`` seeded 4 x 4 windows over
    the three roles (seam_patterns.random_windows)."""
    if family == "ternary":
        return all_ternary_windows()
    kind, n, seed = family
    if kind != "random4":
        raise ValueError(family)
    wins = sp.random_windows(n, 3, seed)
    wins.setflags(write=False)
    return wins


def role_frames(shape, origin, wins, background):
    """uint8 (n, H, W): frames of the role ``background`` with window k's roles at ``origin`` (what hangs over the frame's
    lower / right edge is cut off, as in seam_patterns.window_frames)."""
    shifted = np.asarray(wins).astype(np.int8) - np.int8(background)  # window_frames pads with 0 = the background
    return (sp.window_frames(shape, origin, shifted) + np.int8(background)).astype(np.uint8)


def value_frames(shape, origin, wins, background, values):
    """int32 (n, H, W): role_frames under the strictly increasing map ``values`` = (lo, mid, hi)."""
    lo, mid, hi = values
    if not (INT_MIN < lo < mid < hi <= INT_MAX):
        raise ValueError("not a strictly increasing map above INT_MIN: %s" % (values,))
    return np.array(values, np.int32)[role_frames(shape, origin, wins, background)]


def crop_box(shape, origin, hw):
    """(first row, end row, first column, end column) of the crop around a window of shape ``hw`` at ``origin``: the
    window cut to the frame plus MARGIN background pixels on every side, cut to the frame again -- where the window
    touches (or comes within MARGIN of) the frame's edge the crop ends at the frame's own edge, because an edge is not a
    ring of background: a pixel there has fewer neighbours, none of them higher."""
    H, W = shape
    r0, c0 = origin
    h, w = min(hw[0], H - r0), min(hw[1], W - c0)
    if not (0 <= r0 < H and 0 <= c0 < W and h < H and w < W):
        # (a window as high or as wide as the frame would cut the background in two plateaus)
        raise ValueError("window %s at %s does not leave one background around it in %s" % (hw, origin, shape))
    return max(r0 - MARGIN, 0), min(r0 + h + MARGIN, H), max(c0 - MARGIN, 0), min(c0 + w + MARGIN, W)


Expected = collections.namedtuple("Expected", "shape box is_max markers counts outside_max outside_marker")
Expected.__doc__ = """The oracle's answer for n frames of one window each: ``is_max`` uint8 and ``markers`` int32 (n, crop
rows, crop columns) inside ``box`` (crop_box), ``outside_max`` uint8 (n,) and ``outside_marker`` int32 (n,) for every
pixel outside it, ``counts`` int32 (n,)."""


def window_expected(shape, origin, wins, background, values=(0, 1, 2)):
    """Expected of the frames ``value_frames(shape, origin, wins, background, values)``: is_max = orc.local_maxima and
    markers = orc.label(is_max) of every frame, from one orc.local_maxima call per crop.

    The crop's maxima are labelled in the crop's raster order (seam_patterns.window_labels: one labelling of a mosaic of
    crops), and that IS the frame's order: a pixel's frame index grows with its crop index, so plateaus inside the crop
    keep their order; only the background plateau has pixels outside the crop, and its first pixel in the frame -- the
    frame's first pixel outside the window -- lies in the same row, before or at its first pixel in the crop, with no
    window pixel between the two."""
    wins = np.asarray(wins)
    n = wins.shape[0]
    box = crop_box(shape, origin, wins.shape[1:])
    rlo, rhi, clo, chi = box
    ch, cw = rhi - rlo, chi - clo
    inner = (origin[0] - rlo, origin[1] - clo)
    crops = value_frames((ch, cw), inner, wins, background, values)  # (crop_box: larger than the window on one side at least)
    is_max = np.empty((n, ch, cw), np.uint8)
    for k in range(n):
        is_max[k] = orc.local_maxima(crops[k])
    lab = sp.window_labels(is_max).reshape(n, ch * cw)
    # a crop pixel outside the window: background, of one plateau with everything outside the crop
    in_window = np.zeros((ch, cw), bool)
    in_window[inner[0]:inner[0] + wins.shape[1], inner[1]:inner[1] + wins.shape[2]] = True
    pick = int(np.flatnonzero(~in_window.ravel())[0])
    return Expected(tuple(shape), box, is_max, lab.reshape(n, ch, cw), lab.max(axis=1).astype(np.int32),
                    is_max.reshape(n, -1)[:, pick].copy(), lab[:, pick].copy())


@functools.lru_cache(None)
def expected(family, shape, origin, background):
    """window_expected of a family of ``windows``, kept: it holds under every value map."""
    return window_expected(shape, origin, windows(family), background)


def spread(exp, field, k0=0, k1=None):
    """The whole frames k0 .. k1 - 1 of ``field`` ("is_max" or "markers") of an Expected: (k1 - k0, H, W)."""
    crop = getattr(exp, field)[k0:k1]
    outside = (exp.outside_max if field == "is_max" else exp.outside_marker)[k0:k1]
    rlo, rhi, clo, chi = exp.box
    out = np.empty((crop.shape[0],) + exp.shape, crop.dtype)
    out[:] = outside[:, None, None]
    out[:, rlo:rhi, clo:chi] = crop
    return out


def frame_answer(img):
    """(is_max uint8, markers int32, count) of one whole frame, straight from the oracle."""
    is_max = orc.local_maxima(img)
    markers, count = orc.label(is_max, return_num=True)
    return is_max.astype(np.uint8), markers, count


def frames_answer(frames):
    """frame_answer of every frame of (n, H, W): (is_max (n, H, W) uint8, markers (n, H, W) int32, counts (n,) int32)."""
    res = [frame_answer(f) for f in frames]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.array([r[2] for r in res], np.int32)


# ------------------------------------------------------------------------------------------------------- whole frames
def spoilt_at_the_far_end(frame):
    """int32 copy of a class image with ONE pixel changed: an 8-neighbour of the raster-last pixel of the highest class,
    of another value, is set to that class + 1 -- the last of the neighbours in raster order.  The highest class's plateau
    through that pixel is then no maximum, and only its last pixel can tell.  Returns (frame, (row, column) of that last
    pixel), or None where the last pixel has no neighbour of another value (a constant frame, for one)."""
    f = np.asarray(frame).astype(np.int32)
    H, W = f.shape
    top = int(f.max())
    r, c = (int(v) for v in np.argwhere(f == top)[-1])
    for dr, dc in ((1, 1), (1, 0), (1, -1), (0, 1), (0, -1), (-1, 1), (-1, 0), (-1, -1)):
        rr, cc = r + dr, c + dc
        if 0 <= rr < H and 0 <= cc < W and f[rr, cc] != top:
            f[rr, cc] = top + 1
            return f, (r, c)
    return None


def one_pixel_frames(shape, places, base=7):
    """(names, int32 (2 len(places), H, W)): a constant frame with the pixel at each of ``places`` raised by one (that
    pixel is the only maximum) and lowered by one (everything else is one maximal plateau with a hole)."""
    names, frames = [], []
    for step in (1, -1):
        for r, c in places:
            f = np.full(shape, base, np.int32)
            f[r, c] += step
            names.append("%+d at (%d, %d)" % (step, r, c))
            frames.append(f)
    return names, np.stack(frames)


def peak_frames(shape):
    """Ordered dict of four int32 frames over {0, 1}: a single peak at the first pixel, one at the last pixel, both, and
    the constant frame -- which has no maxima although every pixel of it is a candidate."""
    H, W = shape
    f = collections.OrderedDict((k, np.zeros(shape, np.int32)) for k in ("first", "last", "both", "constant"))
    f["first"][0, 0] = f["both"][0, 0] = 1
    f["last"][H - 1, W - 1] = f["both"][H - 1, W - 1] = 1
    return f


def dense_frames(shape, block=1024):
    """Ordered dict of three int32 frames over {0, 1} for the marker numbering: ``peaks`` -- single-pixel peaks at every
    (2 i, 2 j), the densest isolated maxima there can be; ``squares`` -- 2 x 2 plateaus at every (3 i, 3 j); ``tail`` -- the
    peaks that lie in the frame's last, partial counting block of ``block`` pixels, and nothing before it."""
    H, W = shape
    r, c = np.mgrid[:H, :W]
    f = collections.OrderedDict()
    f["peaks"] = ((r % 2 == 0) & (c % 2 == 0)).astype(np.int32)
    f["squares"] = ((r % 3 < 2) & (c % 3 < 2)).astype(np.int32)
    if (H * W) % block == 0:
        raise ValueError("%s has no partial last block" % (shape,))
    f["tail"] = f["peaks"] * (r * W + c >= (H * W) // block * block)
    return f


# ------------------------------------------------------------------------------------------------ what the windows reach
def tile_of(r, c):
    return r // TILE[0], c // TILE[1]


def window_classes(shape, origin, win, background):
    """What one window does at ``origin``, from the oracle on the whole frame: a dict of booleans.

    * ``background_max``: the background plateau is a maximum
    * ``spoilt_from_another_tile``: the background plateau is no maximum, and every pixel of it that has a higher
      neighbour, and every pixel of it beside such a pixel (the ones that carry the flag), lies in another tile than the
      frame's first pixel -- the plateau's root
    * ``joined_across_a_seam``: window pixels of the background's role belong to the background plateau, it is a maximum
      and those pixels lie in more than one tile
    * ``own_plateau_across_a_seam``: a maximal plateau of two or more pixels lies inside the window, apart from the
      background plateau, in more than one tile"""
    frame = value_frames(shape, origin, win[None], background, (0, 1, 2))[0]
    H, W = shape
    plateaus = orc.label(frame)
    is_max, markers, _ = frame_answer(frame)
    h, w = min(win.shape[0], H - origin[0]), min(win.shape[1], W - origin[1])
    outside = np.ones(shape, bool)
    outside[origin[0]:origin[0] + h, origin[1]:origin[1] + w] = False
    ref = tuple(np.argwhere(outside)[0])
    bg = plateaus == plateaus[ref]
    out = {"background_max": bool(is_max[ref])}
    pad = np.pad(frame, 1, constant_values=INT_MIN)
    higher = np.zeros(shape, bool)
    near = np.zeros(shape, bool)
    for dr in (0, 1, 2):
        for dc in (0, 1, 2):
            higher |= pad[dr:dr + H, dc:dc + W] > frame
    sees = bg & higher
    padded = np.pad(sees, 1)
    for dr in (0, 1, 2):
        for dc in (0, 1, 2):
            near |= padded[dr:dr + H, dc:dc + W]
    involved = np.argwhere(bg & near)
    out["spoilt_from_another_tile"] = bool(sees.any()) and all(tile_of(r, c) != (0, 0) for r, c in involved)
    joined = np.argwhere(bg & ~outside)
    out["joined_across_a_seam"] = out["background_max"] and len({tile_of(r, c) for r, c in joined}) > 1
    own = False
    for m in np.unique(markers[~outside & (markers > 0)]):
        px = np.argwhere(markers == m)
        if m != markers[ref] and len(px) >= 2 and len({tile_of(r, c) for r, c in px}) > 1:
            own = True
    out["own_plateau_across_a_seam"] = own
    return out
