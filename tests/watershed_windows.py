"""Small tie windows for the seams of the watershed, and the host side of their checks (the seam_patterns.py of
csrc/watershed.hip; no tests in here).

The watershed relaxes minimax levels on two 64 x 64 tilings half a tile apart, sweeps 32 x 32 quadrants cyclically (every
row of a sweep starts at another column), labels in 64 x 32 union-find tiles and has a second level and an exact flood
behind them.  Its seams lie at rows and columns 32 and 64.  A frame made here holds ONE small window of elevations and two
seed pixels; everything outside the window is masked out.

Why one window per frame: the reference pushes every seed with age 0 and equal (value, age) entries leave its binary heap
in an order that depends on the heap's shape, so isolated regions of one frame influence each other through the heap
(tests/test_watershed_seams_cpu.py pins a counter-example with nine windows in a frame).  With one window per frame the
heap only ever holds pixels of that window, and the reference's labels of the frame are its labels of the window alone,
placed at the window's position (the same file checks that on a sample).  So the expected labels of ~10^5 frames cost one
oracle call per 3 x 3 window.

Families (all float32, marker ids 1 and 2, the lower raster index of the two seeds gets id 1):

* ``A``   3 x 3 over the three levels {0.25, 0.5, 0.75}: all 3^9 = 19 683 windows, seeds at (0, 0) and (2, 2)
* ``B``   3 x 3 over the two levels {0.25, 0.75}: all 2^9 windows x all 36 pairs of seed pixels = 18 432
* ``C``   3 x 3 without ties: 4 096 seeded permutations of the nine values 1/16 .. 9/16, a seeded seed pair each
* ``Dh``  corridors 1 x 9 over the three levels, all 3^9, seeds at the two ends -- lakes in miniature, the longest tie paths
* ``Dv``  the same corridors as 9 x 1
"""
import collections
import functools
import itertools

import numpy as np

from oracle import oracle as orc

Family = collections.namedtuple("Family", "name values markers")  # values (N, h, w) float32, markers (N, h, w) int32

FAMILIES = ("A", "B", "C", "Dh", "Dv")
FAMILY_SIZES = {"A": 3 ** 9, "B": 2 ** 9 * 36, "C": 4096, "Dh": 3 ** 9, "Dv": 3 ** 9}
LEVELS3 = np.array([0.25, 0.5, 0.75], np.float32)
LEVELS2 = np.array([0.25, 0.75], np.float32)
OUTSIDE = np.float32(0.9)  # the frame's value outside the window (masked out)

SEAM_POSITIONS = [(32, 32), (32, 64), (64, 32), (64, 64)]  # window centres
PHASE_POSITIONS = [p for p in itertools.product((1, 32, 63, 64), repeat=2) if p not in SEAM_POSITIONS]
assert len(PHASE_POSITIONS) == 12


def _digits(base, n=9):
    """(base^n, n) uint8: digit k of the code is pixel k in raster order."""
    codes = np.arange(base ** n, dtype=np.int64)
    return ((codes[:, None] // base ** np.arange(n, dtype=np.int64)[None, :]) % base).astype(np.uint8)


def _seed_markers(n, hw, first, second):
    """int32 (n, h, w) with id 1 at raster index ``first[k]`` and id 2 at ``second[k]`` (first < second)."""
    h, w = hw
    first = np.broadcast_to(np.asarray(first, np.int64), (n,))
    second = np.broadcast_to(np.asarray(second, np.int64), (n,))
    assert (first < second).all()
    mk = np.zeros((n, h * w), np.int32)
    mk[np.arange(n), first] = 1
    mk[np.arange(n), second] = 2
    return mk.reshape(n, h, w)


@functools.lru_cache(None)
def family(name):
    """The Family of a name of FAMILIES; window k of it is ``values[k]``, ``markers[k]`` (do not write to them)."""
    if name == "A":
        values = LEVELS3[_digits(3)].reshape(-1, 3, 3)
        markers = _seed_markers(values.shape[0], (3, 3), 0, 8)
    elif name == "B":
        pairs = np.array(list(itertools.combinations(range(9), 2)), np.int64)  # 36 pairs, first < second
        values = np.repeat(LEVELS2[_digits(2)].reshape(-1, 3, 3), len(pairs), axis=0)  # window code = 36 * pattern + pair
        both = np.tile(pairs, (2 ** 9, 1))
        markers = _seed_markers(values.shape[0], (3, 3), both[:, 0], both[:, 1])
    elif name == "C":
        rng = np.random.default_rng(4096)
        perms = np.stack([rng.permutation(9) for _ in range(4096)])
        values = ((perms + 1).astype(np.float32) / np.float32(16)).reshape(-1, 3, 3)
        pairs = np.sort(np.stack([rng.choice(9, 2, replace=False) for _ in range(4096)]), axis=1)
        markers = _seed_markers(4096, (3, 3), pairs[:, 0], pairs[:, 1])
    elif name in ("Dh", "Dv"):
        hw = (1, 9) if name == "Dh" else (9, 1)
        values = LEVELS3[_digits(3)].reshape((-1,) + hw)
        markers = _seed_markers(values.shape[0], hw, 0, 8)
    else:
        raise ValueError(name)
    values = np.ascontiguousarray(values, np.float32)
    assert values.shape[0] == FAMILY_SIZES[name] and values.shape == markers.shape
    values.setflags(write=False)
    markers.setflags(write=False)
    return Family(name, values, markers)


@functools.lru_cache(None)
def window_expected(name):
    """int32 (N, h, w): the oracle's watershed of every window of a family ALONE (mask all ones), one call per window."""
    fam = family(name)
    ones = np.ones(fam.values.shape[1:], np.uint8)
    out = np.stack([orc.watershed(v, m, ones) for v, m in zip(fam.values, fam.markers)])
    out.setflags(write=False)
    return out


def mixed_subset(n, seed, names=("A", "B")):
    """A seeded sample of ``n`` windows drawn from the union of the families ``names`` (all of one window shape), without
    repetition: (values, markers, expected, codes) with codes[k] = (family name, window index)."""
    sizes = [FAMILY_SIZES[x] for x in names]
    pick = np.sort(np.random.default_rng(seed).choice(sum(sizes), n, replace=False))
    which = np.searchsorted(np.cumsum(sizes), pick, side="right")
    local = pick - np.concatenate([[0], np.cumsum(sizes)])[which]
    values = np.stack([family(names[f]).values[k] for f, k in zip(which, local)])
    markers = np.stack([family(names[f]).markers[k] for f, k in zip(which, local)])
    expected = np.stack([window_expected(names[f])[k] for f, k in zip(which, local)])
    return values, markers, expected, [(names[f], int(k)) for f, k in zip(which, local)]


# ------------------------------------------------------------------------------------------------------------- frames
def frame_shape(hw, vector):
    """The frame of a window shape: W % 4 == 0 (``vector``: the 16-byte tile loads and stores, ws_uf_label4_kernel) or
    W % 4 == 2 (the scalar ones, ws_uf_label_kernel).  3 x 3 windows: 66 x 68 / 66 x 66 -- a window centred at 64 lies at
    62 .. 65, against the frame's last row (and last column, at W = 66).  The corridors need 69 rows / columns for the
    seam at 64 to cut them in the middle (60 .. 68): 66 x 72 / 66 x 70 for 1 x 9 and 70 x 68 / 70 x 66 for 9 x 1."""
    h, w = hw
    H = 66 if h <= 3 else 70
    W = (68 if vector else 66) if w <= 3 else (72 if vector else 70)
    return H, W


def origin(centre, hw):
    """First (row, column) of a window of shape ``hw`` centred at ``centre``."""
    return centre[0] - hw[0] // 2, centre[1] - hw[1] // 2


def host_frame(values, markers, expected, shape, centre):
    """One frame on the host: (img float32, markers int32, mask uint8, expected int32 or None), each (H, W)."""
    H, W = shape
    h, w = values.shape
    r0, c0 = origin(centre, (h, w))
    assert 0 <= r0 and r0 + h <= H and 0 <= c0 and c0 + w <= W, (shape, centre, (h, w))
    img = np.full(shape, OUTSIDE, np.float32)
    mk, mask = np.zeros(shape, np.int32), np.zeros(shape, np.uint8)
    img[r0:r0 + h, c0:c0 + w] = values
    mk[r0:r0 + h, c0:c0 + w] = markers
    mask[r0:r0 + h, c0:c0 + w] = 1
    exp = None
    if expected is not None:
        exp = np.zeros(shape, np.int32)
        exp[r0:r0 + h, c0:c0 + w] = expected
    return img, mk, mask, exp


def device_frames(values, markers, expected, shape, centre):
    """The frames of (n, h, w) DEVICE tensors, assembled on the device by slice assignment (10^5 frames in numpy would take
    longer than the flood): (img float32, markers int32, mask uint8, expected int32), each (n, H, W)."""
    import torch
    H, W = shape
    n, h, w = values.shape
    r0, c0 = origin(centre, (h, w))
    assert 0 <= r0 and r0 + h <= H and 0 <= c0 and c0 + w <= W, (shape, centre, (h, w))
    dev = values.device
    img = torch.full((n, H, W), float(OUTSIDE), dtype=torch.float32, device=dev)
    mk = torch.zeros((n, H, W), dtype=torch.int32, device=dev)
    mask = torch.zeros((n, H, W), dtype=torch.uint8, device=dev)
    exp = torch.zeros((n, H, W), dtype=torch.int32, device=dev)
    img[:, r0:r0 + h, c0:c0 + w] = values
    mk[:, r0:r0 + h, c0:c0 + w] = markers
    mask[:, r0:r0 + h, c0:c0 + w] = 1
    exp[:, r0:r0 + h, c0:c0 + w] = expected
    return img, mk, mask, exp


def describe(what, code, values, markers, got, expected):
    """The text of a failure: ``what`` names family, position, width and mode, ``code`` the window."""
    with np.printoptions(linewidth=200):
        return "%s, window %s\n values:\n%s\n markers:\n%s\n got:\n%s\n expected:\n%s" % (what, code, values, markers, got, expected)


# ---------------------------------------------------------------------------------------------------- float specials
SPECIAL_VALUES = np.array([-np.inf, -3e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1e-40, 1.0, np.nextafter(np.float32(1), np.float32(2)),
                           3e38, np.inf], np.float32)
NEG_SUBNORMAL = np.float32(-1e-45)  # the largest negative subnormal: -2^-149
assert NEG_SUBNORMAL < 0 and NEG_SUBNORMAL == -np.nextafter(np.float32(0), np.float32(1))


def sparse_markers(shape, seed, every=97):
    """int32 (H, W): about one pixel in ``every`` carries a marker, ids 1 .. K in a seeded order (not raster order)."""
    rng = np.random.default_rng(seed)
    sel = rng.random(shape) < 1.0 / every
    mk = np.zeros(shape, np.int32)
    mk[sel] = rng.permutation(int(sel.sum())).astype(np.int32) + 1
    return mk


def signed_zero_frame(shape, seed):
    """(img, markers, mask): a frame over {-0.0, +0.0, 1e-40, 1} in 2 x 2 blocks -- -0.0 and +0.0 are ONE level, plateaus
    of the two run into each other; with -0.0 taken for a value below +0.0 (a key made from the bits alone) they split."""
    H, W = shape
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, 4, ((H + 1) // 2, (W + 1) // 2))
    vals = np.array([-0.0, 0.0, 1e-40, 1.0], np.float32)
    img = np.repeat(np.repeat(vals[pick], 2, axis=0), 2, axis=1)[:H, :W]
    return np.ascontiguousarray(img), sparse_markers(shape, seed + 1), np.ones(shape, np.uint8)


def ulp_frame(shape, seed, base=1.0):
    """(img, markers, mask): ``base`` + k ulp, k in 0 .. 3, in the upper half and -(``base`` + k ulp) in the lower, in 2 x 2
    blocks: neighbouring floats are four levels, not one."""
    H, W = shape
    rng = np.random.default_rng(seed)
    steps = [np.float32(base)]
    for _ in range(3):
        steps.append(np.nextafter(steps[-1], np.float32(np.inf)))
    steps = np.array(steps, np.float32)
    pick = rng.integers(0, 4, ((H + 1) // 2, (W + 1) // 2))
    img = np.repeat(np.repeat(steps[pick], 2, axis=0), 2, axis=1)[:H, :W].copy()
    img[H // 2:] *= np.float32(-1)
    return np.ascontiguousarray(img), sparse_markers(shape, seed + 1), np.ones(shape, np.uint8)


def specials_frame(shape, seed):
    """(img, markers, mask): SPECIAL_VALUES drawn per pixel, a seeded mask with a tenth of the pixels out."""
    rng = np.random.default_rng(seed)
    img = SPECIAL_VALUES[rng.integers(0, len(SPECIAL_VALUES), shape)]
    mask = (rng.random(shape) < 0.9).astype(np.uint8)
    return np.ascontiguousarray(img), sparse_markers(shape, seed + 1), mask


@functools.lru_cache(None)
def special_batch(shape):
    """The B = 8 frames of float specials of a shape: (names, img (8, H, W) float32, markers, mask, expected) with the
    oracle's labels per frame.  Frames 0 and 1 are the two that tests/test_watershed_seams_cpu.py pins as sensitive."""
    frames = [("signed_zeros", signed_zero_frame(shape, 11)), ("one_ulp", ulp_frame(shape, 21)),
              ("one_ulp_base_2^-126", ulp_frame(shape, 31, base=2.0 ** -126))]
    frames += [("specials#%d" % k, specials_frame(shape, 100 + k)) for k in range(5)]
    names = [n for n, _ in frames]
    img, mk, mask = (np.stack([f[j] for _, f in frames]) for j in range(3))
    exp = np.stack([orc.watershed(img[k], mk[k], mask[k]) for k in range(len(frames))])
    return names, img, mk, mask, exp
