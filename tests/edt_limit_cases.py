"""Inputs and expectations for the distance-transform family (csrc/edt.hip: edt_sq, edt_sq_lt, dilate_disk, fill_particle)
at the limits of its contract (include/pcseg.h, check_shape), without a device and without tests.

Group A: squared distances of 2^30 and more.  Group B: the widths at which an LDS stage changes or ends.  Group C:
fill_particle over radius, threshold and labels.  Group D: caps, class bytes of 64 and more, non-finite thresholds.
Everything is integer or byte valued: tests/test_edt_limits_cpu.py holds the expectations against the oracle and against
each other, tests/test_gpu_edt_limits.py compares the device with them by equality.  What is computed once is cached and
handed out read-only."""
import functools

import numpy as np

from oracle import oracle as orc


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


def capped(d2, cap):
    """include/pcseg.h: a squared distance above cap is reported as cap + 1 (in int64: cap + 1 may be 2^31 - 1)"""
    d2 = d2.astype(np.int64)
    out = np.where(d2 > cap, cap + 1, d2)
    assert out.max() < 2 ** 31
    return out.astype(np.int32)


# ================================================================================================ A: distances of 2^30 and more
# (257, 32768) is the smallest frame with a squared distance of 2^30 (pixel (256, 32767) from a zero pixel at (0, 0)); 512
# rows put 473 pixels there.  H * W = 2^24: far inside check_shape's H * W < 2^30
A_SHAPES = [(512, 32768), (32768, 512)]
A_FRAMES = ("one", "two", "ones")
A_BATCHES = (("one", "two"), ("ones", "one"))  # a frame without a zero pixel shares a launch with one that has one
A_CAPS = (50, 2 ** 30)
TWO_30 = 2 ** 30


def a_mask(shape, name):
    """uint8 (H, W), 1 except: "one" a zero pixel at (0, 0); "two" also at (H - 1, W - 1); "ones" none"""
    H, W = shape
    m = np.ones(shape, np.uint8)
    if name in ("one", "two"):
        m[0, 0] = 0
    if name == "two":
        m[H - 1, W - 1] = 0
    assert name in A_FRAMES
    return m


def a_closed_form(shape, name):
    """int64 (H, W): the squared distance to the nearest zero pixel of a_mask; "ones": to scipy's virtual pixel at (-1, 0)"""
    H, W = shape
    r = np.arange(H, dtype=np.int64)[:, None]
    c = np.arange(W, dtype=np.int64)[None, :]
    if name == "one":
        return r * r + c * c
    if name == "two":
        return np.minimum(r * r + c * c, (H - 1 - r) ** 2 + (W - 1 - c) ** 2)
    assert name == "ones"
    return (r + 1) ** 2 + c * c


@functools.lru_cache(maxsize=None)
def a_expected(shape, name):
    """the closed form as the int32 image the device must return"""
    d2 = a_closed_form(shape, name)
    assert d2.max() < 2 ** 31
    return frozen(d2.astype(np.int32))


# ======================================================================================= B: width limits of the LDS stages
# The row-block threshold pass (a reach above 31 pixels) stages 24 bytes per column (rounded up to four columns) beside 1056
# bytes of its own in the 163 840 bytes of a workgroup: include/pcseg.h states W <= 6780
REACH_MAX_W = 6780
B_ROWS = 9                       # two row blocks of eight, a single row in the second
B_REFUSED_W = (REACH_MAX_W + 1, 6828)   # the next width up; 6828 passed the guard that only counted the staged rows
B_BIT_W = (6828, 12001)          # the bit-word pass (reach <= 31) has no width bound
B_ROW_W = (10232, 10233)         # edt_sq: four rows per block fill the LDS exactly at 10232, one row per block from 10233 on
B_FILL = (3, 1, 3)               # (particle, cell, overlap)
B_FILL_REACH = {"row blocks": (20, 33), "bit words": (20, 2)}  # (radius, threshold): R2 = 1088, reach 32; R2 = 400, reach 20
B_DILATE_REACH = {"row blocks": 32, "bit words": 31}
EDT_CAP = 50


@functools.lru_cache(maxsize=None)
def b_class_frames(W):
    """uint8 (2, 9, W) class maps: particle pixels (3) with probability 0.0005, the rest cell (1) with probability 0.7, else
    0, 2, 67 (= 64 + 3), 131 (= 128 + 3) or 255; the second frame holds particle pixels at (0, 0) and (8, W - 1) only"""
    rng = np.random.default_rng(7000 + W)
    p, cell, _ = B_FILL
    x = np.where(rng.random((2, B_ROWS, W)) < 0.7, cell, rng.choice(np.array([0, 2, 64 + p, 128 + p, 255]), (2, B_ROWS, W))).astype(np.uint8)
    x[0][rng.random((B_ROWS, W)) < 0.0005] = p
    x[0, 4, W // 2] = p
    x[1, 0, 0] = x[1, B_ROWS - 1, W - 1] = p
    assert (x[1] == p).sum() == 2
    return frozen(x)


@functools.lru_cache(maxsize=None)
def b_dilate_expected(W, radius):
    """uint8 (2, 9, W): the oracle's disk dilation of the particle pixels of b_class_frames"""
    p = B_FILL[0]
    return frozen(np.stack([orc.binary_dilation_disk(f == p, radius) for f in b_class_frames(W)]).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def b_fill_expected(W, radius, threshold):
    """(out uint8 (2, 9, W), area int64 (2,)) of fill_reference on b_class_frames"""
    out, area = zip(*(fill_reference(f, *B_FILL, radius, threshold) for f in b_class_frames(W)))
    return frozen(np.stack(out), np.array(area, np.int64))


@functools.lru_cache(maxsize=None)
def b_row_masks(W):
    """uint8 (2, 9, W) masks: zero pixels with probability 0.0002 (a handful in a row: searches of hundreds of offsets), and a
    single zero pixel in column 0"""
    rng = np.random.default_rng(9000 + W)
    m = np.ones((2, B_ROWS, W), np.uint8)
    m[0][rng.random((B_ROWS, W)) < 0.0002] = 0
    m[1, 4, 0] = 0
    assert 4 <= (m[0] == 0).sum() <= 60
    return frozen(m)


@functools.lru_cache(maxsize=None)
def b_row_expected(W):
    return frozen(np.stack([orc.edt_sq(m) for m in b_row_masks(W)]))


# ================================================================================================ C: fill_particle's parameters
def fill_reference(ds, particle, cell, overlap, radius, threshold, d2=None):
    """fill_particle_area (include/pcseg.h) in numpy: (out uint8, area).  d2: orc.edt_sq(ds != particle) if at hand.  A frame
    without a particle pixel has scipy's virtual pixel in the distance term and an empty dilation"""
    is_particle = ds == particle
    if d2 is None:
        d2 = orc.edt_sq(~is_particle)
    d2 = d2.astype(np.int64)
    hit = (ds == cell) & ((d2 < threshold * threshold) | (is_particle.any() & (d2 <= radius * radius)))
    return np.where(hit, overlap, ds).astype(np.uint8), int(hit.sum())


# (70, 452): W % 4 == 0, one column block of the bit-word pass (448 columns) plus four columns, rows ending inside a bit
# word.  (45, 83): ragged, the byte path
C_SHAPES = [(70, 452), (45, 83)]
C_DEFAULT = (3, 1, 3)
C_PAIRS = [(0, 0), (0, 1), (0, 2), (1, 2), (3, 3), (20, 2),
           (2, 5),      # R2 = 24: not a square
           (20, 32),    # R2 = 1023: reach 31, not a square, the last of the bit-word pass
           (31, 32),    # reach 31
           (20, 33),    # R2 = 1088: reach 32, the first of the row-block pass
           (5, 40),     # R2 = 1599
           (32, 0), (180, 180)]
C_REFUSED_PAIRS = [(181, 2), (2, 181)]
C_TRIPLES = [(3, 1, 3),
             (0, 200, 255),
             (63, 128, 128),  # the output equals the input, the area still counts
             (5, 255, 0),
             (2, 2, 7)]       # every cell pixel is a particle pixel
C_TRIPLE_PAIRS = [(20, 2), (2, 5)]
C_FRAMES = ("disk", "points", "none", "last column")


def c_cases():
    """[(triple, pair)]: every pair with the default labels, every triple at C_TRIPLE_PAIRS"""
    out = [(C_DEFAULT, pair) for pair in C_PAIRS]
    out += [(t, pair) for t in C_TRIPLES for pair in C_TRIPLE_PAIRS if (t, pair) not in out]
    return out


def reach_of(radius, threshold):
    """floor(sqrt(max(radius^2, threshold^2 - 1))): 31 and less run on bit words, more on staged row blocks"""
    r2 = max(radius * radius, threshold * threshold - 1)
    d = int(np.sqrt(r2))
    while d * d > r2:
        d -= 1
    while (d + 1) * (d + 1) <= r2:
        d += 1
    return d


def c_particle(shape):
    """bool (4, H, W): where the particle pixels of C_FRAMES lie"""
    H, W = shape
    r, c = np.mgrid[:H, :W]
    s = np.zeros((4, H, W), bool)
    s[0] = (r - H // 2) ** 2 + (c - W // 3) ** 2 <= 36
    # single pixels either side of the seam between bit words (rows 31 | 32) and between column blocks (447 | 448)
    for rr, cc in [(31, 20), (32, W // 2), (10, 447), (50, 448), (0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]:
        s[1, rr % H, cc % W] = True
    s[3, H // 4:H // 2, W - 1] = True
    return s


@functools.lru_cache(maxsize=None)
def c_frames(shape, triple):
    """uint8 (4, H, W) class maps for the labels ``triple``: C_FRAMES.  The pixels off the particle are the cell label with
    probability 0.7, else one of 64 + p, 128 + p, 255 (never a particle: only bytes below 64 are looked up in the particle's bit),
    p + 1, the overlap label and cell ^ 128 (never a cell: it differs from the cell label in bit 7 alone, the bit that the
    four-pixel compare of the fill handles apart).  Where cell == particle the cell pixels are the particle pixels: the rest
    draws from that set alone"""
    p, cell, overlap = triple
    H, W = shape
    rng = np.random.default_rng(1000 * H + W + 17 * p + 31 * cell)
    others = np.array(sorted({64 + p, 128 + p, 255, p + 1, overlap, cell ^ 128} - {p}), np.uint8)
    x = rng.choice(others, (4, H, W))
    if cell != p:
        x = np.where(rng.random((4, H, W)) < 0.7, cell, x)
    x = np.where(c_particle(shape), p, x).astype(np.uint8)
    assert not (x[2] == p).any() and ((x[3] == p).any(axis=0) == (np.arange(W) == W - 1)).all()
    return frozen(x)


@functools.lru_cache(maxsize=None)
def c_d2(shape, triple):
    """int32 (4, H, W): the oracle's squared distance to the nearest particle pixel of c_frames"""
    p = triple[0]
    return frozen(np.stack([orc.edt_sq(f != p) for f in c_frames(shape, triple)]))


@functools.lru_cache(maxsize=None)
def c_expected(shape, triple, pair):
    """(out uint8 (4, H, W), area int64 (4,))"""
    out, area = zip(*(fill_reference(f, *triple, *pair, d2=d) for f, d in zip(c_frames(shape, triple), c_d2(shape, triple))))
    return frozen(np.stack(out), np.array(area, np.int64))


C_PRESET_AREA = np.array([5, 0, 1 << 40, -3], np.int64)  # overlap_area is accumulated into


# ================================================================================== D: caps, class bytes, non-finite thresholds
D_CAP_SHAPES = [(33, 70), (5, 1030)]
D_SMALL_CAPS = [0, 1, 2, 3, 4, 5, 8, 9, 10, 15, 16, 17, 48, 49, 50]
D_CAPS = D_SMALL_CAPS + [2 ** 24 + 1, 2 ** 30, 2 ** 31 - 2, 2 ** 31 - 1]
D_CAP_FRAMES = ("sparse", "corner", "none")


@functools.lru_cache(maxsize=None)
def d_cap_masks(shape):
    """uint8 (3, H, W): zero pixels with probability 0.003, one zero pixel at (H - 1, 0), none"""
    H, W = shape
    rng = np.random.default_rng(500 * H + W)
    m = np.ones((3, H, W), np.uint8)
    m[0][rng.random(shape) < 0.003] = 0
    m[0, H // 2, W // 2] = 0
    m[1, H - 1, 0] = 0
    return frozen(m)


@functools.lru_cache(maxsize=None)
def d_cap_d2(shape):
    return frozen(np.stack([orc.edt_sq(m) for m in d_cap_masks(shape)]))


D_SHAPE = (33, 70)
D_RADII = (2, 32)
D_VALUE_BITS = (1 << 1, (1 << 1) | (1 << 5), 1 << 63, 0)
D_RARE_BYTES = (1, 2, 3, 4, 5, 63)                                   # members of some value set: a few pixels each
D_COMMON_BYTES = (0, 64, 65, 66, 67, 68, 69, 127, 128, 129, 133, 191, 255)  # never a member: v >= 64 has no bit (127, 191, 255: v % 64 == 63)


def in_value_set(x, value_bits):
    """bool: bytes below 64 whose bit is set in value_bits"""
    x = x.astype(np.uint64)
    return (x < 64) & (((np.uint64(value_bits) >> np.minimum(x, np.uint64(63))) & np.uint64(1)) != 0)


@functools.lru_cache(maxsize=None)
def d_class_bytes():
    """uint8 (4, 33, 70): D_COMMON_BYTES with a sprinkle of D_RARE_BYTES (probability 0.004 together); the last frame holds
    exactly one pixel of each rare byte, byte 1 at a corner"""
    H, W = D_SHAPE
    rng = np.random.default_rng(4242)
    x = rng.choice(np.array(D_COMMON_BYTES, np.uint8), (4, H, W))
    rare = rng.random((3, H, W)) < 0.004
    x[:3][rare] = rng.choice(np.array(D_RARE_BYTES, np.uint8), int(rare.sum()))
    for b in range(3):  # every frame holds a member of every value set
        x[b, 16 - 8 * b, 35 + 15 * b], x[b, 8 * b, 69 - 30 * b], x[b, 32, 10 + 20 * b] = 1, 5, 63
    for k, v in enumerate(D_RARE_BYTES):
        x[3, (H - 1) * (k % 2), k * 13] = v
    return frozen(x.astype(np.uint8))


@functools.lru_cache(maxsize=None)
def d_dilate_expected(value_bits, radius):
    return frozen(np.stack([orc.binary_dilation_disk(in_value_set(f, value_bits), radius) for f in d_class_bytes()]).astype(np.uint8))


D_THRESHOLDS = (0.0, -0.0, float("inf"), float("-inf"), 0.5)


@functools.lru_cache(maxsize=None)
def d_float_frames():
    """float32 (2, 33, 70): uniform in [-1, 1) with NaN, +inf, -inf, -0.0, 0.0 and subnormals of both signs sprinkled in
    (probability 0.04 each)"""
    H, W = D_SHAPE
    rng = np.random.default_rng(77)
    x = rng.uniform(-1, 1, (2, H, W)).astype(np.float32)
    tiny = np.float32(1e-45)  # the smallest subnormal
    specials = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, tiny, -tiny, np.float32(1e-39), np.float32(-1e-39)], np.float32)
    pick = rng.integers(0, 25, (2, H, W))  # 0 .. 8: a special value
    x = np.where(pick < len(specials), specials[np.minimum(pick, len(specials) - 1)], x).astype(np.float32)
    return frozen(x)


@functools.lru_cache(maxsize=None)
def d_float_expected(threshold):
    """(mask uint8 (2, 33, 70) = img < threshold in float32, d2 int32 = the oracle's transform of it)"""
    with np.errstate(invalid="ignore"):
        mask = (d_float_frames() < np.float32(threshold)).astype(np.uint8)
    return frozen(mask, np.stack([orc.edt_sq(m) for m in mask]))
