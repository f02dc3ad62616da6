"""Inputs that sit on the tile seams of the union-find labellings, and the host side of their checks (plain numpy).

The labelling kernels (csrc/ccl.hip, csrc/tile_ops.h, csrc/frontend.hip) work in 64 x 32 pixel tiles and join the tiles in a
border pass; the run-based variant works in 64-column x 128-row tiles of four 32-row bit words.  Both skip links that a
third pixel implies, by rules that change at tile corners, word seams and the first / last column of a tile.  The frames
made here put every local configuration on those seams:

* :func:`window_frames` places small windows (all 65 536 binary 4 x 4 windows, for instance) at a chosen origin of an
  otherwise empty frame; :func:`window_labels` is the oracle labelling of such windows, so that the expected label image
  of a frame is again ``window_frames`` of it.
* :func:`structured_frames` are whole-frame patterns that cross every seam of a shape; :func:`block_noise` are class
  fields for the fused front end, whose 5 x 5 median would erase one-pixel structure.
* :func:`run_partition` turns the (bit words, run parents) pair of ``dilated_runs`` into a per-pixel root image and
  :func:`same_partition` compares two label / root images as partitions.
"""
import collections

import numpy as np

from oracle import oracle as orc


# ------------------------------------------------------------------------------------------------------------ windows
def all_binary_windows(h=4, w=4):
    """All 2^(h w) binary windows, uint8 (2^(h w), h, w); bit k of the index is pixel k in raster order."""
    n = h * w
    idx = np.arange(1 << n, dtype=np.uint32)
    return ((idx[:, None] >> np.arange(n, dtype=np.uint32)[None, :]) & 1).astype(np.uint8).reshape(-1, h, w)


def random_windows(n, hi, seed, h=4, w=4):
    """``n`` seeded windows over {0 .. hi - 1}, uint8 (n, h, w)."""
    return np.random.default_rng(seed).integers(0, hi, (n, h, w)).astype(np.uint8)


def window_frames(shape, origin, windows):
    """Zero frames of ``shape`` (H, W), frame k holding ``windows[k]`` with its first pixel at ``origin`` (row, column):
    (n, H, W) of the windows' dtype.  A window may hang over the frame's lower / right edge; what hangs over is cut off.
    The frame is the window padded with zeros, so for a labelling in raster order the expected label image of the frames
    is ``window_frames(shape, origin, labels of the windows)`` (of the windows cut to the frame, if they hang over)."""
    windows = np.asarray(windows)
    H, W = shape
    r0, c0 = origin
    if not (0 <= r0 < H and 0 <= c0 < W):
        raise ValueError("origin %s outside the frame %s" % (origin, shape))
    h, w = min(windows.shape[1], H - r0), min(windows.shape[2], W - c0)
    out = np.zeros((windows.shape[0], H, W), windows.dtype)
    out[:, r0:r0 + h, c0:c0 + w] = windows[:, :h, :w]
    return out


def _dense_rank(lab):
    """Per cell of (n, h, w): every non-zero value replaced by its rank among the cell's distinct non-zero values."""
    n = lab.shape[0]
    flat = lab.reshape(n, -1)
    s = np.sort(flat, axis=1)
    first = np.ones(s.shape, bool)
    first[:, 1:] = s[:, 1:] != s[:, :-1]
    distinct = np.where(first, s, 0)  # each distinct value once, 0 elsewhere
    out = np.zeros(flat.shape, np.int32)
    for k in range(flat.shape[1]):  # (a loop over the few pixels of a cell keeps the temporaries at n x cell)
        out[:, k] = ((distinct > 0) & (distinct <= flat[:, k:k + 1])).sum(axis=1)
    out[flat == 0] = 0
    return out.reshape(lab.shape)


def window_labels(windows, connectivity=2, equal=False, radius=0, room=None):
    """The oracle's raster-order labelling of every window on its own: int32 (n, h + 2 radius, w + 2 radius).

    ``equal``: equal-valued components of the window's values (``orc.label`` of an integer image), else components of
    its non-zero pixels.  ``radius`` > 0: the window is first dilated with ``orc.binary_dilation_disk`` (non-zero pixels;
    the result then starts ``radius`` pixels above / left of the window).  ``room`` = (rows, columns): what of the
    (dilated) window lies inside the frame -- the rest is cut off BEFORE labelling, as the frame's edge does.

    One oracle call labels a whole mosaic of windows, each in a cell of its own with an empty rim: components cannot
    join across cells, and the oracle numbers components in raster order of their first pixels, which orders the
    components of one cell exactly as a labelling of the cell alone does.  So a cell's labels are the ranks of the
    mosaic's labels inside it (tests/test_label_seams_cpu.py checks this against one oracle call per window)."""
    windows = np.asarray(windows)
    n, h, w = windows.shape
    hh, ww = h + 2 * radius, w + 2 * radius
    ch, cw = hh + 1, ww + 1  # cell = (dilated) window + one empty row / column
    out = np.zeros((n, hh, ww), np.int32)
    per = 4096
    for k0 in range(0, n, per):
        chunk = windows[k0:k0 + per]
        m = chunk.shape[0]
        gw = int(np.ceil(np.sqrt(m)))
        gh = (m + gw - 1) // gw
        cells = np.zeros((gh * gw, ch, cw), windows.dtype)
        cells[:m, radius:radius + h, radius:radius + w] = chunk
        mosaic = cells.reshape(gh, gw, ch, cw).transpose(0, 2, 1, 3).reshape(gh * ch, gw * cw)
        if radius:
            mosaic = orc.binary_dilation_disk(mosaic != 0, radius).astype(np.uint8)
        if room is not None:  # cut every cell to the part of it that lies inside the frame
            keep = np.zeros((ch, cw), bool)
            keep[:room[0], :room[1]] = True
            mosaic = mosaic * np.tile(keep, (gh, gw)).astype(mosaic.dtype)
        lab = orc.label(mosaic.astype(np.int32) if equal else mosaic != 0, connectivity=connectivity)
        lab = lab.reshape(gh, ch, gw, cw).transpose(0, 2, 1, 3).reshape(gh * gw, ch, cw)[:m, :hh, :ww]
        out[k0:k0 + m] = _dense_rank(np.ascontiguousarray(lab))
    return out


# --------------------------------------------------------------------------------------------------- structured frames
def block_noise(shape, n_classes, offset, seed):
    """Classes 1 .. n_classes in 6 x 6 blocks whose grid starts ``offset`` (0 .. 5) pixels before the frame's first row and
    column: with the six offsets a block edge falls on every seam and one to five pixels beside it.  uint8 (H, W)."""
    H, W = shape
    rng = np.random.default_rng(seed)
    cls = rng.integers(1, n_classes + 1, ((H + offset) // 6 + 2, (W + offset) // 6 + 2)).astype(np.uint8)
    big = np.repeat(np.repeat(cls, 6, axis=0), 6, axis=1)
    return np.ascontiguousarray(big[offset:offset + H, offset:offset + W])


def structured_frames(shape):
    """Ordered dict name -> uint8 (H, W) class image (0 = background) of patterns that cross every seam of ``shape``.
    The boolean routes take ``> 0``, the equal-value route the values themselves."""
    H, W = shape
    r, c = np.mgrid[:H, :W]
    f = collections.OrderedDict()
    # a one-pixel serpentine: every other row, joined alternately at its right and its left end -- one 4-connected component
    # that crosses every vertical seam in every second row and every horizontal seam at a frame edge
    s = np.zeros(shape, np.uint8)
    s[::2, :] = 1
    s[1::4, W - 1] = 1
    s[3::4, 0] = 1
    f["serpentine"] = s
    # a comb: the first row and every other column
    s = np.zeros(shape, np.uint8)
    s[0, :] = 1
    s[:, ::2] = 1
    f["comb"] = s
    # diagonal stripes: period 2 is joined through NW and NE links (and through nothing under 4-connectivity: H W / 2
    # components), period 3 through NW links alone (diag) or NE links alone (anti)
    f["diag2"] = ((r - c) % 2 == 0).astype(np.uint8)
    f["anti2"] = ((r + c) % 2 == 1).astype(np.uint8)
    f["diag3"] = ((r - c) % 3 == 0).astype(np.uint8)
    f["anti3"] = ((r + c) % 3 == 0).astype(np.uint8)
    # a checkerboard of two classes: two 8-connected components of equal values, a full frame for the boolean routes
    f["checker"] = (1 + (r + c) % 2).astype(np.uint8)
    # isolated pixels at spacing 2: every fourth pixel is a root, the 1024-pixel counting blocks are full of roots
    s = np.zeros(shape, np.uint8)
    s[::2, ::2] = 1
    f["lattice"] = s
    # concentric one-pixel rings: classes 1 / 2 alternating, and class 1 alternating with background
    ring = np.minimum(np.minimum(r, H - 1 - r), np.minimum(c, W - 1 - c))
    f["rings12"] = (1 + ring % 2).astype(np.uint8)
    f["rings10"] = (1 - ring % 2).astype(np.uint8)
    f["full"] = np.ones(shape, np.uint8)
    f["empty"] = np.zeros(shape, np.uint8)
    s = np.zeros(shape, np.uint8)
    s[:, W // 2] = 1
    f["vline"] = s
    s = np.zeros(shape, np.uint8)
    s[H // 2, :] = 1
    f["hline"] = s
    return f


# ------------------------------------------------------------------------------------------------------ run components
def unpack_bits(bits, H):
    """32-row column words (.., ceil(H / 32), W) -> (bool mask (.., H, W), True if a bit of a row >= H is set)."""
    words = np.ascontiguousarray(bits).view(np.uint32)
    lead, (nch, W) = words.shape[:-2], words.shape[-2:]
    un = ((words[..., :, None, :] >> np.arange(32, dtype=np.uint32)[:, None]) & 1).astype(bool).reshape(lead + (nch * 32, W))
    return un[..., :H, :], bool(un[..., H:, :].any())


def run_partition(bits, run_parent, H):
    """What ``dilated_runs`` returns -> per-pixel root image, int32 like ``run_parent``: (root's linear index + 1) at the set
    pixels, 0 elsewhere.  ``bits``: (B, ceil(H / 32), W) or (ceil(H / 32), W) column words, ``run_parent``: (B, H, W) or
    (H, W), of which only the run-head entries are defined: a pixel's node is the top pixel of its vertical run INSIDE its
    32-row word, and its root the fixed point of the walk from there.  Only set pixels are touched (sparse frames cost
    what their pixels cost).  Raises ValueError on an entry that is not an earlier-or-equal pixel of the frame (roots are
    minima, so a walk descends)."""
    words = np.ascontiguousarray(bits).view(np.uint32)
    par = np.asarray(run_parent)
    single = words.ndim == 2
    if single:
        words, par = words[None], par[None]
    B, nch, W = words.shape
    if par.shape != (B, H, W) or nch != (H + 31) // 32:
        raise ValueError("bits %s / run_parent %s do not match H = %d" % (words.shape, par.shape, H))
    out = np.zeros((B, H, W), np.int32)
    fb, fch, fc = np.nonzero(words)
    if fb.size:
        w = words[fb, fch, fc]
        j = np.arange(32, dtype=np.uint32)
        on = ((w[:, None] >> j[None, :]) & 1).astype(bool)             # (words, 32)
        head = on.copy()
        head[:, 1:] &= ~on[:, :-1]                                      # a run starts where the bit below it is clear
        top = np.maximum.accumulate(np.where(head, j[None, :].astype(np.int64), -1), axis=1)  # top row of the run a bit is in
        k, jj = np.nonzero(on)
        row = fch[k] * 32 + jj
        if (row >= H).any():
            raise ValueError("a bit of a row >= H is set")
        b, col = fb[k], fc[k]
        cur = (fch[k] * 32 + top[k, jj]) * W + col
        flat = par.reshape(B, H * W)
        while True:
            nxt = flat[b, cur].astype(np.int64)
            if ((nxt < 0) | (nxt > cur)).any():
                raise ValueError("run_parent holds an entry that is not an earlier-or-equal pixel of its frame")
            if (nxt == cur).all():
                break
            cur = nxt
        out[b, row, col] = cur + 1
    return out[0] if single else out


def same_partition(a, b):
    """True if two label / root images ((H, W), or (B, H, W) frame by frame; > 0 = foreground) have the same foreground
    and induce the same components: the pairs (a, b) over the foreground are a one-to-one map."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    fg = a > 0
    if not np.array_equal(fg, b > 0):
        return False
    if not fg.any():
        return True
    frame = np.nonzero(fg)[0].astype(np.int64) if a.ndim == 3 else np.zeros(int(fg.sum()), np.int64)
    ka = frame * (int(a.max()) + 1) + a[fg].astype(np.int64)
    kb = frame * (int(b.max()) + 1) + b[fg].astype(np.int64)
    ua, ia = np.unique(ka, return_inverse=True)
    ub, ib = np.unique(kb, return_inverse=True)
    if ua.size != ub.size:
        return False
    pairs = np.unique(ia.astype(np.int64) * ub.size + ib)
    return pairs.size == ua.size
