"""The serpentine lake: frames built to leave both fixed points of the watershed to their tail kernels (the GPU side is
test_gpu_watershed_tails.py).  Here the frames and what the reference makes of them are pinned without a device.

A one-pixel corridor winds over the whole frame (horizontal runs every 8 rows, joined alternately at the right and left
end); the mask is the corridor only.  Its first pixel A (0.1) carries marker 1, its last pixel B (0.2) marker 2; the pixels
next to them, q1 and q2, are 0.5 and everything between lies below 0.5 in no order along the path.  So the lake between q1
and q2 has the minimax level L = 0.5 throughout and is entered from both ends: the first level's component holds two marker
ids, and the second level has to carry K2 = L(A) from q1 along the whole corridor -- one round per tile crossing, dozens
against a handful of grid rounds -- as the first level has to carry L itself.  The reference floods the lake from q1 (pushed
before q2): everything is labelled 1 except q2 and B."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc

# 3 x 3 tiles of 64 x 64; the second shape has W % 4 != 0 (scalar tile loads and stores, the per-pixel label pass)
SHAPES = [(192, 192), (192, 190)]
CORRIDOR = {(192, 192): 4386, (192, 190): 4340}
LAKE_FRAMES = (0, 2)


def corridor(H, W):
    """The corridor's pixels in path order (the construction of test_watershed_long_winding_path_finishes_in_the_tail_kernel)."""
    rows = list(range(4, H - 4, 8))
    order = []
    for k, r in enumerate(rows):
        cols = range(4, W - 4) if k % 2 == 0 else range(W - 5, 3, -1)
        order += [(r, c) for c in cols]
        if k + 1 < len(rows):
            cend = W - 5 if k % 2 == 0 else 4
            order += [(rr, cend) for rr in range(r + 1, rows[k + 1])]
    return order


def serpentine_lake(H, W):
    order = corridor(H, W)
    n = len(order)
    img = np.full((H, W), 0.9, np.float32)
    mask = np.zeros((H, W), bool)
    markers = np.zeros((H, W), np.int32)
    for i, p in enumerate(order):
        mask[p] = True
        img[p] = 0.3 + 0.1 * ((i * 7919) % n) / n
    img[order[0]], markers[order[0]] = 0.1, 1    # A
    img[order[1]] = 0.5                          # q1
    img[order[-2]] = 0.5                         # q2
    img[order[-1]], markers[order[-1]] = 0.2, 2  # B
    return img, markers, mask


def noise_frame(H, W, seed):
    """Tie-free: every pixel its own value (H * W < 2^24, so float32 keeps them apart)."""
    rng = np.random.default_rng(seed)
    img = (rng.permutation(H * W).reshape(H, W) / float(H * W)).astype(np.float32)
    mask = rng.random((H, W)) < 0.8
    markers = np.zeros((H, W), np.int32)
    for k in range(1, 30):
        r, c = rng.integers(0, H), rng.integers(0, W)
        if mask[r, c]:
            markers[r, c] = k
    return img, markers, mask


@functools.lru_cache(maxsize=None)
def batch(shape):
    """(img, markers, mask) of B = 3 frames -- the lake in frames 0 and 2, noise between them -- and the reference's labels."""
    H, W = shape
    frames = [serpentine_lake(H, W), noise_frame(H, W, 5), serpentine_lake(H, W)]
    img, markers, mask = (np.stack([f[k] for f in frames]) for k in range(3))
    ref = np.stack([orc.watershed(img[b], markers[b], mask[b]) for b in range(3)])
    for a in (img, markers, mask, ref):
        a.setflags(write=False)
    return img, markers, mask, ref


@pytest.mark.parametrize("shape", SHAPES)
def test_reference_floods_the_lake_from_its_first_entry(shape):
    H, W = shape
    order = corridor(H, W)
    n = len(order)
    assert n == CORRIDOR[shape]
    img, markers, mask, ref = batch(shape)
    for b in LAKE_FRAMES:
        assert int(mask[b].sum()) == n and float(img[b][mask[b]].max()) == 0.5
        assert int((ref[b] == 1).sum()) == n - 2 and int((ref[b] == 2).sum()) == 2
        assert ref[b][order[-2]] == 2 and ref[b][order[-1]] == 2
        assert not ref[b][~mask[b]].any()  # nothing outside the mask is labelled
    assert len(np.unique(img[1])) == H * W
