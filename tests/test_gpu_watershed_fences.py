"""Fences of the watershed's union-find walks: a corrupted parent image raises the frame's flag,
never gives wrong labels and never makes a pass touch another frame.

pcseg_watershed4_f32 takes test-only mode bits (include/pcseg.h, PCSEG_WS_POISON_*) that overwrite up to four root entries
of its internal parent image per frame between two passes of the label assignment.  The frame index decides the poison
(b % 6): 0 none (control frame), 1 2000000000, 2 -1, 3 INT_MIN, 4 a two-cycle of two roots, 5 H*W + 5.  With B = 12 every
kind occurs twice in one launch, and each control frame after the first follows a kind-5 frame (past its end).

  mode 2 (parallel flood only): every frame the poison reached comes back flagged; control frames are bitwise equal to
          the same call without the poison bit; a frame with flag 0 equals the sequential reference flood.
  mode 0: every frame equals the reference (poisoned frames are recomputed by the exact flood).
"""
import numpy as np
import pytest

from oracle import oracle as orc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

B = 12
KIND_PAST_END = 5  # H*W + 5: past the frame, below the non-seed offset of the virtual indices

# (H, W) and the label pass the first level takes for it (watershed.hip, assign_labels)
SHAPES = [
    pytest.param((64, 128), id="label4-64x128"),         # W % 4 == 0: ws_uf_label4_kernel
    pytest.param((96, 96), id="label4-96x96"),           # W % 4 == 0: ws_uf_label4_kernel
    pytest.param((70, 100), id="label4-ragged-70x100"),  # W % 4 == 0, neither 64 nor 32 x 64 tiles divide it
    pytest.param((67, 130), id="label-ragged-67x130"),   # W % 4 != 0: ws_uf_label_kernel<UF_OPTIMISTIC>, ragged tiles
]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")
    from particle_col_image_segmentation_amd import ops as _ops
    return _ops


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == bool:
        a = a.astype(np.uint8)
    return torch.from_numpy(a).cuda()


def _smooth(img):
    for _ in range(3):
        img = (img + np.roll(img, 1, 1) + np.roll(img, -1, 1) + np.roll(img, 1, 2) + np.roll(img, -1, 2)) / 5
    return img


def _frames(shape, seed, ties):
    """B frames.  ties=False: smooth basins, dense mask -- large components that cross every tile seam.  ties=True: quantised
    grey levels (plateaus, lakes, equal-valued seeds), as in test_gpu_primitives.py::test_watershed_proof_holds_on_adversarial_ties:
    most frames go on to the second level, which resolves most of them."""
    H, W = shape
    rng = np.random.default_rng(seed)
    img = rng.random((B, H, W))
    if ties:  # 200 grey levels, smoothed a little so that lakes (pits without seeds) exist at every level
        img = np.floor(img * 200) / 200
        img = (img + np.roll(img, 1, 1) + np.roll(img, 1, 2)) / 3
        pk, pm = 0.002, 1.0
    else:
        img = _smooth(img)
        pk, pm = 0.004, 0.97
    img = img.astype(np.float32)
    mask = rng.random((B, H, W)) < pm
    mk = np.zeros((B, H, W), np.int32)
    for b in range(B):
        sel = rng.random((H, W)) < pk
        sel[H // 2, W // 2] = True  # at least one marker
        mk[b][sel] = rng.permutation(int(sel.sum())).astype(np.int32) + 1
        if b % 3 == 0:
            mk[b, 1:3, 1:4] = 500  # a multi-pixel marker
    for b in range(B):
        if b % 6 == KIND_PAST_END:
            # the frame's last pixel unreachable: a chain that ends at H*W + 5 reads -1 there (clamped) and stops on the
            # out-of-frame node instead of walking on ...
            mask[b, H - 1, W - 1] = False
            if b + 1 < B:  # ... and a stray write at that root would hit pixel 5 of the next (control) frame: a seed
                mk[b + 1, 0, 5] = 900
                mask[b + 1, 0, 5] = True
    return img, mk, mask


def _run(ops, img, mk, mask, mode):
    out, flags = ops.watershed(_dev(img), _dev(mk), _dev(mask), mode=mode)
    torch.cuda.synchronize()
    return out.cpu().numpy(), flags.cpu().numpy()


def _refs(img, mk, mask):
    return [orc.watershed(img[b], mk[b], mask[b]) for b in range(B)]


def _first_level(ops, stage, shape, seed):
    img, mk, mask = _frames(shape, seed, ties=False)
    ref = _refs(img, mk, mask)
    clean, clean_f = _run(ops, img, mk, mask, 2)
    got, got_f = _run(ops, img, mk, mask, 2 | stage)
    unflagged = [b for b in range(B) if b % 6 != 0 and got_f[b] != 1]
    assert not unflagged, "poisoned frames not flagged: %s (kinds %s), flags %s" % (unflagged, [b % 6 for b in unflagged],
                                                                                 got_f.tolist())
    for b in range(B):
        if b % 6 == 0:
            np.testing.assert_array_equal(got[b], clean[b], err_msg="control frame %d changed" % b)
            assert got_f[b] == clean_f[b], (b, got_f.tolist(), clean_f.tolist())
        if got_f[b] == 0:
            np.testing.assert_array_equal(got[b], ref[b], err_msg="unflagged frame %d" % b)
    full, _ = _run(ops, img, mk, mask, 0 | stage)
    for b in range(B):
        np.testing.assert_array_equal(full[b], ref[b], err_msg="mode 0, frame %d" % b)


@pytest.mark.parametrize("shape", SHAPES)
def test_poisoned_roots_before_border_pass_raise_the_flag(ops, shape):
    """Roots named from a union-find tile seam, poisoned before ws_uf_border_kernel: the fences of unite_glb over virtual nodes."""
    _first_level(ops, ops.WS_POISON_BORDER, shape, 1)


@pytest.mark.parametrize("shape", SHAPES)
def test_poisoned_roots_before_label_pass_raise_the_flag(ops, shape):
    """Roots poisoned before the first level's label pass: label4_chains and the third-entry walk of ws_uf_label4_kernel
    (W % 4 == 0), walk_root over virtual nodes in ws_uf_label_kernel<UF_OPTIMISTIC> (otherwise); flagged frames also go through UF_REPAIR."""
    _first_level(ops, ops.WS_POISON_LABEL, shape, 2)


def test_poisoned_roots_at_the_second_level_raise_the_flag(ops):
    """Frames with many ties that go on to the second level, poisoned there (listed frames, active tiles) before UF_DETECT /
    UF_ASSIGN.  A poisoned frame that never reaches the second level is untouched: it equals its unpoisoned run."""
    newly_flagged = 0
    for i, p in enumerate(SHAPES):
        shape = p.values[0]
        img, mk, mask = _frames(shape, 30 + i, ties=True)
        ref = _refs(img, mk, mask)
        clean, clean_f = _run(ops, img, mk, mask, 2)
        got, got_f = _run(ops, img, mk, mask, 2 | ops.WS_POISON_LEVEL2)
        for b in range(B):
            if got_f[b] == 0:
                np.testing.assert_array_equal(got[b], ref[b], err_msg="%s: unflagged frame %d" % (p.id, b))
            if b % 6 == 0 or got_f[b] == 0:
                np.testing.assert_array_equal(got[b], clean[b], err_msg="%s: frame %d changed" % (p.id, b))
                assert got_f[b] == clean_f[b], (p.id, b, got_f.tolist(), clean_f.tolist())
            elif clean_f[b] == 0:
                newly_flagged += 1
        full, _ = _run(ops, img, mk, mask, 0 | ops.WS_POISON_LEVEL2)
        for b in range(B):
            np.testing.assert_array_equal(full[b], ref[b], err_msg="%s: mode 0, frame %d" % (p.id, b))
    # the second level really was poisoned: frames it resolves without the poison come back flagged with it
    assert newly_flagged >= 4, newly_flagged


def test_poison_bits_are_validated(ops):
    """At most one poison bit, never with mode 1 (the exact flood alone runs no union-find)."""
    img, mk, mask = (np.zeros((1, 8, 8), np.float32), np.ones((1, 8, 8), np.int32), np.ones((1, 8, 8), bool))
    for mode in (1 | ops.WS_POISON_LABEL, 2 | ops.WS_POISON_BORDER | ops.WS_POISON_LABEL, 64, 3):
        with pytest.raises(Exception):
            _run(ops, img, mk, mask, mode)
    out, flags = _run(ops, img, mk, mask, 6 | ops.WS_POISON_LEVEL2)
    np.testing.assert_array_equal(out[0], orc.watershed(img[0], mk[0], mask[0]))
