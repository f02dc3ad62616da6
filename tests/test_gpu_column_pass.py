"""The column pass that csrc/edt.hip and csrc/voronoi.hip share (csrc/column_pass.h) on the device: both transforms on the
frames of tests/test_column_pass_cpu.py, every result compared with ``==`` to the CPU expectation, and the two workspace
queries against the closed form of their layout."""
import numpy as np
import pytest

from test_column_pass_cpu import CAP, EDT_CAP, RADII, SHAPES, capped, reference

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")


def _host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES)
def test_both_transforms_on_the_shared_pass(shape):
    """one batch of eight frames through the nearest-label transform, the distance transform (exact, capped, fused with its
    threshold) and the disk dilation on the bit words (radius 31) and on staged row blocks (radius 32)"""
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    ref = reference(shape)
    names = ref["names"]
    labels = torch.from_numpy(ref["labels"].copy()).cuda()  # (the shared reference is read-only)
    mask = torch.from_numpy(ref["mask"].copy()).cuda()

    def same(got, want, what):
        got = _host(got)
        for b, name in enumerate(names):
            np.testing.assert_array_equal(got[b], want[b], err_msg="%s %s: %s" % (shape, name, what))

    d2, near, site = ops.nearest_label(labels, want_site=True)  # cap = the largest label = CAP
    same(d2, ref["d2"], "nearest_label d2")
    same(near, ref["near"], "nearest_label near")
    same(site, ref["site"], "nearest_label site")
    edt = ops.edt_sq(mask)
    same(edt, ref["edt"], "edt_sq")
    same(ops.edt_sq(mask, cap=EDT_CAP), capped(ref["edt"], EDT_CAP), "edt_sq cap=%d" % EDT_CAP)
    img = torch.where(mask != 0, 0.25, 0.75).to(torch.float32).contiguous()  # its < 0.5 set is the mask
    d2_lt, mask_lt = ops.edt_sq_lt(img, 0.5)
    same(d2_lt, ref["edt"], "edt_sq_lt")
    same(mask_lt, ref["mask"], "edt_sq_lt mask")
    x = (labels > 0).to(torch.uint8)
    for r in RADII:
        same(ops.dilate_disk(x, 1 << 1, r), ref["dilate"][r].astype(np.uint8), "dilate_disk r=%d" % r)
    # the two transforms against each other on the device (every frame with a site)
    assert torch.equal(d2[:7], edt[:7])
    assert names[7] == "empty" and int(labels.max().item()) == CAP


def _align256(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (3, 257, 5), (2, 33, 1030)])
def test_workspace_queries(B, H, W):
    """bits (4 bytes), up and dn (2 bytes each) per column and 32-row word, the per-frame flag; the distance transform adds
    a 64-bit count per frame and block of eight rows -- each region rounded up to 256 bytes"""
    _need_gpu()
    from particle_col_image_segmentation_amd import _lib
    lib = _lib.load()
    words = B * ((H + 31) // 32) * W
    column = _align256(4 * words) + 2 * _align256(2 * words) + _align256(4 * B)
    assert lib.pcseg_nearest_label_workspace_bytes(B, H, W) == column
    assert lib.pcseg_edt_workspace_bytes(B, H, W) == column + _align256(8 * B * ((H + 7) // 8))
