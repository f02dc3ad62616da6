"""The per-label reductions that share csrc/label_reduce.h -- ops.region_reduce (plane-free: both VEC instantiations of
the column-run walk; with planes: the fused column kernel and the row fallback), ops.region_shape and ops.label_parent --
on the banded images of tests/test_label_reduce_cpu.py: labels that collide in a block's slot table, columns that end
sixteen runs per block, a wave that is one segment.  Every row is compared exactly (the float64 plane sums at the rtol of
test_gpu_primitives.test_region_reduce), from an aligned base and from one 4 bytes off a 16-byte boundary."""
import functools

import numpy as np
import pytest

from test_gpu_refined_cells import _check_lp
from test_label_reduce_cpu import SHAPES, banded, np_plane_sums, np_region_rows, shifted
from test_shape_cpu import shape_table

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CASES = [(s, off) for s in SHAPES for off in (0, 1)]
IDS = ["%dx%dx%d%s" % (s + ("" if off == 0 else "-unaligned",)) for s, off in CASES]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")


def _at(a, off):
    """the int32 array on the device, its base `off` words past a 16-byte boundary"""
    flat = torch.empty((a.size + 4,), dtype=torch.int32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[off:off + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.array(a)))  # (a copy: the images are read-only)
    assert view.data_ptr() % 16 == 4 * off and view.is_contiguous()
    return view


@functools.lru_cache(maxsize=None)
def _expected_stats(shape):
    lab = banded(*shape)
    return np.stack([np_region_rows(l, 517) for l in lab])


@functools.lru_cache(maxsize=None)
def _planes(shape):
    B, H, W = shape
    rng = np.random.default_rng(7 * H + W)
    cls = rng.integers(0, 6, (B, H, W)).astype(np.uint8)
    planes = (rng.random((B, 5, H, W)) * 100).astype(np.float32)
    lab = banded(*shape)
    sums = np.stack([np_plane_sums(lab[b], planes[b], 517) for b in range(B)])
    return cls, planes, sums


@pytest.mark.parametrize("shape,off", CASES, ids=IDS)
def test_region_reduce_plane_free(shape, off):
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    lab, want = banded(*shape), _expected_stats(shape)
    t = _at(lab, off)
    counts = torch.full((shape[0],), 517, dtype=torch.int32, device="cuda")
    stats, _, _, overflow = ops.region_reduce(t, counts)
    assert stats.shape[1] == 517 and overflow.cpu().tolist() == [0] * shape[0]
    np.testing.assert_array_equal(stats.cpu().numpy(), want)  # (absent labels: the neutral row of region_init_kernel)
    stats, _, _, overflow = ops.region_reduce(t, counts, cap=300)
    assert overflow.cpu().tolist() == [1] * shape[0]
    np.testing.assert_array_equal(stats.cpu().numpy(), want[:, :300])


@pytest.mark.parametrize("shape,off", CASES, ids=IDS)
def test_region_reduce_with_class_map_and_five_planes(shape, off):
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    lab, want = banded(*shape), _expected_stats(shape)
    cls, planes, sums = _planes(shape)
    counts = torch.full((shape[0],), 517, dtype=torch.int32, device="cuda")
    stats, cls_out, got, overflow = ops.region_reduce(_at(lab, off), counts, torch.from_numpy(cls).cuda(), torch.from_numpy(planes).cuda())
    assert overflow.cpu().tolist() == [0] * shape[0]
    np.testing.assert_array_equal(stats.cpu().numpy(), want)
    np.testing.assert_allclose(got.cpu().numpy(), sums, rtol=1e-12, atol=0)
    for b in range(shape[0]):
        live = want[b, :, 0] > 0
        np.testing.assert_array_equal(cls_out[b].cpu().numpy()[live], cls[b].ravel()[want[b, live, 7]])


@pytest.mark.parametrize("shape,off", CASES, ids=IDS)
def test_region_shape(shape, off):
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    lab = banded(*shape)
    t = _at(lab, off)
    counts = torch.full((shape[0],), 517, dtype=torch.int32, device="cuda")
    got, overflow = ops.region_shape(t, counts)
    assert overflow.cpu().tolist() == [0] * shape[0]
    for b in range(shape[0]):
        np.testing.assert_array_equal(got[b].cpu().numpy(), shape_table(lab[b], 517))
    # counts below the labels present, cap above: labels above the count are skipped without a flag
    low = torch.full((shape[0],), 260, dtype=torch.int32, device="cuda")
    got, overflow = ops.region_shape(t, low, cap=600)
    assert overflow.cpu().tolist() == [0] * shape[0]
    for b in range(shape[0]):
        np.testing.assert_array_equal(got[b, :260].cpu().numpy(), shape_table(lab[b], 260))


@pytest.mark.parametrize("shape,off", CASES, ids=IDS)
def test_label_parent(shape, off):
    _need_gpu()
    R = banded(*shape)
    A = shifted(R)
    _check_lp(_at(A, off), _at(R, off), [517] * shape[0], 517, None, True, A, R)
