"""The per-label reductions that share csrc/label_reduce.h -- ops.region_reduce (plane-free: both VEC instantiations of
the column-run walk; with planes: the fused column kernel, or the integer columns from that walk and the sums from the row
sums kernel), ops.region_sums2 (the two-image sums kernel, image B's integer columns from the plane-free pass),
ops.region_shape and ops.label_parent -- on the banded images of tests/test_label_reduce_cpu.py: labels that collide in a
block's slot table, columns that end sixteen runs per block, a wave that is one segment.  Every row is compared exactly (the float64 plane sums at the rtol of test_gpu_primitives.test_region_reduce: only the order of the
float64 additions differs between the routes), from an aligned base and from one 4 bytes off a 16-byte boundary."""
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
    """the int32 or float32 array on the device, its base `off` words past a 16-byte boundary"""
    src = torch.from_numpy(np.array(a))  # (a copy: the images are read-only)
    assert src.element_size() == 4
    flat = torch.empty((a.size + 4,), dtype=src.dtype, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[off:off + a.size].view(a.shape)
    view.copy_(src)
    assert view.data_ptr() % 16 == 4 * off and view.is_contiguous()
    return view


@functools.lru_cache(maxsize=None)
def _expected_stats(shape):
    lab = banded(*shape)
    return np.stack([np_region_rows(l, 517) for l in lab])


@functools.lru_cache(maxsize=None)
def _planes(shape, C=5):
    B, H, W = shape
    rng = np.random.default_rng(7 * H + W)
    cls = rng.integers(0, 6, (B, H, W)).astype(np.uint8)
    planes = (rng.random((B, C, H, W)) * 100).astype(np.float32)
    lab = banded(*shape)
    sums = np.stack([np_plane_sums(lab[b], planes[b], 517) for b in range(B)])
    return cls, planes, sums


# the class selection of the plane sums: classes 1 and 4 of the 0 .. 5 of _planes
BITS = (1 << 1) | (1 << 4)


@functools.lru_cache(maxsize=None)
def _selected(shape, C, image="banded"):
    """(class map, expected sums) of the banded image, or of the shifted one, under BITS.  The class map is _planes' with
    class 3 (not selected) on every pixel whose banded label is 2 mod 5: those labels have no selected pixel in the banded
    image"""
    cls, planes, _ = _planes(shape, C)
    lab = banded(*shape)
    cm = np.where(lab % 5 == 2, 3, cls).astype(np.uint8)
    of = lab if image == "banded" else shifted(lab)
    return cm, np.stack([np_plane_sums(of[b], planes[b], 517, cm[b], BITS) for b in range(shape[0])])


# the routes of region_reduce with planes: (shape, labels' offset, planes' offset) in 4-byte words past a 16-byte boundary.
# W % 4 == 0 and both aligned: the fused column kernel; labels off: guarded labels, the row sums kernel; planes off: VECTOR
# labels, the row sums kernel; a ragged width: guarded labels, the row sums kernel.  1032 columns cross the second
# 1024-column block, 34 rows the second 32-row block
VECTOR_SHAPES = [(2, 64, 64), (1, 34, 1032)]
SUM_CASES = [(s, off, 0) for s in SHAPES + VECTOR_SHAPES[1:] for off in (0, 1)] + [(s, 0, 1) for s in VECTOR_SHAPES]
SUM_IDS = ["%dx%dx%d%s%s" % (s + ("" if off == 0 else "-unaligned", "" if poff == 0 else "-planes_unaligned")) for s, off, poff in SUM_CASES]
PLANE_COUNTS = [3, 5, 7, 8]  # NC = 5 not exact / exact, NC = 8 not exact / exact


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


@pytest.mark.parametrize("C", PLANE_COUNTS)
@pytest.mark.parametrize("shape,off,poff", SUM_CASES, ids=SUM_IDS)
def test_region_reduce_plane_sums_on_every_route(shape, off, poff, C):
    """every pixel, then the pixels of the classes in BITS: the integer rows do not depend on the selection, a label
    without a selected pixel sums to exactly 0"""
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    lab, want = banded(*shape), _expected_stats(shape)
    _, planes, sums = _planes(shape, C)
    cm, sel_sums = _selected(shape, C)
    t, tp, tc = _at(lab, off), _at(planes, poff), torch.from_numpy(cm).cuda()
    counts = torch.full((shape[0],), 517, dtype=torch.int32, device="cuda")
    for bits, expected in ((0, sums), (BITS, sel_sums)):
        stats, cls_out, got, overflow = ops.region_reduce(t, counts, tc, tp, sum_classes=bits)
        assert overflow.cpu().tolist() == [0] * shape[0]
        np.testing.assert_array_equal(stats.cpu().numpy(), want)
        got = got.cpu().numpy()
        np.testing.assert_allclose(got, expected, rtol=1e-12, atol=0)
        for b in range(shape[0]):
            live = want[b, :, 0] > 0
            np.testing.assert_array_equal(cls_out[b].cpu().numpy()[live], cm[b].ravel()[want[b, live, 7]])
    unselected = (want[:, :, 0] > 0) & (sel_sums == 0).all(axis=2)
    assert unselected[:, [1, 256, 516]].all() and (got[unselected] == 0).all() and (got[want[:, :, 0] == 0] == 0).all()


@pytest.mark.parametrize("C", PLANE_COUNTS)
@pytest.mark.parametrize("shape", VECTOR_SHAPES, ids=["%dx%dx%d" % s for s in VECTOR_SHAPES])
def test_region_sums2_plane_counts(shape, C):
    """image A = the shifted bands under BITS, image B = the bands, every NC / EXACT form of the sums kernel"""
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    R = banded(*shape)
    _, planes, sums_b = _planes(shape, C)
    cm, sums_a = _selected(shape, C, "shifted")
    counts = torch.full((shape[0],), 517, dtype=torch.int32, device="cuda")
    _, got_a, _ = ops.region_init(counts, 517, C, shape, "cuda")
    _, got_b, _ = ops.region_init(counts, 517, C, shape, "cuda")
    ops.region_sums2(_at(shifted(R), 0), torch.from_numpy(cm).cuda(), BITS, got_a, _at(R, 0), got_b, _at(planes, 0))
    np.testing.assert_allclose(got_a.cpu().numpy(), sums_a, rtol=1e-12, atol=0)
    np.testing.assert_allclose(got_b.cpu().numpy(), sums_b, rtol=1e-12, atol=0)


@pytest.mark.parametrize("with_stats", [True, False], ids=["stats_b", "sums_only"])
@pytest.mark.parametrize("shape", VECTOR_SHAPES, ids=["%dx%dx%d" % s for s in VECTOR_SHAPES])
def test_region_sums2_capacity_below_the_labels(shape, with_stats):
    """cap_b = 300 below the largest label present (517): with stats_b the integer rows below the cap are the reference's
    and every frame is flagged; without, the labels above the cap are skipped and nothing is flagged"""
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    R, want = banded(*shape), _expected_stats(shape)
    _, planes, sums_b = _planes(shape)
    cm, sums_a = _selected(shape, 5, "shifted")
    counts = torch.full((shape[0],), 517, dtype=torch.int32, device="cuda")
    _, got_a, _ = ops.region_init(counts, 517, 5, shape, "cuda")
    stats_b, got_b, overflow_b = ops.region_init(counts, 300, 5, shape, "cuda")
    neutral = stats_b.cpu().numpy()
    ops.region_sums2(_at(shifted(R), 0), torch.from_numpy(cm).cuda(), BITS, got_a, _at(R, 0), got_b, _at(planes, 0),
                     stats_b=stats_b if with_stats else None, overflow_b=overflow_b)
    assert got_b.shape[1] == 300 and overflow_b.cpu().tolist() == [1 if with_stats else 0] * shape[0]
    np.testing.assert_array_equal(stats_b.cpu().numpy(), want[:, :300] if with_stats else neutral)
    np.testing.assert_allclose(got_b.cpu().numpy(), sums_b[:, :300], rtol=1e-12, atol=0)
    np.testing.assert_allclose(got_a.cpu().numpy(), sums_a, rtol=1e-12, atol=0)


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
