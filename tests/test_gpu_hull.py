"""The per-ROI convexity table on the device (csrc/hull.hip) against scikit-image's values (tests/golden/hull.npz) and the
pure-integer restatement of tests/test_hull_cpu.py -- every comparison is equality, floats bit for bit --, the ``convexity`` /
``refined_convexity`` tables of the pipeline, the sharded route and the drop-in helper ``get_cell_convexity``."""
import ctypes

import numpy as np
import pytest

from test_hull_cpu import HULL_ROW, areas, hull_properties, hull_table, load_fixture

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SCALE_TABLE = 512.0 / 19.0
NEW = ("convexity", "refined_convexity")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _device_tables(t, counts, cap=None):
    """(B, H, W) int32 CUDA tensor or numpy -> (stats, hull, overflow, props, counts) on the device"""
    from particle_col_image_segmentation_amd import ops
    if not isinstance(t, torch.Tensor):
        t = torch.from_numpy(np.ascontiguousarray(t, np.int32)).cuda()
    n = torch.tensor(list(counts), dtype=torch.int32).cuda()
    cap = max(1, int(n.max().item())) if cap is None else cap
    stats, _, _, _ = ops.region_reduce(t, n, cap=cap)
    hull, overflow = ops.region_hull(t, n, stats, cap=cap)
    return stats, hull, overflow, ops.hull_properties(stats, hull, n), n


def _assert_frames_equal(hull, props, labs, counts, cap, what):
    got, gp = hull.cpu().numpy(), props.cpu().numpy()
    for b, lab in enumerate(labs):
        n = min(int(counts[b]), cap)
        want = hull_table(lab, n)
        np.testing.assert_array_equal(got[b, :n], want, err_msg="%s frame %d" % (what, b))
        np.testing.assert_array_equal(_bits(gp[b, :n]), _bits(hull_properties(areas(lab, n), want)), err_msg="%s frame %d" % (what, b))


# ------------------------------------------------------------------ 1. the fixture: scikit-image's own values
def test_fixture_images_equal_skimage_bit_for_bit():
    _need_gpu()
    total = 0
    for name, lab, lbl, val in load_fixture():
        n = int(lab.max())
        stats, hull, overflow, props, _ = _device_tables(lab[None], [n])
        assert int(overflow[0]) == 0
        h, p, st = hull[0, :n].cpu().numpy(), props[0, :n].cpu().numpy(), stats[0, :n].cpu().numpy()
        np.testing.assert_array_equal(_bits(p[lbl - 1]), _bits(val), err_msg=name)
        # the integer table: convex_area and the Euler number as stored, feret_sq4 = 4 feret^2 (an integer below 2^36)
        want = np.stack([val[:, 0], np.rint(4.0 * val[:, 2] ** 2), val[:, 3], np.zeros(len(val))], axis=1).astype(np.int64)
        np.testing.assert_array_equal(h[lbl - 1], want, err_msg=name)
        dead = st[:, 0] == 0
        assert (h[dead] == 0).all() and np.isnan(p[dead]).all(), name
        total += len(lbl)
    assert total > 2300


# ------------------------------------------------------------------ 2. ragged shapes, cap, empty frames, tall ROIs
@pytest.mark.parametrize("shape", [(1, 67), (67, 1), (33, 70), (37, 83), (64, 64), (5, 1030), (300, 5), (2, 2), (67, 130)])
def test_ragged_shapes_and_unaligned_base(shape):
    _need_gpu()
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    B = 3
    # blocky labels: random seeds grown by repetition, plus scattered pixels -- labels are NOT connected here (several
    # blobs and specks per label, boxes that overlap, rows of a box without a pixel of the label)
    small = rng.integers(0, 6, (B, (H + 2) // 3, (W + 2) // 3))
    labs = np.repeat(np.repeat(small, 3, axis=1), 3, axis=2)[:, :H, :W].astype(np.int32)
    labs = np.where(rng.random(labs.shape) < 0.1, rng.integers(0, 9, labs.shape), labs).astype(np.int32)
    if H >= 300:
        labs[1, :, 1] = 7  # a ROI over every row: the tall path
    counts = [int(l.max()) for l in labs]
    _, hull, overflow, props, n = _device_tables(labs, counts)
    cap = hull.shape[1]
    _assert_frames_equal(hull, props, labs, counts, cap, "aligned")
    assert int(overflow.sum()) == 0
    # the same images at a base address that is 4 bytes off a 16-byte boundary
    flat = torch.empty((B * H * W + 1,), dtype=torch.int32, device="cuda")
    view = flat[1:].view(B, H, W)
    view.copy_(torch.from_numpy(labs))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    _, hull_u, _, props_u, _ = _device_tables(view, counts)
    _assert_frames_equal(hull_u, props_u, labs, counts, cap, "unaligned")


def test_cap_below_the_label_count():
    _need_gpu()
    from particle_col_image_segmentation_amd import _lib, ops
    cases = {c[0]: c[1] for c in load_fixture()}
    lab = cases["func_128_s7_ct3/class_map"]
    n = int(lab.max())
    cap = 40
    assert n > cap
    labs = np.stack([lab, np.where(lab <= cap, lab, 0)])
    t = torch.from_numpy(labs).cuda()
    want = [hull_table(l, cap) for l in labs]
    stats, _, _, _ = ops.region_reduce(t, torch.tensor([n, n], dtype=torch.int32).cuda(), cap=cap)
    for counts, flags in (([n, cap], [1, 0]), ([n, 10], [1, 0]), ([cap + 1, 0], [1, 0])):
        c = torch.tensor(counts, dtype=torch.int32).cuda()
        hull, overflow = ops.region_hull(t, c, stats, cap=cap)
        assert overflow.cpu().tolist() == flags
        for b in range(2):
            k = min(counts[b], cap)
            np.testing.assert_array_equal(hull[b, :k].cpu().numpy(), want[b][:k])
    # the same call on a table with guard words on both sides: nothing outside the rows below min(counts, cap) is touched
    lib = _lib.load()
    c = torch.tensor([n, 10], dtype=torch.int32).cuda()
    guarded = torch.full((64 + 2 * cap * 4 + 64,), -7, dtype=torch.int64, device="cuda")
    flag = torch.full((2 + 2,), -7, dtype=torch.int32, device="cuda")
    nbytes = lib.pcseg_region_hull_workspace_bytes(2, lab.shape[0], lab.shape[1], cap)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    ptr = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)
    _lib.check(lib.pcseg_region_hull(ptr(t), ptr(c), ptr(stats), ptr(guarded, 64 * 8), ptr(flag, 4), 2, lab.shape[0], lab.shape[1], cap,
                                     ptr(ws), nbytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "region_hull")
    torch.cuda.synchronize()
    assert (guarded[:64] == -7).all() and (guarded[-64:] == -7).all() and flag.cpu().tolist() == [-7, 1, 0, -7]
    body = guarded[64:-64].view(2, cap, 4).cpu().numpy()
    np.testing.assert_array_equal(body[0], want[0])
    np.testing.assert_array_equal(body[1, :10], want[1][:10])
    assert (body[1, 10:] == -7).all()


def test_batch_with_an_empty_frame():
    _need_gpu()
    cases = {c[0]: c[1] for c in load_fixture()}
    a = cases["func_64_s1/class_map"]
    b = cases["func_64_s1/watershed"]
    assert a.shape == b.shape
    labs = np.stack([a, b, np.zeros_like(a), a[::-1].copy()])
    counts = [int(l.max()) for l in labs]
    assert counts[2] == 0
    _, hull, overflow, props, _ = _device_tables(labs, counts)
    _assert_frames_equal(hull, props, labs, counts, hull.shape[1], "batch")
    assert overflow.cpu().tolist() == [0, 0, 0, 0]


def test_synthetic_frames_both_label_images():
    """two 512^2 frames: ~0.6 H rows of particle ROI (the tall path) among hundreds of small ROIs"""
    _need_gpu()
    from particle_col_image_segmentation_amd import ops, synth
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    pipe = FramePipeline(dict(synth.CELL_TYPES_5))
    res = pipe.run(torch.from_numpy(synth.gen_batch(41, 2, 512, 512)).cuda())
    res.synchronize()
    cap = res["stats"].shape[1]
    for key, cnt, st in (("labels", "counts", "stats"), ("ws_labels", "n_markers", "ws_stats")):
        hull, overflow = ops.region_hull(res[key], res[cnt], res[st], cap=cap)
        props = ops.hull_properties(res[st], hull, res[cnt])
        assert int(overflow.sum()) == 0
        labs, counts, stats = res[key].cpu().numpy(), res[cnt].cpu().numpy(), res[st].cpu().numpy()
        for b in range(2):
            n = int(counts[b])
            assert n > 50 and (key != "labels" or (stats[b, :min(n, cap), 5] - stats[b, :min(n, cap), 3]).max() > 200)
        _assert_frames_equal(hull, props, labs, counts, cap, key)
    pipe.synchronize()


# ------------------------------------------------------------------ 3. tables
def _expected_rows(t, lab_images):
    """the convexity rows the restatement gives for the (frame position, label) keys of a table"""
    per_frame, rows = {}, []
    for f, l in t[:, :2]:
        f, l = int(f), int(l)
        if f not in per_frame:
            tab = hull_table(lab_images[f])
            per_frame[f] = hull_properties(areas(lab_images[f]), tab)
        p = per_frame[f][l - 1]
        rows.append([p[0], p[1], p[2] / SCALE_TABLE, p[3], p[0] / (SCALE_TABLE * SCALE_TABLE)])
    return np.array(rows, np.float64).reshape(-1, 5)


@pytest.mark.parametrize("graph", [False, True])
def test_pipeline_convexity_tables(graph):
    _need_gpu()
    from particle_col_image_segmentation_amd import synth
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    pipe = FramePipeline(dict(synth.CELL_TYPES_5), graph=graph)
    stacks = torch.from_numpy(synth.gen_batch(9, 2, 256, 256)).cuda()
    res = pipe.run(stacks)
    every = dict(neighbours=True, pair_edges=np.linspace(0.0, 5.0, 6), refined=True, surface=True, surface_edges=np.linspace(0.0, 4.0, 9),
                 distances=True, shape=True, check=False)
    tabs = pipe.tables(res, convex=True, **every)
    plain = pipe.tables(res, **every)
    assert set(tabs) == set(plain) | set(NEW) | {k + "_columns" for k in NEW}
    for k in plain:  # every other table: bit for bit
        np.testing.assert_array_equal(tabs[k], plain[k], err_msg=k)
    assert tabs["convexity_columns"] == HULL_ROW and tabs["refined_convexity_columns"] == HULL_ROW
    cells, refined = tabs["cells"], tabs["refined"]
    assert cells.shape[0] > 10
    np.testing.assert_array_equal(tabs["convexity"][:, :3], tabs["shapes"][:, :3])
    np.testing.assert_array_equal(tabs["convexity"][:, :2], cells[:, :2])
    rk = refined[refined[:, 6] >= 1]
    assert rk.shape[0] > 10
    np.testing.assert_array_equal(tabs["refined_convexity"][:, :3], tabs["refined_shapes"][:, :3])
    np.testing.assert_array_equal(tabs["refined_convexity"][:, :2], rk[:, :2])
    for name, key in (("convexity", "labels"), ("refined_convexity", "ws_labels")):
        t = tabs[name]
        np.testing.assert_array_equal(_bits(t[:, 3:]), _bits(_expected_rows(t, res[key].cpu().numpy())), err_msg=name)
    only = pipe.tables(res, convex=True, check=False)
    assert set(only) - set(pipe.tables(res, check=False)) == {"convexity", "convexity_columns"}
    np.testing.assert_array_equal(only["convexity"], tabs["convexity"])
    both = pipe.tables(res, convex=True, refined=True, check=False)
    np.testing.assert_array_equal(both["refined_convexity"], tabs["refined_convexity"])
    pipe.synchronize()


def test_run_sharded_forwards_convexity_tables():
    _need_gpu()
    from particle_col_image_segmentation_amd import synth
    from particle_col_image_segmentation_amd.distributed import run_sharded
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    dev = torch.device("cuda")
    pipe = FramePipeline(dict(synth.CELL_TYPES_5))
    stacks = synth.gen_batch(8300, 3, 256, 256)
    make_batch = lambda ids: torch.from_numpy(stacks[list(ids)]).to(dev)
    kw = dict(batch=2, check=False, convex=True, refined=True)
    host = run_sharded(3, make_batch, pipe, **kw)
    forced = run_sharded(3, make_batch, pipe, force_gather=True, device=dev, **kw)
    pipe.synchronize()
    per = [pipe.tables(pipe.run(make_batch(ids)), frame_ids=ids, check=False, convex=True, refined=True) for ids in ([0, 1], [2])]
    for k in NEW:
        np.testing.assert_array_equal(host[k], forced[k], err_msg=k)
        np.testing.assert_array_equal(host[k], np.concatenate([p[k] for p in per]), err_msg=k)
    np.testing.assert_array_equal(host["convexity"][:, :2], host["cells"][:, :2])
    assert host["convexity"].shape[0] > 10 and host["refined_convexity"].shape[0] > 10
    assert not set(run_sharded(3, make_batch, pipe, batch=2, check=False)) & set(NEW)


# ------------------------------------------------------------------ 4. drop-in
@pytest.fixture
def hull_calls(monkeypatch):
    from particle_col_image_segmentation_amd import ops
    calls = []
    real = ops.region_hull

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ops, "region_hull", counted)
    return calls


def test_get_cell_convexity_equals_the_fixture(hull_calls):
    _need_gpu()
    from conftest import FUNC_CASES, load_golden
    from particle_col_image_segmentation_amd import tiff_analysis as ta
    fixture = {c[0]: c for c in load_fixture()}
    for case in FUNC_CASES:
        g = load_golden(case)
        ct = {int(k): str(v) for k, v in zip(g["ct_keys"], g["ct_vals"])}
        _, lab, lbl, val = fixture[case + "/denoised"]
        np.testing.assert_array_equal(lab, g["label_im"])
        row_of = {int(l): i for i, l in enumerate(lbl)}

        def check(got, what):
            for name, d in got.items():
                idx = [row_of[int(l)] for l in d["labels"]]
                want = val[idx].reshape(-1, 4)
                for k, col in ((0, "convex_area"), (1, "solidity"), (3, "euler_number")):
                    np.testing.assert_array_equal(_bits(d[col]), _bits(want[:, k]), err_msg="%s %s %s" % (case, what, col))
                np.testing.assert_array_equal(_bits(d["feret_um"]), _bits(want[:, 2] / ta.PX_TO_UM_CONV), err_msg="%s %s" % (case, what))

        # ---- regionprops: every region of the frame, one device call however often the helper is asked
        del hull_calls[:]
        regs = ta.regionprops(g["label_im"])
        assert len(hull_calls) == 0 and len(regs) == len(lbl)
        got = ta.get_cell_convexity({"all": regs})
        assert got["all"]["labels"].tolist() == lbl.tolist()
        check(got, "regionprops")
        check(ta.get_cell_convexity({"some": regs[::2], "rest": regs[1::2]}), "regionprops again")
        assert len(hull_calls) == 1
        with pytest.raises(AttributeError):
            regs[0].solidity
        # ---- get_cell_positions_and_areas: nothing until asked, then one call for the frame (cells and clusters share it)
        if "crash" in g.files:
            continue
        del hull_calls[:]
        cell_pos, cell_clusters, _, _ = ta.get_cell_positions_and_areas(g["denoised"], dict(ct), merged=True)
        assert len(hull_calls) == 0
        assert sum(len(v) for v in cell_pos.values()) + sum(len(v) for v in cell_clusters.values()) > 0
        check(ta.get_cell_convexity(cell_pos), "cell_pos")
        check(ta.get_cell_convexity(cell_clusters), "cell_clusters")
        assert len(hull_calls) == 1
