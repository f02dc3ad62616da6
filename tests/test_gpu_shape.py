"""The per-ROI shape table on the device (csrc/shape.hip) against the numpy / exact-rational restatement of
tests/test_shape_cpu.py (integer table: bit for bit; derived columns: inside the bound derived there), the ``shapes`` /
``refined_shapes`` tables of the pipeline, the sharded route and the lazy drop-in attributes of ``Region``."""
import math

import numpy as np
import pytest

from test_shape_cpu import COLUMNS, SHAPE_ROW, deviation, exact_properties, load_fixture, region_table, shape_table

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SCALE_TABLE = 512.0 / 19.0
NEW = ("shapes", "refined_shapes")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")


def _device_tables(labs, cap=None, counts=None):
    """(B, H, W) int32 numpy -> (stats, shape, overflow, counts) numpy from the device"""
    from particle_col_image_segmentation_amd import ops
    t = torch.from_numpy(np.ascontiguousarray(labs, np.int32)).cuda()
    n = torch.tensor([int(l.max()) for l in labs] if counts is None else counts, dtype=torch.int32).cuda()
    cap = max(1, int(n.max().item())) if cap is None else cap
    stats, _, _, _ = ops.region_reduce(t, n, cap=cap)
    shape, overflow = ops.region_shape(t, n, cap=cap)
    return stats, shape, overflow, n


def _assert_rows_equal(shape, labs, counts, cap, what):
    got = shape.cpu().numpy()
    for b, lab in enumerate(labs):
        n = min(int(counts[b]), cap)
        want = shape_table(lab, n)
        np.testing.assert_array_equal(got[b, :n], want, err_msg="%s frame %d" % (what, b))


def _assert_inside_bound(got, ex, what):
    dev = deviation(got, ex)
    print("%-30s %5d rows, worst deviation / bound per column: %s" % (what, len(got), np.array2string(dev.max(axis=0, initial=0), precision=3)))
    bad = np.argwhere(~(dev <= 1.0))
    assert len(bad) == 0, (what, [(int(i) + 1, COLUMNS[k], got[i, k], ex[i, k]) for i, k in bad[:5]])


# ------------------------------------------------------------------ 1. integer table and derived columns on the fixture
def test_fixture_images_integer_table_bit_for_bit_and_derived_inside_bound():
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    for name, lab, val, _ in load_fixture():
        stats, shape, overflow, n = _device_tables(lab[None])
        k = int(n[0])
        np.testing.assert_array_equal(shape[0, :k].cpu().numpy(), shape_table(lab, k), err_msg=name)
        np.testing.assert_array_equal(stats[0, :k].cpu().numpy(), region_table(lab, k), err_msg=name)
        assert int(overflow[0]) == 0
        props = ops.shape_properties(stats, shape, n)[0, :k].cpu().numpy()
        st, sh = stats[0, :k].cpu().numpy(), shape[0, :k].cpu().numpy()
        live = st[:, 0] > 0
        assert np.isnan(props[~live]).all()
        ex = exact_properties(st[live], sh[live])
        _assert_inside_bound(props[live], ex, name)
        # where the integers say a == c the device takes the formula's own branch, exactly
        sym = ex[:, 0] == ex[:, 2]
        np.testing.assert_array_equal(props[live][sym, 8], ex[sym, 8], err_msg=name)


def test_integer_valued_shapes_are_exact():
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    cases = {c[0]: c[1] for c in load_fixture()}
    got = {}
    for name in ("single_pixel", "line_h", "line_v", "line_diag", "block_2x2", "full_frame"):
        stats, shape, _, n = _device_tables(cases[name][None])
        got[name] = ops.shape_properties(stats, shape, n)[0, 0].cpu().numpy()
    p = got["single_pixel"]
    assert p[:8].tolist() == [0.0] * 8 and p[8] == math.pi / 4 and p[9] == math.sqrt(4 / math.pi) and p[10] == 1.0 and p[11] == 0.0
    h = got["line_h"]  # 7 pixels in a row: column variance 4
    assert h[0] == 4.0 and h[1] == 0.0 and h[2] == 0.0 and h[3] == 4.0 and h[4] == 0.0 and h[5] == 8.0 and h[6] == 0.0 and h[7] == 1.0
    assert abs(h[8]) == math.pi / 2 and h[10] == 1.0 and h[11] == 5.0
    v = got["line_v"]
    assert v[0] == 0.0 and v[2] == 4.0 and v[3] == 4.0 and v[4] == 0.0 and v[7] == 1.0 and v[8] == 0.0 and v[11] == 5.0
    d = got["line_diag"]  # a == c == 4, b == -4: the a - c == 0 branch with b < 0
    assert d[0] == 4.0 and d[1] == -4.0 and d[2] == 4.0 and d[3] == 8.0 and d[4] == 0.0 and d[8] == -math.pi / 4
    assert d[11] == 5 * math.sqrt(2) and d[10] == 7 / 49
    q = got["block_2x2"]
    assert q[0] == 0.25 and q[1] == 0.0 and q[2] == 0.25 and q[3] == 0.25 and q[4] == 0.25 and q[7] == 0.0 and q[8] == math.pi / 4
    assert q[11] == 4.0 and q[10] == 1.0
    f = got["full_frame"]  # 7 x 10: variances (49 - 1) / 12 and (100 - 1) / 12
    assert f[0] == 99 / 12 and f[2] == 4.0 and f[1] == 0.0 and f[10] == 1.0


# ------------------------------------------------------------------ 2. the benchmark batch, a 2048^2 frame, ragged shapes
def test_benchmark_batch_both_label_images_and_a_2048_frame():
    _need_gpu()
    from particle_col_image_segmentation_amd import ops, synth
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    dev = torch.device("cuda")
    pipe = FramePipeline(dict(synth.CELL_TYPES_5))
    for size, B, frames in ((1024, 64, (0, 1, 7, 13, 31, 32, 50, 63)), (2048, 1, (0,))):
        stack = synth.gen_batch_torch(10000, B, size, size, dev)
        res = pipe.run(stack)
        res.synchronize()
        cap = res["stats"].shape[1]
        for key, cnt in (("labels", "counts"), ("ws_labels", "n_markers")):
            shape, overflow = ops.region_shape(res[key], res[cnt], cap=cap)
            assert int(overflow.sum()) == 0
            counts = res[cnt].cpu().numpy()
            got = shape.cpu().numpy()
            for b in frames:
                lab = res[key][b].cpu().numpy()
                n = min(int(counts[b]), cap)
                assert n > 100
                np.testing.assert_array_equal(got[b, :n], shape_table(lab, n), err_msg="%s %d frame %d" % (key, size, b))
            if size == 1024:  # the derived columns of one frame against the exact evaluation
                st = res["stats" if key == "labels" else "ws_stats"]
                props = ops.shape_properties(st, shape, res[cnt])[0].cpu().numpy()
                n = min(int(counts[0]), cap)
                s0 = st[0, :n].cpu().numpy()
                live = s0[:, 0] > 0
                _assert_inside_bound(props[:n][live], exact_properties(s0[live], got[0, :n][live]), "benchmark frame 0 " + key)
        del stack, res
    pipe.synchronize()


@pytest.mark.parametrize("shape", [(1, 67), (67, 1), (33, 70), (37, 83), (64, 64), (5, 1030), (100, 4), (31, 2), (2, 2)])
def test_ragged_shapes_and_unaligned_base(shape):
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    B = 3
    # blocky labels: random seeds grown by repetition, so that runs, borders and single pixels all occur
    small = rng.integers(0, 6, (B, (H + 2) // 3, (W + 2) // 3))
    labs = np.repeat(np.repeat(small, 3, axis=1), 3, axis=2)[:, :H, :W].astype(np.int32)
    labs = np.where(rng.random(labs.shape) < 0.1, rng.integers(0, 9, labs.shape), labs).astype(np.int32)
    counts = [int(l.max()) for l in labs]
    stats, shape_t, overflow, n = _device_tables(labs)
    _assert_rows_equal(shape_t, labs, counts, shape_t.shape[1], "aligned")
    assert int(overflow.sum()) == 0
    # the same images at a base address that is 4 bytes off a 16-byte boundary
    flat = torch.empty((B * H * W + 1,), dtype=torch.int32, device="cuda")
    view = flat[1:].view(B, H, W)
    view.copy_(torch.from_numpy(labs))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    shape_u, _ = ops.region_shape(view, n, cap=shape_t.shape[1])
    _assert_rows_equal(shape_u, labs, counts, shape_t.shape[1], "unaligned")


def test_cap_below_the_label_count():
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    cases = {c[0]: c[1] for c in load_fixture()}
    lab = cases["func_256_s9/class_map"]
    n = int(lab.max())
    cap = 40
    assert n > cap
    labs = np.stack([lab, np.where(lab <= cap, lab, 0)])  # frame 1 holds no label above cap
    t = torch.from_numpy(labs).cuda()
    counts = torch.tensor([n, n], dtype=torch.int32).cuda()
    lib_shape, overflow = ops.region_shape(t, counts, cap=cap)
    assert overflow.cpu().tolist() == [1, 0]
    for b in range(2):
        np.testing.assert_array_equal(lib_shape[b].cpu().numpy(), shape_table(labs[b], cap))
    # the same call on a table with guard words on both sides: nothing outside the (B, cap, 8) block is touched
    import ctypes
    from particle_col_image_segmentation_amd import _lib
    lib = _lib.load()
    guarded = torch.full((64 + 2 * cap * 8 + 64,), -7, dtype=torch.int64, device="cuda")
    flag = torch.full((2 + 2,), -7, dtype=torch.int32, device="cuda")
    nbytes = lib.pcseg_region_shape_workspace_bytes(2, *lab.shape)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    ptr = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)
    _lib.check(lib.pcseg_region_shape(ptr(t), ptr(counts), ptr(guarded, 64 * 8), ptr(flag, 4), 2, lab.shape[0], lab.shape[1], cap, ptr(ws),
                                      nbytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "region_shape")
    torch.cuda.synchronize()
    assert (guarded[:64] == -7).all() and (guarded[-64:] == -7).all() and flag.cpu().tolist() == [-7, 1, 0, -7]
    assert torch.equal(guarded[64:-64].view(2, cap, 8), lib_shape)
    # counts below the labels present: rows up to the count are exact, labels above it are skipped without a flag
    low = torch.tensor([10, 10], dtype=torch.int32).cuda()
    part, overflow = ops.region_shape(t, low, cap=cap)
    assert overflow.cpu().tolist() == [1, 0]
    for b in range(2):
        np.testing.assert_array_equal(part[b, :10].cpu().numpy(), shape_table(labs[b], 10))


# ------------------------------------------------------------------ 3. tables
def _expected_shape_rows(keys, lab_images, stats_tables):
    """rows (frame position, label) -> (integer shape rows (n, 8), exact derived columns (n, 12)) from the restatement"""
    per_frame = {}
    sh = np.zeros((len(keys), 8), np.int64)
    st = np.zeros((len(keys), 8), np.int64)
    for i, (b, l) in enumerate(keys):
        if b not in per_frame:
            per_frame[b] = shape_table(lab_images[b])
        sh[i], st[i] = per_frame[b][l - 1], stats_tables[b][l - 1]
    return sh, exact_properties(st, sh)


@pytest.mark.parametrize("graph", [False, True])
def test_pipeline_shape_tables(graph):
    _need_gpu()
    from particle_col_image_segmentation_amd import synth
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    ct = dict(synth.CELL_TYPES_5)
    pipe = FramePipeline(ct, graph=graph)
    stacks = torch.from_numpy(synth.gen_batch(9, 3, 256, 256)).cuda()
    res = pipe.run(stacks)
    every = dict(neighbours=True, pair_edges=np.linspace(0.0, 5.0, 6), refined=True, surface=True, surface_edges=np.linspace(0.0, 4.0, 9),
                 distances=True, check=False)
    tabs = pipe.tables(res, shape=True, **every)
    plain = pipe.tables(res, **every)
    assert set(tabs) == set(plain) | set(NEW) | {k + "_columns" for k in NEW}
    for k in plain:  # every other table: bit for bit
        np.testing.assert_array_equal(tabs[k], plain[k], err_msg=k)
    assert tabs["shapes_columns"] == SHAPE_ROW and tabs["refined_shapes_columns"] == SHAPE_ROW
    cells, refined = tabs["cells"], tabs["refined"]
    assert cells.shape[0] > 20
    np.testing.assert_array_equal(tabs["shapes"][:, :2], cells[:, :2])
    rk = refined[refined[:, 6] >= 1]
    assert rk.shape[0] > 20
    np.testing.assert_array_equal(tabs["refined_shapes"][:, :2], rk[:, :2])
    np.testing.assert_array_equal(tabs["refined_shapes"][:, 2], tabs["refined_neighbours"][:, 2])
    np.testing.assert_array_equal(tabs["shapes"][:, 2], tabs["neighbours"][:, 2])
    # values: the integer columns exact, the derived ones inside the bound (lengths at the scale of the other _um columns)
    for name, key, st_key in (("shapes", "labels", "stats"), ("refined_shapes", "ws_labels", "ws_stats")):
        t = tabs[name]
        labs = res[key].cpu().numpy()
        stats = res[st_key].cpu().numpy()
        keys = [(int(f), int(l)) for f, l in t[:, :2]]
        sh, exact = _expected_shape_rows(keys, labs, stats)
        np.testing.assert_array_equal(t[:, 3:7], sh[:, [6, 3, 4, 5]], err_msg=name)  # n_border, n_1, n_sqrt2, n_mid: exact
        # the table's columns in COLUMNS order, lengths back in pixels (one rounding each way through the scale); l1 and l2
        # are not in the table: minor and eccentricity are judged against the exact l1, l2
        got = np.stack([t[:, 9], -t[:, 8], t[:, 7], exact[:, 3], exact[:, 4], t[:, 10] * SCALE_TABLE, t[:, 11] * SCALE_TABLE, t[:, 12],
                        t[:, 13], t[:, 14] * SCALE_TABLE, t[:, 15], t[:, 16] * SCALE_TABLE], axis=1)
        _assert_inside_bound(got, exact, name + (" graph" if graph else ""))
    only = pipe.tables(res, shape=True, check=False)
    assert set(only) - set(pipe.tables(res, check=False)) == {"shapes", "shapes_columns"}
    np.testing.assert_array_equal(only["shapes"], tabs["shapes"])
    pipe.synchronize()


def test_run_sharded_forwards_shape_tables():
    _need_gpu()
    from particle_col_image_segmentation_amd import synth
    from particle_col_image_segmentation_amd.distributed import run_sharded
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    dev = torch.device("cuda")
    pipe = FramePipeline(dict(synth.CELL_TYPES_5))
    stacks = synth.gen_batch(8300, 6, 256, 256)
    make_batch = lambda ids: torch.from_numpy(stacks[list(ids)]).to(dev)
    kw = dict(batch=4, check=False, shape=True, refined=True)
    host = run_sharded(6, make_batch, pipe, **kw)
    forced = run_sharded(6, make_batch, pipe, force_gather=True, device=dev, **kw)
    pipe.synchronize()
    per = [pipe.tables(pipe.run(make_batch(ids)), frame_ids=ids, check=False, shape=True, refined=True) for ids in ([0, 1, 2, 3], [4, 5])]
    for k in NEW:
        np.testing.assert_array_equal(host[k], forced[k], err_msg=k)
        np.testing.assert_array_equal(host[k], np.concatenate([p[k] for p in per]), err_msg=k)
    np.testing.assert_array_equal(host["shapes"][:, :2], host["cells"][:, :2])
    assert host["shapes"].shape[0] > 20 and host["refined_shapes"].shape[0] > 20
    assert not set(run_sharded(6, make_batch, pipe, batch=4, check=False)) & set(NEW)


# ------------------------------------------------------------------ 4. drop-in
ATTRS = ("inertia_tensor", "inertia_tensor_eigvals", "major_axis_length", "minor_axis_length", "eccentricity", "orientation",
         "equivalent_diameter", "extent", "perimeter")


def _row_of(region):
    t = region.inertia_tensor
    assert t.shape == (2, 2) and t[0, 1] == t[1, 0]
    return [t[0, 0], t[0, 1], t[1, 1], *region["inertia_tensor_eigvals"], region.major_axis_length, region["minor_axis_length"],
            region.eccentricity, region.orientation, region["equivalent_diameter"], region.extent, region.perimeter]


@pytest.fixture
def shape_calls(monkeypatch):
    from particle_col_image_segmentation_amd import ops
    calls = []
    real = ops.region_shape

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ops, "region_shape", counted)
    return calls


def test_dropin_region_attributes(shape_calls):
    _need_gpu()
    from conftest import FUNC_CASES, load_golden
    from particle_col_image_segmentation_amd import tiff_analysis as ta
    fixture = {c[0]: c for c in load_fixture()}
    for case in FUNC_CASES:
        g = load_golden(case)
        ct = {int(k): str(v) for k, v in zip(g["ct_keys"], g["ct_vals"])}
        _, lab, val, _ = fixture[case + "/denoised"]
        np.testing.assert_array_equal(lab, g["label_im"])
        stats = region_table(lab)
        ex = exact_properties(stats, shape_table(lab))
        # ---- regionprops: every region, one launch however many attributes are read
        del shape_calls[:]
        regs = ta.regionprops(g["label_im"])
        assert len(shape_calls) == 0 and len(regs) == len(val)
        got = np.array([_row_of(r) for r in regs])
        assert len(shape_calls) == 1
        _assert_inside_bound(got, ex, case + " regionprops vs exact")
        _assert_inside_bound(val, ex, case + " skimage vs exact")
        dv = deviation(got, val)  # and within the bound of the stored scikit-image values themselves
        print("%-30s vs scikit-image, worst / bound per column: %s" % (case, np.array2string(dv.max(axis=0, initial=0), precision=3)))
        assert (dv <= 1.0).all(), case
        for other in ("solidity", "convex_area", "euler_number"):
            with pytest.raises(AttributeError):
                getattr(regs[0], other)
        # ---- get_cell_positions_and_areas: nothing until asked, then one launch for the frame
        if "crash" in g.files:
            continue
        del shape_calls[:]
        cell_pos, cell_clusters, _, merged = ta.get_cell_positions_and_areas(g["denoised"], dict(ct), merged=True)
        assert len(shape_calls) == 0
        members = [r for groups in merged.values() for grp in groups for r in grp["regions"]]
        everyone = [r for regs in list(cell_pos.values()) + list(cell_clusters.values()) for r in regs] + members
        assert everyone
        rows = np.array([_row_of(r) for r in everyone])
        assert len(shape_calls) == 1
        idx = np.array([r.label - 1 for r in everyone])
        _assert_inside_bound(rows, ex[idx], case + " get_cell_positions_and_areas")
        assert (deviation(rows, val[idx]) <= 1.0).all(), case


def test_dropin_refined_regions(shape_calls):
    _need_gpu()
    from conftest import load_golden
    from particle_col_image_segmentation_amd import tiff_analysis as ta
    g = load_golden("func_256_s9")
    ct = {int(k): str(v) for k, v in zip(g["ct_keys"], g["ct_vals"])}
    cell_pos, cell_clusters, _, _ = ta.get_refined_cell_positions_and_areas(g["denoised"], g["stack"][3], dict(ct))
    assert len(shape_calls) == 0
    regs = [r for v in list(cell_pos.values()) + list(cell_clusters.values()) for r in v]
    assert len(regs) > 10
    rows = np.array([_row_of(r) for r in regs])
    assert len(shape_calls) == 1
    lab = g["rf_labels"]
    stats, shape = region_table(lab), shape_table(lab)
    idx = np.array([r.label - 1 for r in regs])
    for r in regs:
        assert int(r.area) == stats[r.label - 1, 0]
    _assert_inside_bound(rows, exact_properties(stats[idx], shape[idx]), "refined regions")
