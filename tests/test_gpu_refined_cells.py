"""Refined ROIs related to the class-map components they split (refine_boundaries.py:1-12, goal 2) against numpy
restatements: ops.label_parent (np.unique over packed (r, a) keys, then a lexsort argmax), the refined / cell_resolution /
frames_refined tables of FramePipeline.tables(refined=True), their neighbour tables, run_sharded and the drop-in."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CT3 = {1: "3D05", 2: "6B07", 3: "Particle", 4: "C3M10", 5: "Background"}
SCALE_TABLE = 512.0 / 19.0


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")


def np_label_parent(A, R, counts_r, cap, cls_a=None):
    B = A.shape[0]
    parent = np.zeros((B, cap), np.int64)
    px = np.zeros((B, cap), np.int64)
    nov = np.zeros((B, cap), np.int64)
    cls = np.zeros((B, cap), np.int64)
    over = np.zeros(B, np.int64)
    for b in range(B):
        n = min(int(counts_r[b]), cap)
        a = A[b].ravel().astype(np.int64)
        r = R[b].ravel().astype(np.int64)
        ok = (r >= 1) & (r <= n) & (a >= 1)
        u, c = np.unique((r[ok] << 32) | a[ok], return_counts=True)
        ur, ua = u >> 32, u & 0xFFFFFFFF
        o = np.lexsort((ua, -c, ur))
        ur, ua, c = ur[o], ua[o], c[o]
        first = np.r_[True, ur[1:] != ur[:-1]] if ur.size else np.zeros(0, bool)
        parent[b, ur[first] - 1] = ua[first]
        px[b, ur[first] - 1] = c[first]
        nov[b] = np.bincount(ur, minlength=cap + 1)[1:cap + 1]
        p = parent[b]
        over[b] = int((p > cap).any())
        if cls_a is not None:
            inside = (p >= 1) & (p <= cap)
            cls[b, inside] = cls_a[b, p[inside] - 1]
    return parent, px, nov, cls, over


def _run_lp(A, R, counts, cap, cls_a=None, stats=False):
    from particle_col_image_segmentation_amd import ops
    dev = torch.device("cuda")
    tA = A if isinstance(A, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(A, np.int32)).to(dev)
    tR = R if isinstance(R, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(R, np.int32)).to(dev)
    tc = torch.from_numpy(np.asarray(counts, np.int32)).to(dev)
    st = None
    if stats:
        st, _, _, _ = ops.region_reduce(tR.clone(), tc, cap=cap)  # (an aligned copy)
    tcls = None if cls_a is None else torch.from_numpy(np.asarray(cls_a, np.uint8)).to(dev)
    out = ops.label_parent(tA, tR, tc, cls_a=tcls, cap=cap, stats_r=st, return_spilled=True)
    torch.cuda.synchronize()
    return [o.cpu().numpy().astype(np.int64) for o in out]


def _check_lp(A, R, counts, cap, cls_a=None, stats=False, Ah=None, Rh=None):
    got = _run_lp(A, R, counts, cap, cls_a, stats)
    Ah = A if Ah is None else Ah
    Rh = R if Rh is None else Rh
    exp = np_label_parent(Ah, Rh, counts, cap, cls_a)
    for g, e, name in zip(got[:5], exp, ("parent", "parent_px", "n_overlap", "cls_r", "overflow")):
        np.testing.assert_array_equal(g, e, err_msg=name)
    return got


def _blobs(rng, B, H, W, cell, n_lab, zero=0.2):
    out = np.zeros((B, H, W), np.int32)
    gh, gw = -(-H // cell) + 1, -(-W // cell) + 1
    for b in range(B):
        g = rng.integers(1, n_lab + 1, (gh, gw))
        g[rng.random((gh, gw)) < zero] = 0
        oy, ox = rng.integers(0, cell, 2)
        out[b] = np.kron(g, np.ones((cell, cell), np.int64))[oy:oy + H, ox:ox + W]
    return out


@pytest.mark.parametrize("W", [1, 3, 63, 1021, 1024])
def test_label_parent_random_blobs(W):
    _need_gpu()
    rng = np.random.default_rng(W)
    B, H = 3, 97
    A = _blobs(rng, B, H, W, 7, 300)
    R = _blobs(rng, B, H, W, 5, 400)
    counts = [400, 120, 0]
    cap = 400
    cls_a = rng.integers(0, 6, (B, cap))
    for stats in (False, True):
        _check_lp(A, R, counts, cap, cls_a, stats)


def test_label_parent_ties_background_and_empty():
    _need_gpu()
    A = np.zeros((2, 8, 16), np.int32)
    R = np.zeros((2, 8, 16), np.int32)
    R[0, 0:4, 0:8] = 1
    A[0, 0:4, 0:4] = 3  # half / half: the tie goes to the smaller label
    A[0, 0:4, 4:8] = 2
    R[0, 4:8, 0:8] = 2  # on A = 0 only: no parent
    R[0, 0:8, 8:16] = 3
    A[0, 0:8, 8:16] = 5
    A[0, 0, 8] = 0  # ignored pixel
    got = _check_lp(A, R, [3, 0], 8, np.arange(1, 17).reshape(2, 8))
    assert got[0][0, :3].tolist() == [2, 0, 5] and got[1][0, :3].tolist() == [16, 0, 63]
    assert got[2][0, :3].tolist() == [2, 0, 1] and got[3][0, :3].tolist() == [2, 0, 5]
    assert (got[0][1] == 0).all() and got[4].tolist() == [0, 0]


def test_label_parent_many_components_take_the_spill_path():
    _need_gpu()
    rng = np.random.default_rng(5)
    H = W = 256
    A = np.zeros((2, H, W), np.int32)
    R = np.zeros((2, H, W), np.int32)
    R[0, :32, :32] = 1  # 21 components: more than the 16 candidate slots
    A[0, :32, :32] = (np.arange(32 * 32).reshape(32, 32) // 50) + 1
    R[0, 32:, :] = 2  # several thousand components, two windows apart and beyond
    A[0, 32:, :] = rng.integers(1, 9000, (H - 32, W))
    A[0, 40:50, 10:20] = 8999  # a clear winner in the last window
    R[1] = 1  # the whole second frame, labels in a window far from the first
    A[1] = rng.integers(50000, 50020, (H, W))
    A[1, :, :3] = 0
    for stats in (False, True):
        got = _check_lp(A, R, [2, 1], 60000, stats=stats)
        assert got[5][0] == 3 and got[4].tolist() == [0, 0]
    assert got[0][0, 1] == 8999 and got[2][0, 1] > 4096


def test_label_parent_sixteen_slots_exactly():
    _need_gpu()
    A = np.zeros((1, 8, 64), np.int32)
    R = np.zeros((1, 8, 64), np.int32)
    R[0, :4, :32] = 1
    A[0, :4, :32] = np.arange(32)[None] // 2 + 1  # 16 components, 8 px each: a 16-way tie, fits the slots
    R[0, 4:, :34] = 2
    A[0, 4:, :34] = np.arange(34)[None] // 2 + 40  # 17 components: spills
    A[0, 4:, 33] = 40  # ... and 40 wins
    got = _check_lp(A, R, [2], 64)
    assert got[0][0, :2].tolist() == [1, 40] and got[2][0, :2].tolist() == [16, 17] and got[5][0] == 1


def test_label_parent_cap_flag_and_skipped_rows():
    _need_gpu()
    A = np.zeros((3, 16, 16), np.int32)
    R = np.zeros((3, 16, 16), np.int32)
    R[0, :8] = 1
    A[0, :8] = 7  # parent above cap = 4: flagged
    R[1, :8] = 1
    A[1, :8] = 2
    R[1, 8:] = 9  # R label above cap: skipped
    A[1, 8:] = 3
    R[2, :4] = 1
    A[2, :4, :10] = 7  # the larger overlap is label 7, above cap: flagged too
    A[2, :4, 10:] = 1
    got = _check_lp(A, R, [1, 9, 1], 4, np.full((3, 4), 3))
    assert got[4].tolist() == [1, 0, 1] and got[0][1, 0] == 2 and got[3][0, 0] == 0


def test_label_parent_odd_offset_view_and_many_frames():
    _need_gpu()
    rng = np.random.default_rng(9)
    B, H, W = 64, 40, 64
    A = _blobs(rng, B, H, W, 6, 200)
    R = _blobs(rng, B, H, W, 4, 500)
    counts = rng.integers(0, 501, B)
    cls_a = rng.integers(0, 6, (B, 500))
    dev = torch.device("cuda")
    flatA = torch.zeros(B * H * W + 1, dtype=torch.int32, device=dev)
    flatR = torch.zeros(B * H * W + 3, dtype=torch.int32, device=dev)
    flatA[1:].copy_(torch.from_numpy(A.ravel()))
    flatR[3:].copy_(torch.from_numpy(R.ravel()))
    tA, tR = flatA[1:].view(B, H, W), flatR[3:].view(B, H, W)
    assert tA.data_ptr() % 16 and tR.data_ptr() % 16
    _check_lp(tA, tR, counts, 500, cls_a, True, A, R)
    _check_lp(A, R, counts, 500, cls_a, True)


def test_label_parent_4096_frame():
    _need_gpu()
    rng = np.random.default_rng(4096)
    H = W = 4096
    A = _blobs(rng, 1, H, W, 3, 20000)
    y, x = np.mgrid[:H, :W]
    R = ((y // 64) * 64 + x // 64 + 1).astype(np.int32)[None]  # 64 x 64 tiles, one label each
    R[0, :1024, :1024] = 1  # one ROI over a quarter of the frame: thousands of components, five label windows
    got = _check_lp(A, R, [4096], 4096, stats=True)
    assert got[5][0] >= 1 and got[2][0, 0] > 4096


# ---------------------------------------------------------------- pipeline tables against a restatement

def _np_floor_div(a, b):
    return np.floor_divide(np.float64(a), np.float64(b))


def restate(pipe, res, tabs):
    """refined / cell_resolution / frames_refined from the downloaded label images and the existing tables."""
    tb = pipe.tables_
    labels = res["labels"].cpu().numpy()
    ws = res["ws_labels"].cpu().numpy()
    den = res["denoised"].cpu().numpy()
    nm = res["n_markers"].cpu().numpy()
    cap = res["stats"].shape[1]
    B = labels.shape[0]
    cls_a = np.zeros((B, cap), np.int64)
    for b in range(B):
        u, idx = np.unique(labels[b].ravel(), return_index=True)
        keep = (u >= 1) & (u <= cap)
        cls_a[b, u[keep] - 1] = den[b].ravel()[idx[keep]]
    parent, px, nov, cls, _ = np_label_parent(labels, ws, nm, cap, cls_a)
    rois, cells, fr = tabs["rois"], tabs["cells"], tabs["frames"]
    K = len(tb.slot_names)
    frame_ids = fr[:, 0]
    ref_rows, res_rows, frame_rows = [], [], []
    for b, fid in enumerate(frame_ids):
        rr = rois[rois[:, 0] == fid]
        lab = rr[:, 1].astype(np.int64)
        area = rr[:, 2].astype(np.int64)
        c = cls[b, lab - 1]
        slot = tb.slot[c].astype(np.int64)
        kind = np.zeros(len(lab), np.int64)
        ok = slot != 255
        s_ok = np.where(ok, slot, 0)
        mc, mu = tb.min_cell[np.minimum(s_ok, len(tb.min_cell) - 1)], tb.min_cluster[np.minimum(s_ok, len(tb.min_cluster) - 1)]
        kind[ok & (area >= mc) & (area < mu)] = 1
        kind[ok & (area >= mu)] = 2
        ncell = np.ones(len(lab), np.int64) * (kind == 1)
        nan = 0
        for t in range(K):
            cl = (kind == 2) & (slot == t)
            ce = (kind == 1) & (slot == t)
            if cl.any():
                if not ce.any():
                    ncell[cl] = -1
                    nan = 1
                else:
                    avg = np.float64(area[ce].sum()) / np.float64(ce.sum())
                    ncell[cl] = [int(_np_floor_div(x, avg)) for x in area[cl]]
        ref_rows.append(np.stack([rr[:, 0], lab, parent[b, lab - 1], px[b, lab - 1], nov[b, lab - 1], c, kind, ncell, rr[:, 2],
                                  rr[:, 3], rr[:, 4]], axis=1).astype(np.float64))
        cc = cells[cells[:, 0] == fid]
        live = kind >= 1
        pl = parent[b, lab - 1]
        row = [fid, nan]
        out = []
        for a_lab, a_cls, a_kind, a_cells in cc[:, [1, 2, 3, 11]].astype(np.int64):
            m = live & (pl == a_lab)
            ch = int(m.sum())
            resolved = int(a_kind == 2 and ch >= 2)
            integ = 1 if a_kind == 1 else ((-1 if (ncell[m] < 0).any() else int(ncell[m].sum())) if resolved else a_cells)
            out.append((fid, a_lab, ch, resolved, integ, tb.slot[a_cls], a_kind))
        res_rows.append(np.array([o[:5] for o in out], np.float64).reshape(-1, 5))
        for t in range(K):
            mine = [o for o in out if o[5] == t]
            integ = [o[4] for o in mine]
            row += [((kind == 1) & (slot == t)).sum(), ((kind == 2) & (slot == t)).sum(),
                    sum(1 for o in mine if o[6] == 2 and o[3]), sum(1 for o in mine if o[6] == 2 and not o[3]),
                    -1 if any(v < 0 for v in integ) else sum(integ)]
        frame_rows.append(row)
    return (np.concatenate(ref_rows).reshape(-1, 11), np.concatenate(res_rows).reshape(-1, 5),
            np.array(frame_rows, np.float64))


def _check_refined(pipe, res, tabs, e):
    rf, rs, fr = restate(pipe, res, tabs)
    np.testing.assert_array_equal(tabs["refined"], rf)
    np.testing.assert_array_equal(tabs["cell_resolution"], rs)
    np.testing.assert_array_equal(tabs["frames_refined"], fr)
    from test_gpu_neighbours import brute
    K = len(pipe.tables_.slot_names)
    pts = rf[rf[:, 6] >= 1]
    frames = tabs["frames"][:, 0]
    foff = np.searchsorted(pts[:, 0], np.concatenate([frames, [np.inf]]), side="left").astype(np.int64)
    slot = pipe.tables_.slot[pts[:, 5].astype(np.int64)].astype(np.int32)
    xy = np.stack([pts[:, 10] + 1.0, pts[:, 9] + 1.0], axis=1)
    ed, ei, eh = brute(xy, slot, pts[:, 1].astype(np.int32), foff, K, SCALE_TABLE, e)
    nb, ph = tabs["refined_neighbours"], tabs["refined_pair_hist"]
    np.testing.assert_array_equal(nb[:, :3], np.stack([pts[:, 0], pts[:, 1], slot], axis=1))
    np.testing.assert_array_equal(nb[:, 3:3 + K], ed)
    np.testing.assert_array_equal(nb[:, 3 + K:], ei)
    np.testing.assert_array_equal(ph[:, 3:], eh.reshape(-1, eh.shape[2]))
    return rf, rs


@pytest.mark.parametrize("shape,graph", [((4, 256, 256), False), ((4, 256, 256), True), ((3, 200, 250), False),
                                         ((8, 1024, 1024), False)])
def test_pipeline_refined_tables(shape, graph):
    _need_gpu()
    from particle_col_image_segmentation_amd import synth
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    B, H, W = shape
    dev = torch.device("cuda")
    pipe = FramePipeline(CT3 if W == 250 else None, graph=graph, lanes=2 if graph else None)
    stacks = synth.gen_batch_torch(9100 + H + W, B, H, W, dev)
    buf = torch.empty_like(stacks)
    buf.copy_(stacks)
    res = pipe.run(buf)
    e = np.linspace(0.0, 8.0, 33)
    tabs = pipe.tables(res, check=False, distances=True, neighbours=True, pair_edges=e, refined=True)
    plain = pipe.tables(res, check=False, distances=True, neighbours=True, pair_edges=e)
    new = {"refined", "cell_resolution", "frames_refined", "refined_neighbours", "refined_pair_hist"}
    assert set(tabs) == set(plain) | new | {k + "_columns" for k in new}
    for k in plain:
        if not k.endswith("_columns"):
            np.testing.assert_array_equal(tabs[k], plain[k], err_msg=k)
    rf, rs = _check_refined(pipe, res, tabs, e)
    assert rf.shape[0] == tabs["rois"].shape[0] > 10 and rs.shape[0] == tabs["cells"].shape[0]
    assert (rf[:, 2] > 0).any() and (rf[:, 6] >= 1).any()
    only = pipe.tables(res, check=False, refined=True)
    for k in ("refined", "cell_resolution", "frames_refined"):
        np.testing.assert_array_equal(only[k], tabs[k])
    assert "refined_neighbours" not in only


def test_run_sharded_forwards_refined():
    _need_gpu()
    from particle_col_image_segmentation_amd import synth
    from particle_col_image_segmentation_amd.distributed import run_sharded
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    dev = torch.device("cuda")
    pipe = FramePipeline(CT3)
    stacks = synth.gen_batch(9300, 6, 192, 192)
    make_batch = lambda ids: torch.from_numpy(stacks[list(ids)]).to(dev)
    e = np.linspace(0.0, 6.0, 17)
    kw = dict(batch=4, check=False, refined=True, neighbours=True, pair_edges=e)
    host = run_sharded(6, make_batch, pipe, **kw)
    forced = run_sharded(6, make_batch, pipe, force_gather=True, device=dev, **kw)
    pipe.synchronize()
    keys = ("refined", "cell_resolution", "frames_refined", "refined_neighbours", "refined_pair_hist")
    per = [pipe.tables(pipe.run(make_batch(ids)), frame_ids=ids, check=False, refined=True, neighbours=True, pair_edges=e)
           for ids in ([0, 1, 2, 3], [4, 5])]
    for k in keys:
        np.testing.assert_array_equal(host[k], forced[k], err_msg=k)
        np.testing.assert_array_equal(host[k], np.concatenate([p[k] for p in per]), err_msg=k)
    plain = run_sharded(6, make_batch, pipe, batch=4, check=False)
    assert not any(k in plain for k in keys)


def test_dropin_refined_cell_positions(tmp_path):
    _need_gpu()
    from particle_col_image_segmentation_amd import synth
    from particle_col_image_segmentation_amd import tiff_analysis as ta
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    ct = dict(synth.CELL_TYPES_5)
    stack = synth.gen_batch(9400, 1, 256, 256)
    pipe = FramePipeline(ct)
    res = pipe.run(torch.from_numpy(stack).cuda())
    tabs = pipe.tables(res, check=False, refined=True)
    z = res["denoised"][0].cpu().numpy()
    bm = stack[0, pipe.boundary_plane]
    if tabs["frames_refined"][0, 1]:
        with pytest.raises(ValueError, match="NaN"):
            ta.get_refined_cell_positions_and_areas(z, bm, ct)
        return
    cell_pos, clusters, particle_area, resolution = ta.get_refined_cell_positions_and_areas(z, bm, ct)
    rf, rs = tabs["refined"], tabs["cell_resolution"]
    names = pipe.tables_.slot_names
    got = sorted((r.label, r.parent, 1, 1) for regs in cell_pos.values() for r in regs)
    got += sorted((r.label, r.parent, 2, r.cells) for regs in clusters.values() for r in regs)
    exp = sorted((int(r[1]), int(r[2]), 1, 1) for r in rf if r[6] == 1)
    exp += sorted((int(r[1]), int(r[2]), 2, int(r[7])) for r in rf if r[6] == 2)
    assert got == exp and len(got) > 0
    for name, regs in cell_pos.items():
        for r in regs:
            row = rf[rf[:, 1] == r.label][0]
            assert names[pipe.tables_.slot[int(row[5])]] == name and r.area == row[8]
            assert r.centroid == (row[9], row[10])
    assert particle_area == int(pipe.tables(res, check=False)["frames"][0, 3])
    fr = tabs["frames_refined"][0]
    for t, name in enumerate(names):
        d = resolution.get(name, {"resolved": [], "residual": [], "count_integrated": 0})
        assert len(d["resolved"]) == fr[2 + 5 * t + 2] and len(d["residual"]) == fr[2 + 5 * t + 3]
        assert d["count_integrated"] == fr[2 + 5 * t + 4]
        for lab in d["resolved"]:
            assert rs[rs[:, 1] == lab][0, 3] == 1
    nn = ta.get_cell_neighbour_distances(cell_pos)
    assert set(nn) == set(cell_pos)
    out = tmp_path / "pos.csv"
    ta.write_cell_position_info(cell_pos, clusters, str(out), particle_area)
    assert len(out.read_text().splitlines()) == 1 + len(got)
    with pytest.raises(ValueError):
        ta.get_refined_cell_positions_and_areas(z, bm[:-1], ct)
