"""Local neighbourhoods on the device (csrc/local_counts.hip, local.py, FramePipeline.neighbourhoods) against the numpy
restatements of tests/local_reference.py and against the two device routes whose per-cell marks they are
(``spatial.window_pair_counts``, ``ops.point_neighbours``).  Everything is compared with assert_array_equal: no tolerance; the
derived float columns by their bits."""
import numpy as np
import pytest

import local_reference as lr
import ops_contract_cases as cc
import workspace_cases as wc
from test_gpu_window_pairs import SCALE_TABLE, edges_for_reach
from test_window_pairs_cpu import masks

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MASKS = ("empty", "full", "checkerboard", "random60", "blob")
LATTICE_EDGES = np.array([0.0, 1.0, np.sqrt(2.0), 2.0, np.sqrt(5.0), 5.0, np.sqrt(50.0), 9.0])  # exact lattice distances: [lo, hi)


@pytest.fixture(scope="module")
def lc():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")
    from particle_col_image_segmentation_amd import local
    return local


def query_set(H, W, R):
    """the four corners, a pixel on each edge, the centre (twice), (-1, -1), just outside each side, farther than R away"""
    return np.array([(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 3), (H // 2, 0), (H // 3, W - 1),
                     (H // 2, W // 2), (H // 2, W // 2), (-1, -1), (-1, W // 2), (H, W // 2), (H // 2, -1), (H // 2, W),
                     (H + R + 3, W // 2), (H // 2, -R - 2), (-R - 1, -R - 1), (H // 2, W + R)], np.int32)


def check(lc, planes, queries, foff, edges, scale=1.0, C=1):
    """one call against the brute restatement; returns the device result as numpy"""
    from particle_col_image_segmentation_amd import ops
    counts, area = lc.disk_counts(torch.from_numpy(planes).cuda(), torch.from_numpy(np.asarray(queries, np.int32).reshape(-1, 2)).cuda(),
                                  torch.from_numpy(np.asarray(foff, np.int64)).cuda(), edges, scale, sets=C)
    counts, area = counts.cpu().numpy(), area.cpu().numpy()
    thr = ops.surface_thresholds(edges, scale)
    want, want_area = lr.disk_counts(planes, queries, foff, thr, C)
    assert counts.dtype == np.int32 and area.dtype == np.int64 and counts.shape == want.shape and area.shape == want_area.shape
    bad = np.argwhere(counts != want)
    assert bad.size == 0, "query %d (%s), set %d, bin %d: %d, expected %d" % (
        bad[0][0], np.asarray(queries).reshape(-1, 2)[bad[0][0]], bad[0][1], bad[0][2], counts[tuple(bad[0])], want[tuple(bad[0])])
    np.testing.assert_array_equal(area, want_area)
    return counts, area


def batch_of(H, W, seed, garbage=True):
    """the five masks as set 0 of five frames, random bits above it"""
    ms = masks(H, W, seed=seed)
    planes = np.stack([ms[k] for k in MASKS]).astype(np.uint8)
    if garbage:
        planes |= (np.random.default_rng([seed, H, W, 1]).integers(0, 128, planes.shape).astype(np.uint8) << 1)
    return planes


@pytest.mark.parametrize("W", [1, 31, 32, 33, 63, 64, 65, 70, 129])
def test_widths_heights_reaches_and_masks(lc, W):
    """tail bits and one to five words; heights around a wave's rows per pass; every reach class; queries on, at and off the
    image"""
    rows = lc.local_rows()
    for H in (1, 2, 37, rows - 1, rows + 1):
        planes = batch_of(H, W, W)
        for R in ((0, 1, 31, 32, 33, 64, 65, max(H, W) + 7) if H in (2, rows + 1) else (rows + 2, 33)):
            q = query_set(H, W, R)
            queries = np.concatenate([q] * len(MASKS))
            foff = np.arange(len(MASKS) + 1) * len(q)
            counts, area = check(lc, planes, queries, foff, edges_for_reach(R))
            per = counts.reshape(len(MASKS), len(q), 1, -1)
            assert per[MASKS.index("empty")].sum() == 0 and area[MASKS.index("full"), 0] == H * W
            assert (per[:, 8] == per[:, 9]).all()  # the duplicated query
            assert per[:, -4:].sum() == 0          # farther than R from the image


def test_sets_batch_order_lattice_edges_and_a_second_scale(lc):
    H, W = 37, 70
    rng = np.random.default_rng(11)
    q = query_set(H, W, 8)
    for C in (1, 3, 8):
        planes = rng.integers(0, 256, (3, H, W)).astype(np.uint8)  # independent random bits per set, garbage above bit C
        queries = np.concatenate([q, q[:5], q[3:]])
        foff = np.array([0, len(q), len(q) + 5, len(queries)])
        counts, area = check(lc, planes, queries, foff, LATTICE_EDGES, C=C)
        order = [2, 0, 1]
        parts = [queries[foff[b]:foff[b + 1]] for b in order]
        c2, a2 = check(lc, planes[order], np.concatenate(parts), np.concatenate([[0], np.cumsum([len(p) for p in parts])]), LATTICE_EDGES, C=C)
        np.testing.assert_array_equal(c2, np.concatenate([counts[foff[b]:foff[b + 1]] for b in order]))
        np.testing.assert_array_equal(a2, area[order])
        check(lc, planes, queries, foff, LATTICE_EDGES / 9.95, scale=9.95, C=C)  # the same bins at another scale
    # [lo, hi) on the full mask around the centre: bin [5, sqrt 50) holds d2 = 25 .. 49, (5, 5) and (1, 7) open the next
    full = np.ones((1, H, W), np.uint8)
    counts, _ = check(lc, full, [(18, 35)], [0, 1], LATTICE_EDGES)
    ring = lambda lo, hi: sum(1 for dy in range(-9, 10) for dx in range(-9, 10) if lo <= dy * dy + dx * dx < hi)
    assert counts[0, 0].tolist() == [ring(0, 1), ring(1, 2), ring(2, 4), ring(4, 5), ring(5, 25), ring(25, 50), ring(50, 81)]
    assert counts[0, 0, 0] == 1 and counts[0, 0, 1] == 4 and ring(25, 26) == 12 and ring(50, 51) == 12  # (3, 4), (5, 0); (5, 5), (1, 7)


def test_frames_without_query_and_no_query_at_all(lc):
    H, W = 9, 33
    planes = batch_of(H, W, 4)[:3]
    q = query_set(H, W, 5)
    check(lc, planes, q, [0, 0, len(q), len(q)], edges_for_reach(5), C=2)  # only the middle frame has queries
    counts, area = check(lc, planes, np.zeros((0, 2), np.int32), [0, 0, 0, 0], edges_for_reach(5), C=2)
    assert counts.shape == (0, 2, 6) and area[:, 0].tolist() == [0, H * W, int((planes[2] & 1).sum())]


@pytest.mark.parametrize("m", [1, 65, 1024])
def test_bin_counts(lc, m):
    """one bin (64 row phases), one more than a pass of bins, the most -- on a frame of fewer rows than a pass and on one with
    more rows than a pass and a reach beyond them"""
    assert lc.local_bins() == 64
    for H, W in ((33, 65), (lc.local_rows() + 6, 37)):
        planes = batch_of(H, W, m)[3:]
        q = query_set(H, W, 40)
        queries = np.concatenate([q, q])
        foff = [0, len(q), 2 * len(q)]
        counts, _ = check(lc, planes, queries, foff, np.linspace(0.0, 40.0, m + 1), C=2)
        assert counts.sum() > 0
        check(lc, planes, queries, foff, np.concatenate([np.linspace(0.0, 40.0, m + 1)[:-1], [np.hypot(H, W) + 1.0]]), C=2)


def test_ring_counts_over_the_window_are_the_window_pair_counts(lc):
    """the cross-route check: with every window pixel as a query the column sums are spatial.window_pair_counts' bins"""
    from particle_col_image_segmentation_amd import spatial
    ms = masks(37, 70, seed=5)
    batch = np.stack([ms["blob"], ms["random60"], ms["empty"], ms["checkerboard"]])
    e = edges_for_reach(33)
    queries = np.concatenate([np.argwhere(M) for M in batch]).astype(np.int32)
    foff = np.concatenate([[0], np.cumsum([int(M.sum()) for M in batch])]).astype(np.int64)
    x = torch.from_numpy(batch.astype(np.uint8)).cuda()
    counts, area = lc.disk_counts(x, torch.from_numpy(queries).cuda(), torch.from_numpy(foff).cuda(), e, 1.0, sets=1)
    hist = spatial.window_pair_counts(x, e, 1.0).cpu().numpy()
    frame = torch.repeat_interleave(torch.arange(4).cuda(), torch.from_numpy(np.diff(foff)).cuda())
    sums = torch.zeros((4, len(e) - 1), dtype=torch.int64).cuda().index_add_(0, frame, counts[:, 0].to(torch.int64)).cpu().numpy()
    np.testing.assert_array_equal(sums, hist[:, 1:-1])
    np.testing.assert_array_equal(area[:, 0].cpu().numpy(), hist[:, 0])
    assert sums[0].min() > 0 and sums[2].sum() == 0


# ------------------------------------------------------------------ point counts
def point_batch(seed, sizes, K, extent=10):
    """frame-contiguous points on a half-pixel lattice (duplicates, distances exactly at an edge), slots -1 .. K"""
    rng = np.random.default_rng([seed, K, len(sizes)])
    n = sum(sizes)
    xy = rng.integers(0, 2 * extent, (n, 2)).astype(np.float64) / 2.0
    slot = rng.integers(-1, K + 1, n).astype(np.int32)
    foff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    for b in range(len(sizes)):
        if sizes[b] >= 2:
            xy[foff[b] + 1], slot[foff[b]:foff[b] + 2] = xy[foff[b]], 0  # a duplicate position
    return xy, slot, foff


def check_points(lc, xy, slot, foff, K, scale, edges):
    from particle_col_image_segmentation_amd import ops
    dev = [torch.from_numpy(a).cuda() for a in (xy, slot, foff)]
    got = lc.point_counts(dev[0], dev[1], dev[2], K, scale, edges).cpu().numpy()
    want = lr.point_counts(xy, slot, foff, K, scale, edges)
    assert got.dtype == np.int32 and got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, "point %d, slot %d, bin %d: %d, expected %d" % (*bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    # the per-slot sums against the device's own pair histogram
    ids = torch.arange(len(slot), dtype=torch.int32).cuda()
    hist = ops.point_neighbours(dev[0], dev[1], ids, dev[2], K, scale, edges)[2].cpu().numpy()
    frame = np.searchsorted(foff, np.arange(len(slot)), side="right") - 1
    q = 0
    for a in range(K):
        for b in range(a, K):
            for f in range(len(foff) - 1):
                sel = (frame == f) & (slot == a)
                np.testing.assert_array_equal(got[sel][:, b].sum(axis=0), hist[f, q, 1:-1] * (2 if a == b else 1), err_msg=str((a, b, f)))
            q += 1
    return got


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_point_counts_frame_sizes_slots_duplicates_and_edge_distances(lc, K):
    tile = lc.local_point_tile()
    assert tile == 64
    xy, slot, foff = point_batch(3, (0, 1, 2, tile - 1, tile, tile + 1, 0, 2 * tile - 1, 2 * tile + 1), K)
    edges = np.array([0.0, 0.5, 1.0, np.sqrt(2.0), 2.0, np.sqrt(5.0), 2.5, 5.0])  # distances of the half-pixel lattice
    got = check_points(lc, xy, slot, foff, K, 1.0, edges)
    typed = (slot >= 0) & (slot < K)
    assert (got[~typed] == -1).all() and (~typed).any() and got[typed][:, 0, 0].sum() >= 2  # the duplicates, in bin 0
    check_points(lc, xy, slot, foff, K, 1.5, edges)
    check_points(lc, xy * 3.0, slot, foff, K, 3.0, edges)  # the same distances at another scale: at the edges up to the rounding of sqrt


@pytest.mark.parametrize("m", [1, 910, 911, 1024])
def test_point_counts_bin_counts(lc, m):
    """four slots and 910 bins are the last shape whose block has four waves (8 (m + 1) + 16 K m <= 64 KB), 911 the first with
    two"""
    xy, slot, foff = point_batch(8, (70, 0, 9), 4, extent=20)
    got = check_points(lc, xy, slot, foff, 4, 1.0, np.linspace(0.0, 30.0, m + 1))
    assert got[got >= 0].sum() > 0


# ------------------------------------------------------------------ prior contents of outputs and workspace
def test_prior_state_of_outputs_and_workspace(lc, monkeypatch):
    """counts, area and the workspaces pre-filled with each of workspace_cases.STATES: equal results, the red zones behind the
    workspace and around the outputs untouched"""
    from particle_col_image_segmentation_amd import ops
    H, W = 37, 70
    planes = torch.from_numpy(batch_of(H, W, 9)[2:]).cuda()
    q = query_set(H, W, 33)
    queries = torch.from_numpy(np.concatenate([q] * 3)).cuda()
    foff = torch.from_numpy(np.arange(4, dtype=np.int64) * len(q)).cuda()
    other = (torch.from_numpy(batch_of(19, 129, 2)[:2]).cuda(), torch.from_numpy(np.concatenate([query_set(19, 129, 33)] * 2)).cuda(),
             torch.from_numpy(np.arange(3, dtype=np.int64) * len(q)).cuda())
    e = edges_for_reach(33)
    xy, slot, pf = point_batch(5, (70, 0, 9), 3)
    pts = [torch.from_numpy(a).cuda() for a in (xy, slot, pf)]
    state, handed, snaps = ["zeros"], [], {}
    real_empty = torch.empty

    def ws(nbytes, device):
        fill = wc.state_fill(state[0], nbytes, snaps.get(state[0]))
        whole = torch.from_numpy(fill).to(device)
        handed.append((nbytes, whole, wc.red_zone(fill, nbytes)))
        return whole[:max(nbytes, 256)]

    class Proxy:
        def __getattr__(self, name):
            return getattr(torch, name)

        def empty(self, shape, dtype=None, device=None):
            n = int(np.prod(shape))
            pad = wc.RED_ZONE // 8
            whole = real_empty((n + 2 * pad,), dtype=dtype, device=device)
            whole.view(torch.uint8).fill_({"zeros": 0, "ones": 0xFF}.get(state[0], 0x5A))
            handed.append((None, whole, whole.clone(), pad, n))
            return whole[pad:pad + n].view(shape)

    monkeypatch.setattr(ops, "_ws", ws)
    monkeypatch.setattr(lc, "torch", Proxy())

    def run(args):
        del handed[:]
        counts, area = lc.disk_counts(args[0], args[1], args[2], e, 1.0, sets=3)
        near = lc.point_counts(pts[0], pts[1], pts[2], 3, 1.0, e)
        torch.cuda.synchronize()
        assert len(handed) == 5  # two workspaces, three outputs
        for h in handed:
            if h[0] is not None:
                assert wc.first_changed(wc.red_zone(h[1], h[0]).cpu().numpy(), h[2]) < 0, "a write behind the workspace"
                if h[0] > 4096:
                    leftover = h[1][:h[0]].cpu().numpy()  # (the larger one: disk_counts')
            else:
                _, whole, before, pad, n = h
                assert torch.equal(whole[:pad].view(torch.uint8), before[:pad].view(torch.uint8)), "a write in front of an output"
                assert torch.equal(whole[pad + n:].view(torch.uint8), before[pad + n:].view(torch.uint8)), "a write behind an output"
        return counts.cpu().numpy().copy(), area.cpu().numpy().copy(), near.cpu().numpy().copy(), leftover

    snaps["leftover-other"] = run(other)[3]
    snaps["leftover-same"] = run((torch.flip(planes, dims=[0]), queries, foff))[3]
    base = None
    for s in wc.STATES:
        state[0] = s
        got = run((planes, queries, foff))[:3]
        if base is None:
            base = got
            want = lr.disk_counts(planes.cpu().numpy(), queries.cpu().numpy(), foff.cpu().numpy(), ops.surface_thresholds(e, 1.0), 3)
            np.testing.assert_array_equal(got[0], want[0])
            np.testing.assert_array_equal(got[1], want[1])
            np.testing.assert_array_equal(got[2], lr.point_counts(xy, slot, pf, 3, 1.0, e))
        for a, b in zip(got, base):
            np.testing.assert_array_equal(a, b, err_msg=s)


def test_refusals_come_before_a_launch(lc, monkeypatch):
    """on device tensors, with the two ways into the library replaced: a refused call never reaches them"""
    from particle_col_image_segmentation_amd import ops, spatial
    cc.install(ops, monkeypatch)
    be = cc.Backend(ops, "cuda", "cpu")
    planes, queries, foff = be.tensor(torch.uint8, (2, 9, 11)), be.tensor(torch.int32, (7, 2)), be.tensor(torch.int64, (3,))
    xy, slot = be.tensor(torch.float64, (7, 2)), be.tensor(torch.int32, (7,))
    e = [0.0, 1.0, 2.5]
    with pytest.raises(cc.Reached):
        lc.disk_counts(planes, queries, foff, e, 1.0)
    with pytest.raises(cc.Reached):
        lc.point_counts(xy, slot, foff, 2, 1.0, e)
    for bad, raises in ((dict(planes=planes.cpu()), TypeError), (dict(planes=planes.to(torch.int32)), TypeError), (dict(planes=planes[0]), ValueError),
                        (dict(queries=queries.to(torch.int64)), TypeError), (dict(queries=be.tensor(torch.int32, (7, 3))), ValueError),
                        (dict(frame_offsets=be.tensor(torch.int64, (4,))), ValueError), (dict(frame_offsets=foff.cpu()), TypeError),
                        (dict(edges=[0.0, 2.0, 1.0]), ValueError), (dict(edges=[0.0, spatial.MAX_REACH + 1.5]), ValueError),
                        (dict(scale=0.0), ValueError), (dict(sets=9), ValueError)):
        kw = dict(planes=planes, queries=queries, frame_offsets=foff, edges=e, scale=1.0)
        kw.update(bad)
        with pytest.raises(raises):
            lc.disk_counts(**kw)
    for bad, raises in ((dict(xy=xy.cpu()), TypeError), (dict(xy=xy.to(torch.float32)), TypeError), (dict(slot=be.tensor(torch.int32, (8,))), ValueError),
                        (dict(slot=slot.to(torch.int64)), TypeError), (dict(frame_offsets=foff.to(torch.int32)), TypeError),
                        (dict(edges=[0.5, 1.0]), ValueError), (dict(edges=None), ValueError), (dict(K=5), ValueError), (dict(scale=float("nan")), ValueError)):
        kw = dict(xy=xy, slot=slot, frame_offsets=foff, K=2, scale=1.0, edges=e)
        kw.update(bad)
        with pytest.raises(raises):
            lc.point_counts(**kw)
    # an empty batch and an empty point set return without a launch
    assert tuple(lc.disk_counts(be.tensor(torch.uint8, (0, 9, 11)), be.tensor(torch.int32, (0, 2)), be.tensor(torch.int64, (1,)), e, 1.0, sets=2)[0].shape) == (0, 2, 2)
    assert tuple(lc.point_counts(be.tensor(torch.float64, (0, 2)), be.tensor(torch.int32, (0,)), foff, 2, 1.0, e).shape) == (0, 2, 2)


# ------------------------------------------------------------------ the pipeline
@pytest.fixture(scope="module")
def batch(lc):
    from particle_col_image_segmentation_amd import synth
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    pipe = FramePipeline(dict(synth.CELL_TYPES_5))
    stacks = synth.gen_batch(31, 3, 128, 128)
    res = pipe.run(torch.from_numpy(stacks).cuda())
    e = np.concatenate([[0.0], np.sqrt(np.array([4, 25, 50, 100, 400.0])) / SCALE_TABLE, [1.5, 2.5]])
    tabs = pipe.tables(res, check=False)
    return pipe, res, e, tabs


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _planes_of(pipe, res, mask):
    slot = pipe.tables_.slot
    den = res["denoised"].cpu().numpy()
    lut = np.where(slot != 255, np.left_shift(2, np.minimum(slot, 7).astype(np.int64)), 0).astype(np.uint8)
    return (mask != 0).astype(np.uint8) | lut[den]


def test_neighbourhoods_against_the_restatement_and_clustering(batch, lc):
    from particle_col_image_segmentation_amd import ops
    pipe, res, e, tabs = batch
    K, m = len(pipe.tables_.slot_names), len(e) - 1
    fid = [7, 3, 11]
    out = pipe.neighbourhoods(res, e, window="particle", of="cells", frame_ids=fid)
    cols = out["neighbourhoods_columns"]
    assert cols == lc.neighbourhood_columns(list(pipe.tables_.slot_names), e) == lr.columns(list(pipe.tables_.slot_names))
    got = out["neighbourhoods"]
    assert got.dtype == np.float64 and got.shape[1] == len(cols) == 11 + 6 * K
    # the points of pair_hist: the rows of `cells`, positions as the pair tables take them
    cells = tabs["cells"]
    rc = cells[:, 5:7].copy()
    xy = np.stack([rc[:, 1] + 1.0, rc[:, 0] + 1.0], axis=1)
    slot = np.where(pipe.tables_.slot[cells[:, 2].astype(int)] == 255, -1, pipe.tables_.slot[cells[:, 2].astype(int)]).astype(np.int64)
    foff = np.concatenate([[0], np.cumsum([(cells[:, 0] == b).sum() for b in range(3)])]).astype(np.int64)
    mask = ops.particle_mask(res["recreated"], pipe.tables_.particle_value).cpu().numpy()
    planes = _planes_of(pipe, res, mask)
    thr = ops.surface_thresholds(e, SCALE_TABLE)
    want = lr.neighbourhood_rows(fid, xy, rc, slot, cells[:, 1], foff, planes, e, SCALE_TABLE, thr, K)
    np.testing.assert_array_equal(_bits(got), _bits(want))  # NaN placement included
    seen = got[:, 3] == 1
    assert seen.any() and (~seen).any() and np.isfinite(got[seen][:, cols.index("expected_%s" % pipe.tables_.slot_names[0])]).all()
    # summed over the in-window rows of slot a, n_<b> is clustering's obs (twice it when a == b)
    cl = pipe.clustering(res, e, window="particle", of="cells", frame_ids=fid)["clustering"].reshape(3, -1, m, 18)
    names = list(pipe.tables_.slot_names)
    q = 0
    for a in range(K):
        for b in range(a, K):
            for f in range(3):
                rows = got[seen & (got[:, 0] == fid[f]) & (got[:, 2] == a)]
                total = rows[:, cols.index("n_%s" % names[b])].reshape(-1, m).sum(axis=0) if len(rows) else np.zeros(m)
                np.testing.assert_array_equal(total, cl[f, q, :, 10] * (2 if a == b else 1), err_msg=str((a, b, f)))
            q += 1
    assert cl[:, :, :, 10].sum() > 0
    # a window of the caller's: the same mask gives the same table; the refined points run through the same chain
    own = pipe.neighbourhoods(res, e, window=torch.from_numpy(mask).cuda(), of="cells", frame_ids=fid)
    np.testing.assert_array_equal(_bits(own["neighbourhoods"]), _bits(got))
    ref = pipe.neighbourhoods(res, e, window="frame", of="refined")
    assert ref["neighbourhoods"].shape[1] == len(cols) and (ref["neighbourhoods"][:, 3] == 1).all()
    np.testing.assert_array_equal(ref["neighbourhoods"][:, cols.index("cum_win_px")].reshape(-1, m)[:, 0], ref["neighbourhoods"][:, 7].reshape(-1, m)[:, 0])


def test_res_is_only_read(batch):
    pipe, res, e, tabs = batch
    pipe.neighbourhoods(res, e, of="refined")
    again = pipe.tables(res, check=False)
    assert sorted(again) == sorted(tabs)
    for k in tabs:
        np.testing.assert_array_equal(again[k], tabs[k], err_msg=k)


def test_dropin_against_the_method(lc):
    from conftest import load_golden
    from particle_col_image_segmentation_amd import tiff_analysis as ta
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    g = load_golden("func_256_s9")
    ct = {int(k): str(v) for k, v in zip(g["ct_keys"], g["ct_vals"])}
    pipe = FramePipeline(ct)
    res = pipe.run(torch.from_numpy(g["stack"][None]).cuda())
    e = np.linspace(0.0, 5.0, 11)
    want = pipe.neighbourhoods(res, e, window="particle", raster=19.0)
    cell_pos, cell_clusters, _, _ = ta.get_cell_positions_and_areas(g["denoised"], dict(ct))
    got = ta.get_cell_neighbourhoods(g["denoised"], dict(ct), cell_pos, cell_clusters, e, window="particle", px_to_um=SCALE_TABLE)
    names = list(cell_pos) + [n for n in cell_clusters if n not in cell_pos]
    assert names == list(pipe.tables_.slot_names)[:len(names)] and got["neighbourhoods_columns"] == lc.neighbourhood_columns(names, e)
    pick = [want["neighbourhoods_columns"].index(c) for c in got["neighbourhoods_columns"]]  # the slots the frame has
    w, h = want["neighbourhoods"][:, pick], got["neighbourhoods"]
    assert w.shape == h.shape and w.shape[0] > 0 and np.nansum(w[:, 9]) > 0
    w, h = w[np.lexsort((w[:, 4], w[:, 1]))], h[np.lexsort((h[:, 4], h[:, 1]))]  # the drop-in lists strain by strain: by (label, bin)
    np.testing.assert_array_equal(_bits(h), _bits(w))
