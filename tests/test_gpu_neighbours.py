"""Per-strain nearest neighbours and pair-distance histograms on the device (refine_boundaries.py:8-12, goal 3) against
a chunked numpy brute force on the exact formula: d2 = dx*dx + dy*dy (each product and the sum rounded on their own),
d = sqrt(d2) / scale, minima on d2 with the smallest id on ties, bin k = edges[k] <= d < edges[k + 1]."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CT3 = {1: "3D05", 2: "6B07", 3: "Particle", 4: "C3M10", 5: "Background"}
SCALE_TABLE = 512.0 / 19.0


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")


def brute(xy, slot, ids, foff, K, scale, edges=None, chunk=512):
    n = xy.shape[0]
    dist = np.full((n, K), np.nan)
    nid = np.full((n, K), -1, np.int64)
    P = K * (K + 1) // 2
    pidx = np.full((K, K), -1, np.int64)
    for p, (a, b) in enumerate((a, b) for a in range(K) for b in range(a, K)):
        pidx[a, b] = pidx[b, a] = p
    m = 0 if edges is None else len(edges) - 1
    hist = np.zeros((len(foff) - 1, P, m + 2), np.int64)
    for f in range(len(foff) - 1):
        lo, hi = int(foff[f]), int(foff[f + 1])
        X, Y, S, I = xy[lo:hi, 0], xy[lo:hi, 1], slot[lo:hi], ids[lo:hi].astype(np.int64)
        nf = hi - lo
        for r0 in range(0, nf, chunk):
            r1 = min(nf, r0 + chunk)
            dx = X[r0:r1, None] - X[None, :]
            dy = Y[r0:r1, None] - Y[None, :]
            d2 = dx * dx + dy * dy
            rows = np.arange(r0, r1)
            notself = rows[:, None] != np.arange(nf)[None, :]
            for t in range(K):
                cand = notself & (S == t)[None, :]
                dd = np.where(cand, d2, np.inf)
                best = dd.min(axis=1)
                has = cand.any(axis=1)
                tie = np.where(cand & (dd == best[:, None]), I[None, :], np.iinfo(np.int64).max).min(axis=1)
                ok = has & (S[r0:r1] >= 0) & (S[r0:r1] < K)
                dist[lo + r0:lo + r1, t] = np.where(ok, np.sqrt(best) / scale, np.nan)
                nid[lo + r0:lo + r1, t] = np.where(ok, tie, -1)
            if edges is not None:
                upper = rows[:, None] < np.arange(nf)[None, :]
                d = np.sqrt(d2) / scale
                k = np.searchsorted(edges, d, side="right") - 1  # m = overflow (d >= edges[m])
                p = pidx[S[r0:r1, None], S[None, :]]
                key = (p * (m + 1) + k)[upper]
                c = np.bincount(key, minlength=P * (m + 1)).reshape(P, m + 1)
                hist[f, :, 1:] += c
        for a in range(K):
            for b in range(a, K):
                na, nb = int((S == a).sum()), int((S == b).sum())
                hist[f, pidx[a, b], 0] = na * (na - 1) // 2 if a == b else na * nb
    return dist, nid, hist


def _edges(scale):
    # edges that are exact distances of lattice points: pairs land ON them, which pins the [lo, hi) convention
    k = np.array([1, 2, 4, 5, 8, 9, 13, 25, 50, 100.0])
    return np.unique(np.concatenate([[0.0], np.sqrt(k) / scale, [np.sqrt(200.0) / scale * 1.01]]))


def _points(sizes, K, seed):
    rng = np.random.default_rng(seed)
    xy, slot, ids = [], [], []
    for f, n in enumerate(sizes):
        if f % 2 == 0:  # integer lattice: equidistant ties, duplicates, distances exactly on the edges
            p = rng.integers(0, 12 if n < 300 else 30, (n, 2)).astype(np.float64)
        else:
            p = rng.uniform(0, 60, (n, 2))
            if n > 4:
                p[1] = p[0]  # an exact duplicate: distance 0 to each other
        s = rng.integers(0, K, n)
        if f % 3 == 1 and K > 1:
            s[s == K - 1] = 0  # an absent slot
        if f % 3 == 2 and K > 1 and n > 3:
            s[s == 0] = 1
            s[0] = 0  # a slot with one member
        xy.append(p)
        slot.append(s)
        ids.append(rng.integers(1, 60, n))  # repeated ids: the tie rule picks the smallest
    foff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cat = lambda v, d: np.concatenate(v).astype(d) if v else np.zeros(0, d)
    return cat(xy, np.float64).reshape(-1, 2), cat(slot, np.int32), cat(ids, np.int32), foff


def _run(xy, slot, ids, foff, K, scale, edges):
    from particle_col_image_segmentation_amd import ops
    dev = torch.device("cuda")
    d, i, h = ops.point_neighbours(torch.from_numpy(xy).to(dev), torch.from_numpy(slot).to(dev),
                                   torch.from_numpy(ids).to(dev), torch.from_numpy(foff).to(dev), K, scale, edges)
    torch.cuda.synchronize()
    return d.cpu().numpy(), i.cpu().numpy(), None if h is None else h.cpu().numpy()


@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("scale", [1.0, SCALE_TABLE])
def test_point_neighbours_matches_brute_force(K, scale):
    _need_gpu()
    xy, slot, ids, foff = _points([0, 1, 2, 255, 256, 257, 1000], K, 100 + K)
    e = _edges(scale)
    d, i, h = _run(xy, slot, ids, foff, K, scale, e)
    ed, ei, eh = brute(xy, slot, ids, foff, K, scale, e)
    np.testing.assert_array_equal(d, ed)
    np.testing.assert_array_equal(i, ei)
    np.testing.assert_array_equal(h, eh)
    assert (h[:, :, 1:].sum(axis=2) == h[:, :, 0]).all()
    assert h[:, :, 0].sum() > 0 and (eh[:, :, -1] > 0).any()
    # without edges: the same neighbours, no histogram
    d2, i2, h2 = _run(xy, slot, ids, foff, K, scale, None)
    assert h2 is None
    np.testing.assert_array_equal(d2, ed)
    np.testing.assert_array_equal(i2, ei)


def test_point_neighbours_large_frame_full_histogram():
    """One frame of 20 000 points (many query and candidate tiles, several candidate splits), four slots, 1024 bins."""
    _need_gpu()
    rng = np.random.default_rng(7)
    n, K = 20000, 4
    xy = np.round(rng.uniform(0, 400, (n, 2)), 1)
    slot = rng.integers(0, K, n).astype(np.int32)
    ids = rng.integers(1, 1 << 20, n).astype(np.int32)
    foff = np.array([0, n], np.int64)
    e = np.linspace(0.0, 300.0 / SCALE_TABLE, 1025)
    d, i, h = _run(xy, slot, ids, foff, K, SCALE_TABLE, e)
    ed, ei, eh = brute(xy, slot, ids, foff, K, SCALE_TABLE, e)
    np.testing.assert_array_equal(d, ed)
    np.testing.assert_array_equal(i, ei)
    np.testing.assert_array_equal(h, eh)
    assert (h[:, :, 1:].sum(axis=2) == h[:, :, 0]).all() and h[0, :, -1].sum() > 0


def _synth(seed, B, H=256, W=256):
    from particle_col_image_segmentation_amd import synth
    return synth.gen_batch(seed, B, H, W)


def _check_tables(pipe, tabs, e):
    cells, nb, ph = tabs["cells"], tabs["neighbours"], tabs["pair_hist"]
    K = len(pipe.tables_.slot_names)
    assert nb.shape == (cells.shape[0], 3 + 2 * K) and ph.shape[1] == 4 + len(e)
    np.testing.assert_array_equal(nb[:, :2], cells[:, :2])
    slot = pipe.tables_.slot[cells[:, 2].astype(np.int64)].astype(np.int32)
    np.testing.assert_array_equal(nb[:, 2], slot)
    frames = np.unique(tabs["frames"][:, 0])
    foff = np.searchsorted(cells[:, 0], np.concatenate([frames, [np.inf]]), side="left").astype(np.int64)
    xy = np.stack([cells[:, 6] + 1.0, cells[:, 5] + 1.0], axis=1)
    ed, ei, eh = brute(xy, slot, cells[:, 1].astype(np.int32), foff, K, SCALE_TABLE, e)
    np.testing.assert_array_equal(nb[:, 3:3 + K], ed)
    np.testing.assert_array_equal(nb[:, 3 + K:], ei)
    P = K * (K + 1) // 2
    assert ph.shape[0] == len(frames) * P
    np.testing.assert_array_equal(ph[:, 0], np.repeat(frames, P))
    ab = np.array([(a, b) for a in range(K) for b in range(a, K)], np.float64)
    np.testing.assert_array_equal(ph[:, 1:3], np.tile(ab, (len(frames), 1)))
    np.testing.assert_array_equal(ph[:, 3:], eh.reshape(-1, eh.shape[2]))
    return ed


@pytest.mark.parametrize("three", [False, True])
def test_pipeline_neighbour_tables(three):
    _need_gpu()
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    pipe = FramePipeline(CT3 if three else None)
    stacks = _synth(8100 + three, 4)
    res = pipe.run(torch.from_numpy(stacks).cuda())
    e = np.linspace(0.0, 8.0, 65)
    tabs = pipe.tables(res, distances=True, neighbours=True, pair_edges=e, check=False)
    plain = pipe.tables(res, distances=True, check=False)
    assert set(plain) == {"cells", "rois", "groups", "frames", "distances", "cells_columns", "rois_columns",
                          "groups_columns", "frames_columns", "distances_columns"}
    assert set(tabs) == set(plain) | {"neighbours", "pair_hist", "neighbours_columns", "pair_hist_columns"}
    for k in ("cells", "rois", "groups", "frames", "distances"):
        np.testing.assert_array_equal(tabs[k], plain[k])
    assert tabs["cells"].shape[0] > 20
    _check_tables(pipe, tabs, e)
    if not three:  # two strains: nn_um_<other> is the `distances` value of the same row
        nb, dist = tabs["neighbours"], tabs["distances"]
        assert dist.shape[0] > 0
        got = {(f, l): (nb[r, 4] if s == 0 else nb[r, 3]) for r, (f, l, s) in enumerate(nb[:, :3])}
        other = np.array([got[(f, l)] for f, l, _ in dist])
        # within one ulp, not bit for bit: cell_distance_kernel is compiled to d2 = fma(dx, dx, dy * dy), the neighbour
        # kernel rounds both products (the formula the brute force above restates exactly)
        np.testing.assert_array_max_ulp(other, dist[:, 2], maxulp=1)
        assert (other == dist[:, 2]).mean() > 0.5


def test_run_sharded_forwards_neighbour_tables():
    _need_gpu()
    from particle_col_image_segmentation_amd.distributed import run_sharded
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    dev = torch.device("cuda")
    pipe = FramePipeline(CT3)
    stacks = _synth(8200, 6)
    make_batch = lambda ids: torch.from_numpy(stacks[list(ids)]).to(dev)
    e = np.linspace(0.0, 6.0, 33)
    kw = dict(batch=4, check=False, neighbours=True, pair_edges=e)
    host = run_sharded(6, make_batch, pipe, **kw)
    forced = run_sharded(6, make_batch, pipe, force_gather=True, device=dev, **kw)
    pipe.synchronize()
    for k in ("cells", "neighbours", "pair_hist"):
        np.testing.assert_array_equal(host[k], forced[k])
    per = [pipe.tables(pipe.run(make_batch(ids)), frame_ids=ids, check=False, neighbours=True, pair_edges=e)
           for ids in ([0, 1, 2, 3], [4, 5])]
    for k in ("neighbours", "pair_hist"):
        np.testing.assert_array_equal(host[k], np.concatenate([p[k] for p in per]))
    _check_tables(pipe, host, e)


def test_dropin_cell_neighbour_distances():
    """tiff_analysis.get_cell_neighbour_distances on a reference-style cell_pos dict (strain -> regions)."""
    _need_gpu()
    from types import SimpleNamespace
    from particle_col_image_segmentation_amd import tiff_analysis as ta
    rng = np.random.default_rng(11)
    names, sizes = ["6B07", "3D05", "C3M10"], [40, 1, 25]
    cell_pos, label = {}, 1
    for name, n in zip(names, sizes):
        cell_pos[name] = []
        for _ in range(n):
            cell_pos[name].append(SimpleNamespace(label=label, centroid=tuple(rng.uniform(0, 300, 2))))
            label += 1
    e = np.linspace(0.0, 30.0, 17)
    nn, pairs = ta.get_cell_neighbour_distances(cell_pos, edges=e)
    regs = [(t, r) for t, name in enumerate(names) for r in cell_pos[name]]
    xy = np.array([[r.centroid[1], r.centroid[0]] for _, r in regs])
    slot = np.array([t for t, _ in regs], np.int32)
    ids = np.array([r.label for _, r in regs], np.int32)
    ed, ei, eh = brute(xy, slot, ids, np.array([0, len(regs)], np.int64), 3, ta.PX_TO_UM_CONV, e)
    row = 0
    for t, (name, n) in enumerate(zip(names, sizes)):
        d = nn[name]
        np.testing.assert_array_equal(d["labels"], ids[row:row + n])
        np.testing.assert_array_equal(d["same_um"], ed[row:row + n, t])
        np.testing.assert_array_equal(d["same_label"], ei[row:row + n, t])
        for u, other in enumerate(names):
            if u != t:
                np.testing.assert_array_equal(d["other_um"][other], ed[row:row + n, u])
                np.testing.assert_array_equal(d["other_label"][other], ei[row:row + n, u])
        row += n
    assert np.isnan(nn["3D05"]["same_um"]).all() and (nn["3D05"]["same_label"] == -1).all()
    for p, (a, b) in enumerate((a, b) for a in range(3) for b in range(a, 3)):
        h = pairs[(names[a], names[b])]
        assert h["n_pairs"] == eh[0, p, 0] and h["over"] == eh[0, p, -1]
        np.testing.assert_array_equal(h["bins"], eh[0, p, 1:-1])
