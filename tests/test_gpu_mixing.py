"""Random-labelling envelopes of the pair-distance histograms on the device (csrc/mixing.hip) against the numpy restatement
of tests/mixing_reference.py: the labelling rule of include/pcseg.h word for word, the counts by brute force on
point_neighbours' formula.  Everything is compared for exact equality."""
import numpy as np
import pytest

import mixing_reference as mr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CT3 = {1: "3D05", 2: "6B07", 3: "Particle", 4: "C3M10", 5: "Background"}
SCALE_TABLE = 512.0 / 19.0
SIZES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 700]
PERMS = [0, 1, 63, 64, 65, 130]
ENV = tuple(pre + k for pre in ("", "cum_") for k in mr.FIELDS)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")


def _edges(scale):
    # edges that are exact distances of lattice points: pairs land ON them, which pins the [lo, hi) convention
    k = np.array([1, 2, 4, 5, 8, 9, 13, 25, 50, 100.0])
    return np.unique(np.concatenate([[0.0], np.sqrt(k) / scale, [np.sqrt(200.0) / scale * 1.01]]))


def _points(sizes, K, seed):
    """The point sets of test_gpu_neighbours.py -- integer lattices with duplicates and distances exactly on the edges, a
    frame with an absent slot, a slot with one member -- plus a few points of no slot (-1 and K)."""
    rng = np.random.default_rng(seed)
    xy, slot = [], []
    for f, n in enumerate(sizes):
        if f % 2 == 0:
            p = rng.integers(0, 12 if n < 300 else 30, (n, 2)).astype(np.float64)
        else:
            p = rng.uniform(0, 60, (n, 2))
            if n > 4:
                p[1] = p[0]
        s = rng.integers(0, K, n)
        if f % 3 == 1 and K > 1:
            s[s == K - 1] = 0  # an absent slot
        if f % 3 == 2 and K > 1 and n > 3:
            s[s == 0] = 1
            s[0] = 0  # a slot with one member
        if n > 5:
            s[rng.integers(0, n, 3)] = -1
            s[rng.integers(0, n, 2)] = K
        xy.append(p)
        slot.append(s)
    foff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return np.concatenate(xy).astype(np.float64).reshape(-1, 2), np.concatenate(slot).astype(np.int32), foff


def _run(xy, slot, foff, K, scale, edges, P, seed=0, keys=None, counts=True):
    from particle_col_image_segmentation_amd import ops
    dev = torch.device("cuda")
    out = ops.pair_label_mixing(torch.from_numpy(xy).to(dev), torch.from_numpy(slot).to(dev), torch.from_numpy(foff).to(dev), K, scale,
                                edges, P, seed=seed, frame_keys=None if keys is None else torch.tensor(keys, dtype=torch.int64).to(dev),
                                counts=counts)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(got, counts):
    np.testing.assert_array_equal(got["counts"], counts)
    want = mr.envelope(counts)
    assert set(got) == set(ENV) | {"counts"}
    for k in ENV:
        assert got[k].dtype == np.int64
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("scale", [1.0, SCALE_TABLE])
def test_counts_and_envelope_match_the_restatement(K, scale):
    _need_gpu()
    xy, slot, foff = _points(SIZES, K, 300 + K)
    e = _edges(scale)
    keys = list(range(40, 40 + len(SIZES)))
    want = mr.mixing(xy, slot, foff, K, scale, e, max(PERMS), seed=77, keys=keys)  # permutation p does not depend on P
    assert want[:, 0].sum() > 0 and (K == 1 or (want[:, 1:] != want[:, :1]).any())
    for P in PERMS:  # permutation groups: partial, exact, more than one
        _same(_run(xy, slot, foff, K, scale, e, P, seed=77, keys=keys), want[:, :P + 1])


def test_tile_seam():
    """One point more than the kernel's LDS point tile, and two tiles plus one."""
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    T = ops.mixing_tile()
    rng = np.random.default_rng(21)
    sizes = [T + 1, 2 * T + 1]
    xy = rng.integers(0, 40, (sum(sizes), 2)).astype(np.float64)
    slot = rng.integers(0, 2, sum(sizes)).astype(np.int32)
    foff = np.array([0, sizes[0], sum(sizes)], np.int64)
    e = _edges(1.0)
    _same(_run(xy, slot, foff, 2, 1.0, e, 3), mr.mixing(xy, slot, foff, 2, 1.0, e, 3))


@pytest.mark.parametrize("K,m", [(4, 100), (1, 1024), (3, 64)])
def test_bin_chunks(K, m):
    """More (slot pair, bin) rows than one launch's LDS histogram holds: the bins are walked in chunks; 1024 bins; and the
    measured shape (three strains, 64 bins), whose histogram needs more than 64 KB of LDS."""
    _need_gpu()
    rng = np.random.default_rng(23)
    n = 300
    xy = rng.integers(0, 25, (n, 2)).astype(np.float64)
    slot = rng.integers(0, K, n).astype(np.int32)
    foff = np.array([0, 0, n], np.int64)
    e = np.sqrt(np.linspace(0.0, 400.0, m + 1))  # lattice distances on many of the edges
    _same(_run(xy, slot, foff, K, 1.0, e, 5), mr.mixing(xy, slot, foff, K, 1.0, e, 5))


@pytest.mark.parametrize("K", [2, 4])
def test_observed_row_is_point_neighbours_histogram(K):
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    dev = torch.device("cuda")
    xy, slot, foff = _points(SIZES, K, 500 + K)
    e = _edges(SCALE_TABLE)
    m = len(e) - 1
    t = [torch.from_numpy(v).to(dev) for v in (xy, slot, foff)]
    ids = torch.arange(xy.shape[0], dtype=torch.int32, device=dev)
    hist = ops.point_neighbours(t[0], t[1], ids, t[2], K, SCALE_TABLE, e)[2]
    mix = ops.pair_label_mixing(t[0], t[1], t[2], K, SCALE_TABLE, e, 5)
    assert torch.equal(mix["obs"], hist[:, :, 1:m + 1]) and int(mix["obs"].sum()) > 0
    pts = ops.Points(t[0], t[1], ids, t[2])  # a packed point set where point_neighbours' callers have one
    again = ops.pair_label_mixing(pts, None, None, K, SCALE_TABLE, e, 5)
    assert all(torch.equal(again[k], mix[k]) for k in mix)


def test_invariants_on_a_large_frame():
    _need_gpu()
    rng = np.random.default_rng(33)
    n, P = 2000, 70
    xy = np.round(rng.uniform(0, 200, (n, 2)), 1)
    foff = np.array([0, n], np.int64)
    e = np.linspace(0.0, 40.0, 33)
    for K in (3, 1):
        slot = rng.integers(0, K, n).astype(np.int32)
        got = _run(xy, slot, foff, K, 1.0, e, P)
        c = got["counts"]
        assert c[0, 0].sum() > 10000
        # relabelling moves a pair between the slot pairs, never between the bins
        np.testing.assert_array_equal(c.sum(axis=2), np.broadcast_to(c[:, :1].sum(axis=2), (1, P + 1, len(e) - 1)))
        if K == 1:
            np.testing.assert_array_equal(c, np.broadcast_to(c[:, :1], c.shape))
        else:
            assert (c[:, 1:] != c[:, :1]).any()
        for pre in ("", "cum_"):
            assert (got[pre + "lo"] * P <= got[pre + "sum"]).all() and (got[pre + "sum"] <= got[pre + "hi"] * P).all()
            assert (got[pre + "n_le"] + got[pre + "n_ge"] >= P).all()


def test_keys_and_seeds():
    _need_gpu()
    rng = np.random.default_rng(44)
    n, K, P = 200, 3, 20
    one = rng.uniform(0, 50, (n, 2))
    s_one = rng.integers(0, K, n).astype(np.int32)
    other = rng.uniform(0, 50, (6 * 37, 2))
    # the frame at batch positions 0 and 5, among other frames, with the same key
    xy = np.concatenate([one, other[:4 * 37], one, other[4 * 37:]])
    slot = np.concatenate([s_one, rng.integers(0, K, 4 * 37).astype(np.int32), s_one, rng.integers(0, K, 2 * 37).astype(np.int32)])
    foff = np.concatenate([[0], np.cumsum([n, 37, 37, 37, 37, n, 37, 37])]).astype(np.int64)
    e = np.linspace(0.0, 20.0, 11)
    keys = [9, 1, 2, 3, 4, 9, 6, 7]
    got = _run(xy, slot, foff, K, 1.0, e, P, seed=5, keys=keys)
    for k in got:
        np.testing.assert_array_equal(got[k][0], got[k][5], err_msg=k)
    alone = _run(one, s_one, np.array([0, n], np.int64), K, 1.0, e, P, seed=5, keys=[9])
    np.testing.assert_array_equal(alone["counts"][0], got["counts"][0])
    seeded = _run(one, s_one, np.array([0, n], np.int64), K, 1.0, e, P, seed=6, keys=[9])
    keyed = _run(one, s_one, np.array([0, n], np.int64), K, 1.0, e, P, seed=5, keys=[10])
    for o in (seeded, keyed):
        np.testing.assert_array_equal(o["counts"][0, 0], alone["counts"][0, 0])  # the observed labelling has no seed
        assert (o["counts"] != alone["counts"]).any()
    # a seed is a 64-bit number
    big = _run(one, s_one, np.array([0, n], np.int64), K, 1.0, e, P, seed=(1 << 64) - 3, keys=[9])
    np.testing.assert_array_equal(big["counts"], mr.mixing(one, s_one, np.array([0, n]), K, 1.0, e, P, seed=(1 << 64) - 3, keys=[9]))


def _table_from(points, frames, slot, K, e, P, seed):
    """The ``mixing`` table the restatement gives for the rows ``points`` = (frame, x, y) with their slots."""
    foff = np.searchsorted(points[:, 0], np.concatenate([frames, [np.inf]]), side="left").astype(np.int64)
    counts = mr.mixing(points[:, 1:3], slot, foff, K, SCALE_TABLE, e, P, seed=seed, keys=frames.astype(np.int64))
    env = mr.envelope(counts)
    rows = []
    ab = [(a, b) for a in range(K) for b in range(a, K)]
    for f, frame in enumerate(frames):
        for q, (a, b) in enumerate(ab):
            for k in range(len(e) - 1):
                v = lambda name: float(env[name][f, q, k])
                half = lambda c: [v(c + "obs"), v(c + "sum") / P, v(c + "lo"), v(c + "hi"), v(c + "n_le"), v(c + "n_ge")]
                rows.append([frame, a, b, k, e[k], e[k + 1], P] + half("") + half("cum_"))
    return np.array(rows, np.float64)


def _pipeline_reference(pipe, tabs, e, P, seed):
    K = len(pipe.tables_.slot_names)
    frames = tabs["frames"][:, 0]
    cells = tabs["cells"]
    slot = pipe.tables_.slot[cells[:, 2].astype(np.int64)].astype(np.int32)
    slot[slot == 255] = -1
    want = _table_from(np.stack([cells[:, 0], cells[:, 6] + 1.0, cells[:, 5] + 1.0], axis=1), frames, slot, K, e, P, seed)
    rf = tabs["refined"]
    pts = rf[rf[:, 6] >= 1]
    rslot = pipe.tables_.slot[pts[:, 5].astype(np.int64)].astype(np.int32)
    rslot[rslot == 255] = -1
    rwant = _table_from(np.stack([pts[:, 0], pts[:, 10] + 1.0, pts[:, 9] + 1.0], axis=1), frames, rslot, K, e, P, seed)
    return want, rwant


@pytest.mark.parametrize("three", [False, True])
def test_pipeline_mixing_tables(three):
    _need_gpu()
    from particle_col_image_segmentation_amd import synth
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    pipe = FramePipeline(CT3 if three else None)
    stacks = synth.gen_batch(8300 + three, 3, 256, 256)
    res = pipe.run(torch.from_numpy(stacks).cuda())
    e, P, seed = np.linspace(0.0, 8.0, 17), 19, 3
    kw = dict(check=False, neighbours=True, pair_edges=e, refined=True)
    tabs = pipe.tables(res, mixing=P, mixing_seed=seed, **kw)
    plain = pipe.tables(res, **kw)
    new = {"mixing", "refined_mixing"}
    assert set(tabs) == set(plain) | new | {k + "_columns" for k in new}
    for k in plain:
        if not k.endswith("_columns"):
            np.testing.assert_array_equal(tabs[k], plain[k], err_msg=k)
    want, rwant = _pipeline_reference(pipe, tabs, e, P, seed)
    np.testing.assert_array_equal(tabs["mixing"], want)
    np.testing.assert_array_equal(tabs["refined_mixing"], rwant)
    assert tabs["cells"].shape[0] > 20 and tabs["mixing"][:, 7].sum() > 0 and (tabs["mixing"][:, 9] != tabs["mixing"][:, 10]).any()
    # the observed counts are pair_hist's
    K = len(pipe.tables_.slot_names)
    np.testing.assert_array_equal(tabs["mixing"][:, 7].reshape(3, K * (K + 1) // 2, 16), tabs["pair_hist"][:, 4:-1].reshape(3, -1, 16))
    # the same frames as ids 7..9, in another order: per id the same rows
    order, ids = [2, 0, 1], [9, 7, 8]
    res2 = pipe.run(torch.from_numpy(stacks[order]).cuda())
    first = pipe.tables(pipe.run(torch.from_numpy(stacks).cuda()), frame_ids=[7, 8, 9], mixing=P, mixing_seed=seed, **kw)
    second = pipe.tables(res2, frame_ids=ids, mixing=P, mixing_seed=seed, **kw)
    for k in new:
        assert (first[k][:, 1:] != tabs[k][:, 1:]).any()  # other ids, other shuffles
        for fid in (7, 8, 9):
            np.testing.assert_array_equal(first[k][first[k][:, 0] == fid], second[k][second[k][:, 0] == fid], err_msg=k)
    # P = 0 and None switch the tables off
    assert "mixing" not in pipe.tables(res, mixing=0, **kw)
    with pytest.raises(ValueError):
        pipe.tables(res, check=False, mixing=P)


def test_run_sharded_forwards_mixing_tables():
    _need_gpu()
    from particle_col_image_segmentation_amd import synth
    from particle_col_image_segmentation_amd.distributed import run_sharded
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    dev = torch.device("cuda")
    pipe = FramePipeline(CT3)
    stacks = synth.gen_batch(8400, 6, 192, 192)
    make_batch = lambda ids: torch.from_numpy(stacks[list(ids)]).to(dev)
    e = np.linspace(0.0, 6.0, 9)
    kw = dict(check=False, pair_edges=e, mixing=9, mixing_seed=2, refined=True)
    host = run_sharded(6, make_batch, pipe, batch=4, **kw)
    forced = run_sharded(6, make_batch, pipe, batch=4, force_gather=True, device=dev, **kw)
    pipe.synchronize()
    per = [pipe.tables(pipe.run(make_batch(ids)), frame_ids=ids, **kw) for ids in ([0, 1, 2, 3], [4, 5])]
    for k in ("mixing", "refined_mixing"):
        assert host[k].shape == (6 * 6 * 8, 19)
        np.testing.assert_array_equal(host[k], forced[k], err_msg=k)
        np.testing.assert_array_equal(host[k], np.concatenate([p[k] for p in per]), err_msg=k)
    assert "mixing" not in run_sharded(6, make_batch, pipe, batch=4, check=False, pair_edges=e)


def test_dropin_cell_mixing():
    """tiff_analysis.get_cell_mixing on a golden 256 x 256 class map equals the table route for that frame."""
    _need_gpu()
    from conftest import load_golden
    from particle_col_image_segmentation_amd import tiff_analysis as ta
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    g = load_golden("func_256_s9")
    ct = {int(k): str(v) for k, v in zip(g["ct_keys"], g["ct_vals"])}
    pipe = FramePipeline(ct)
    res = pipe.run(torch.from_numpy(g["stack"][None]).cuda())
    np.testing.assert_array_equal(res["denoised"][0].cpu().numpy(), g["denoised"])
    e = np.linspace(0.0, 6.0, 13)
    tabs = pipe.tables(res, pair_edges=e, mixing=29, mixing_seed=4, check=False)
    cell_pos, clusters, _, _ = ta.get_cell_positions_and_areas(g["denoised"], dict(ct))
    regions = {name: list(cell_pos.get(name, [])) + list(clusters.get(name, [])) for name in pipe.tables_.slot_names}
    assert sum(len(v) for v in regions.values()) == tabs["cells"].shape[0] > 20
    cols, rows = ta.get_cell_mixing(regions, e, permutations=29, seed=4, px_to_um=SCALE_TABLE)
    assert cols == tabs["mixing_columns"]
    np.testing.assert_array_equal(rows, tabs["mixing"])
    assert rows[:, 7].sum() > 0 and (rows[:, 9] != rows[:, 10]).any()
