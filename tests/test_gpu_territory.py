"""The nearest-label transform, territories and adjacency on the device (csrc/voronoi.hip) against the brute-force
restatement of tests/test_territory_cpu.py -- every comparison is equality, the um2 columns by their bits --, ``expand_labels``
against scikit-image (tests/golden/territory.npz, off the tie pixels), the ``territories`` / ``adjacency`` tables of the
pipeline, the sharded route and the drop-in helper ``get_cell_territories``."""
import numpy as np
import pytest

from test_territory_cpu import GOLDEN, adjacency_pairs, degrees, nearest_label, territory_table, tie_mask

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SCALE_TABLE = 512.0 / 19.0
NEW = ("territories", "adjacency", "refined_territories", "refined_adjacency")
SHAPES = [(1, 67), (67, 1), (2, 2), (33, 70), (37, 83), (64, 64), (5, 1030), (300, 5), (67, 130)]
CAP = 40


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _contents(H, W, seed):
    """the frames at which the transform can still go wrong, for one shape"""
    rng = np.random.default_rng(seed)
    z = lambda: np.zeros((H, W), np.int32)
    out = [("empty", z())]
    a = z(); a[H // 2, W // 3] = 3
    out.append(("one site", a))
    out.append(("all sites", (1 + (np.arange(H * W).reshape(H, W) * 7) % 5).astype(np.int32)))
    a = z(); a[0, 0], a[0, W - 1], a[H - 1, 0], a[H - 1, W - 1] = 4, 3, 2, 1
    out.append(("corners", a))
    a = z()  # sites on the rows either side of a bit-word seam (and nowhere else)
    for k, r in enumerate(r for r in (31, 32, 33, 63, 64) if r < H):
        a[r, rng.integers(0, W, max(1, W // 16))] = 1 + k
    if not a.any():
        a[H - 1, W - 1] = 1
    out.append(("seams", a))
    a = z()  # single-pixel labels on a lattice of spacing 2: nearly every pixel tied, upper and lower site equally far;
    k = 0    # labels run past CAP (ignored: never a site, never an index)
    for r in range(0, H, 2):
        for c in range(0, W, 2):
            k += 1
            a[r, c] = 1 + (k * 7) % 60
    out.append(("lattice", a))
    a = z()  # one label made of several blobs, two more labels, labels below zero and above CAP in between
    for _ in range(6):
        r, c = rng.integers(0, H), rng.integers(0, W)
        a[max(r - 1, 0):r + 2, max(c - 2, 0):c + 2] = 5
    for l in (1, 2, -3, CAP + 7, 2 ** 31 - 1, -2 ** 31):
        a[rng.integers(0, H), rng.integers(0, W)] = l
    out.append(("blobs", a))
    a = np.where(rng.random((H, W)) < 0.03, rng.integers(1, CAP + 1, (H, W)), 0).astype(np.int32)
    out.append(("sparse", a))
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_nearest_label_shapes_and_contents(shape):
    """every content as one batch of different frames, from an unaligned base pointer; with and without a selection"""
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    H, W = shape
    frames = _contents(H, W, 100 * H + W)
    labs = np.stack([f for _, f in frames])
    B = labs.shape[0]
    buf = torch.empty((B * H * W + 1,), dtype=torch.int32, device="cuda")
    t = buf[1:].view(B, H, W)  # 4 bytes past a 16-byte boundary
    t.copy_(_dev(labs))
    assert t.data_ptr() % 16 == 4
    rng = np.random.default_rng(7)
    sel = rng.random((B, CAP)) < 0.7
    for s in (None, sel):
        d2, near, site = ops.nearest_label(t, None if s is None else torch.from_numpy(s).cuda(), cap=CAP, want_site=True)
        d2, near, site = d2.cpu().numpy(), near.cpu().numpy(), site.cpu().numpy()
        for b, (name, lab) in enumerate(frames):
            want = nearest_label(lab, None if s is None else s[b], CAP)
            for got, w, what in zip((d2[b], near[b], site[b]), want, ("d2", "near", "site")):
                np.testing.assert_array_equal(got, w, err_msg="%s %s %s sel=%s" % (shape, name, what, s is not None))
    assert ops.nearest_label(t, cap=CAP)[2] is None
    # three different frames of the batch alone (B = 3)
    d3 = ops.nearest_label(t[3:6].contiguous(), cap=CAP)
    for b in range(3):
        w = nearest_label(labs[3 + b], None, CAP)
        np.testing.assert_array_equal(d3[0][b].cpu().numpy(), w[0])
        np.testing.assert_array_equal(d3[1][b].cpu().numpy(), w[1])


def test_one_row_per_block_beyond_4094_columns():
    """the row search stages one row per block where four no longer fit 64 KB of LDS"""
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    H, W = 3, 4100
    rng = np.random.default_rng(11)
    lab = np.zeros((2, H, W), np.int32)
    for b in range(2):
        for l in range(1, 13):
            lab[b, rng.integers(0, H), rng.integers(0, W)] = l
    lab[1, 1, 2000:2003], lab[1, 0, 2001], lab[1, 2, 2001] = 0, 9, 4  # upper and lower site equally far
    d2, near, site = ops.nearest_label(_dev(lab), want_site=True)
    for b in range(2):
        for got, w in zip((d2, near, site), nearest_label(lab[b], None, 12)):
            np.testing.assert_array_equal(got[b].cpu().numpy(), w)


def test_default_cap_and_argument_checks():
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    lab = np.zeros((1, 9, 11), np.int32)
    lab[0, 2, 3], lab[0, 7, 8] = 2, 6
    d2, near, _ = ops.nearest_label(_dev(lab))  # cap = the largest label
    w = nearest_label(lab[0])
    np.testing.assert_array_equal(d2[0].cpu().numpy(), w[0])
    np.testing.assert_array_equal(near[0].cpu().numpy(), w[1])
    with pytest.raises(ValueError):
        ops.nearest_label(_dev(lab), sel=torch.ones((2, 6), dtype=torch.uint8).cuda())
    with pytest.raises(TypeError):
        ops.nearest_label(_dev(lab).to(torch.int64))


@pytest.mark.parametrize("shape", [(37, 83), (67, 130), (64, 64)])
def test_territory_reduce_and_pairs(shape):
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    H, W = shape
    frames = _contents(H, W, 100 * H + W)
    labs = np.stack([f for _, f in frames])
    B = labs.shape[0]
    rng = np.random.default_rng(3)
    mask = rng.random((B, H, W)) < 0.4
    slot_of = rng.integers(0, 4, (B, CAP)).astype(np.uint8)  # slot 3: no type (K = 3)
    t = _dev(labs)
    d2, near, _ = ops.nearest_label(t, cap=CAP)
    d2h, nearh = d2.cpu().numpy(), near.cpu().numpy()
    if W % 4 == 0:  # the vector loads also want aligned images: the same inputs 4 bytes past a 16-byte boundary
        aligned = (near, d2)
        near, d2 = (torch.empty((x.numel() + 1,), dtype=torch.int32, device="cuda")[1:].view(x.shape).copy_(x) for x in aligned)
        assert near.data_ptr() % 16 == 4 and d2.data_ptr() % 16 == 4 and near.is_contiguous()
        for m in (None, mask):
            md = None if m is None else torch.from_numpy(m).cuda()
            assert torch.equal(ops.territory_reduce(near, d2, md, 400, CAP), ops.territory_reduce(*aligned, md, 400, CAP))
    for r2 in (0, 1, 400, -1):
        for m in (None, mask):
            got = ops.territory_reduce(near, d2, None if m is None else torch.from_numpy(m).cuda(), r2, CAP).cpu().numpy()
            for b, (name, _) in enumerate(frames):
                want = territory_table(nearh[b], d2h[b], r2, CAP, None if m is None else m[b])
                np.testing.assert_array_equal(got[b], want, err_msg="%s %s r2=%d mask=%s" % (shape, name, r2, m is not None))
        p = ops.territory_pairs(near, d2, r2, pair_cap=4096, slot_of=torch.from_numpy(slot_of).cuda(), n_types=3)
        assert p["n_overflow"] == 0 and not p["overflow"].cpu().numpy().any()
        rows = np.stack([p[k].cpu().numpy() for k in ("frame", "a", "b", "border", "contact")], axis=1)
        deg = p["degree"].cpu().numpy()
        for b, (name, _) in enumerate(frames):
            want = adjacency_pairs(nearh[b], d2h[b], r2)
            np.testing.assert_array_equal(rows[rows[:, 0] == b][:, 1:], want, err_msg="%s %s r2=%d" % (shape, name, r2))
            np.testing.assert_array_equal(deg[b], degrees(want, slot_of[b], 3), err_msg="%s %s r2=%d degree" % (shape, name, r2))
        assert (np.diff(rows[:, 0]) >= 0).all()
    # near outside 1 .. cap is ignored by the reduction, never an index: a smaller cap than the labels in `near`
    small = ops.territory_reduce(near, d2, None, -1, 3).cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(small[b], territory_table(nearh[b], d2h[b], -1, CAP)[:3])
    wild = near.clone()
    wild[:, 0, 0] = -5
    wild[:, H - 1, W - 1] = 2 ** 31 - 1
    got = ops.territory_reduce(wild, d2, None, -1, CAP).cpu().numpy()
    wh = wild.cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(got[b], territory_table(np.where(wh[b] > CAP, 0, wh[b]), d2h[b], -1, CAP))


def test_contact_four_wise_and_diagonal():
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    lab = np.zeros((1, 6, 8), np.int32)
    lab[0, 1:3, 1:3] = 1
    lab[0, 1:3, 3:5] = 2  # abuts 1 four-wise over two rows
    lab[0, 3, 5] = 3      # abuts 2 only diagonally
    d2, near, _ = ops.nearest_label(_dev(lab))
    p = ops.territory_pairs(near, d2, -1)
    got = {(int(a), int(b)): (int(n), int(c)) for a, b, n, c in zip(*(p[k].cpu().tolist() for k in ("a", "b", "border", "contact")))}
    want = adjacency_pairs(*nearest_label(lab[0])[1::-1], -1)
    assert got == {(a, b): (n, c) for a, b, n, c in want.tolist()}
    assert got[(1, 2)][1] == 2 and got[(2, 3)][1] == 0 and got[(2, 3)][0] > 0
    p0 = ops.territory_pairs(near, d2, 0)
    assert [p0[k].cpu().tolist() for k in ("a", "b", "border", "contact")] == [[1], [2], [2], [2]]


def test_pair_table_overflow_is_flagged_and_raised():
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    H, W = 33, 70
    frames = dict(_contents(H, W, 1))
    simple = np.zeros((H, W), np.int32)
    simple[5, 5], simple[20, 40], simple[30, 60] = 1, 2, 3
    labs = np.stack([simple, frames["lattice"], frames["corners"]])
    d2, near, _ = ops.nearest_label(_dev(labs), cap=60)
    d2h, nearh = d2.cpu().numpy(), near.cpu().numpy()
    cap = 2
    assert adjacency_pairs(nearh[1], d2h[1], -1).shape[0] > 8 * cap
    p = ops.territory_pairs(near, d2, -1, pair_cap=8 * cap)
    assert p["overflow"].cpu().tolist() == [0, 1, 0] and p["n_overflow"] == 1
    rows = np.stack([p[k].cpu().numpy() for k in ("frame", "a", "b", "border", "contact")], axis=1)
    assert (rows[:, 0] == 1).sum() == 8 * cap  # a full table, nothing past it
    for b in (0, 2):
        np.testing.assert_array_equal(rows[rows[:, 0] == b][:, 1:], adjacency_pairs(nearh[b], d2h[b], -1))
    live = torch.ones((3, 60), dtype=torch.bool, device="cuda")
    slot_of = torch.zeros((3, 60), dtype=torch.uint8, device="cuda")
    fid = torch.arange(3, dtype=torch.int64, device="cuda")
    args = (_dev(labs), live, slot_of, fid, SCALE_TABLE, 1)
    with pytest.raises(RuntimeError, match="pair table"):
        ops.territory_rows(*args, check=True, pair_cap=8 * cap)
    rows_t, adj, over = ops.territory_rows(*args, check=False, pair_cap=8 * cap)
    assert over.cpu().tolist() == [0, 1, 0]
    ops.territory_rows(*args, check=True)  # 8 x 60 slots hold the lattice


def test_expand_labels_equals_skimage_off_the_ties():
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    g = np.load(GOLDEN)
    for name in (str(n) for n in g["names"]):
        lab = g["lab_" + name].astype(np.int32)
        if name.startswith("ties_"):  # against the brute-force rule only
            d2, near, site = ops.nearest_label(_dev(lab[None]), want_site=True)
            for got, w in zip((d2, near, site), nearest_label(lab)):
                np.testing.assert_array_equal(got[0].cpu().numpy(), w, err_msg=name)
            continue
        off = ~g["tie_" + name]
        np.testing.assert_array_equal(ops.nearest_label(_dev(lab[None]))[0][0].cpu().numpy(), g["d2_" + name])
        for k, dist in enumerate(g["distances"]):
            got = ops.expand_labels(_dev(lab), float(dist)).cpu().numpy()
            assert got.shape == lab.shape
            np.testing.assert_array_equal(got[off], g["exp_%s_%d" % (name, k)][off], err_msg="%s %s" % (name, dist))
        assert not ops.expand_labels(_dev(lab), -1.0).any()
    batch = np.stack([g["lab_discs_64"], g["lab_discs_64"][::-1].copy()]).astype(np.int32)
    got = ops.expand_labels(_dev(batch), 2.5).cpu().numpy()
    np.testing.assert_array_equal(got[0], ops.expand_labels(_dev(batch[0]), 2.5).cpu().numpy())


# ------------------------------------------------------------------ tables
def _expected_tables(t_rows, lab_images, masks, r2, K):
    """the territory / adjacency rows the restatement gives for the (frame position, label, slot) keys of a table"""
    terr, adj = [], []
    for f in sorted(set(int(v) for v in t_rows[:, 0])):
        keys = t_rows[t_rows[:, 0] == f]
        labels = keys[:, 1].astype(np.int64)
        cap = int(labels.max())
        sel = np.zeros(cap, bool)
        sel[labels - 1] = True
        slot_of = np.full(cap, 255, np.int64)
        slot_of[labels - 1] = np.where(keys[:, 2] < 0, 255, keys[:, 2]).astype(np.int64)
        d2, near, _ = nearest_label(lab_images[f], sel, cap)
        tab = territory_table(near, d2, r2, cap, masks[f])
        pairs = adjacency_pairs(near, d2, r2)
        deg = degrees(pairs, slot_of, K)
        s2 = np.float64(SCALE_TABLE * SCALE_TABLE)
        for l in labels:
            row = tab[l - 1].astype(np.float64)
            terr.append(list(row) + list(deg[l - 1].astype(np.float64)) + [row[0] / s2, row[1] / s2])
        slot = lambda l: float(slot_of[l - 1]) if slot_of[l - 1] < 4 else -1.0
        adj += [[float(f), a, b, slot(a), slot(b), n, c] for a, b, n, c in pairs.tolist()]
    return np.array(terr, np.float64).reshape(len(terr), -1), np.array(adj, np.float64).reshape(-1, 7)


@pytest.mark.parametrize("reach", [None, 0.3])
def test_pipeline_territory_tables(reach):
    _need_gpu()
    from particle_col_image_segmentation_amd import ops, synth
    from particle_col_image_segmentation_amd.distributed import run_sharded
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    pipe = FramePipeline(dict(synth.CELL_TYPES_5))
    host_stacks = synth.gen_batch(9, 2, 128, 128)
    stacks = torch.from_numpy(host_stacks).cuda()
    res = pipe.run(stacks)
    every = dict(neighbours=True, pair_edges=np.linspace(0.0, 5.0, 6), refined=True, surface=True, surface_edges=np.linspace(0.0, 4.0, 9),
                 distances=True, shape=True, convex=True, check=False)
    tabs = pipe.tables(res, territory=True, territory_reach=reach, **every)
    plain = pipe.tables(res, **every)
    assert set(tabs) == set(plain) | set(NEW) | {k + "_columns" for k in NEW}
    for k in plain:  # every table that existed before: equal with and without the new keywords
        np.testing.assert_array_equal(tabs[k], plain[k], err_msg=k)
    K = len(pipe.tables_.slot_names)
    cols = pipe.table_columns(5, territory=True, territory_reach=reach, **{k: v for k, v in every.items() if k not in ("distances", "check")})
    empty = pipe.empty_device_tables(5, device="cuda", territory=True, territory_reach=reach,
                                     **{k: v for k, v in every.items() if k not in ("distances", "check")})
    for k in NEW:
        assert tabs[k + "_columns"] == cols[k] and tabs[k].shape[1] == len(cols[k]) == empty[k].shape[1], k
    cells, refined = tabs["cells"], tabs["refined"]
    rk = refined[refined[:, 6] >= 1]
    assert cells.shape[0] > 3 and rk.shape[0] > 3
    np.testing.assert_array_equal(tabs["territories"][:, :3], tabs["convexity"][:, :3])
    np.testing.assert_array_equal(tabs["territories"][:, :2], cells[:, :2])
    np.testing.assert_array_equal(tabs["refined_territories"][:, :3], tabs["refined_neighbours"][:, :3])
    np.testing.assert_array_equal(tabs["refined_territories"][:, :2], rk[:, :2])
    r2 = ops.reach_um_r2(reach, SCALE_TABLE)
    masks = ops.particle_mask(res["recreated"], pipe.tables_.particle_value).cpu().numpy()
    for name, adj_name, key in (("territories", "adjacency", "labels"), ("refined_territories", "refined_adjacency", "ws_labels")):
        t, a = tabs[name], tabs[adj_name]
        want_t, want_a = _expected_tables(t, res[key].cpu().numpy(), masks, r2, K)
        np.testing.assert_array_equal(_bits(t[:, 3:]), _bits(want_t), err_msg=name)
        np.testing.assert_array_equal(a, want_a, err_msg=adj_name)
        assert a.shape[0] > 0
    if reach is None:
        assert tabs["territories"][:, 3].sum() == 2 * 128 * 128  # unbounded territories tile the frames
    # the sharded route with one rank: the same tables, the same schema
    make_batch = lambda ids: torch.from_numpy(host_stacks[list(ids)]).cuda()
    kw = dict(batch=2, check=False, territory=True, territory_reach=reach, refined=True)
    host = run_sharded(2, make_batch, pipe, **kw)
    forced = run_sharded(2, make_batch, pipe, force_gather=True, device=torch.device("cuda"), **kw)
    pipe.synchronize()
    for k in NEW:
        np.testing.assert_array_equal(host[k], tabs[k], err_msg=k)
        np.testing.assert_array_equal(forced[k], tabs[k], err_msg=k)
        assert host[k + "_columns"] == cols[k]
    assert not set(run_sharded(2, make_batch, pipe, batch=2, check=False)) & set(NEW)
    only = pipe.tables(res, territory=True, territory_reach=reach, check=False)
    assert set(only) - set(pipe.tables(res, check=False)) == {"territories", "adjacency", "territories_columns", "adjacency_columns"}
    np.testing.assert_array_equal(only["territories"], tabs["territories"])
    pipe.synchronize()


def test_get_cell_territories_equals_the_table_rows():
    _need_gpu()
    from particle_col_image_segmentation_amd import synth
    from particle_col_image_segmentation_amd import tiff_analysis as ta
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    ct = dict(synth.CELL_TYPES_5)
    pipe = FramePipeline(ct)
    res = pipe.run(torch.from_numpy(synth.gen_batch(9, 1, 128, 128)).cuda())
    for reach in (None, 0.3):
        tabs = pipe.tables(res, territory=True, territory_reach=reach, check=False)
        z = res["denoised"][0].cpu().numpy()
        cell_pos, cell_clusters, _, _ = ta.get_cell_positions_and_areas(z, dict(ct))
        got = ta.get_cell_territories(z, cell_pos, cell_clusters, dict(ct), reach=reach, px_to_um=SCALE_TABLE)
        # the drop-in's slots count its strains in ITS order: map them onto the table's type slots by name
        to_table = {float(k): float(pipe.tables_.slot_names.index(n)) for k, n in enumerate(got["names"])}
        to_table[-1.0] = -1.0
        K, names = len(got["names"]), pipe.tables_.slot_names
        assert sorted(got["names"]) == sorted(names)
        t, want = got["territories"].copy(), tabs["territories"][:, 1:]
        t[:, 1] = [to_table[v] for v in t[:, 1]]
        order = [got["names"].index(n) for n in names]
        t[:, 6:6 + K] = got["territories"][:, 6:6 + K][:, order]
        t[:, 6 + K:6 + 2 * K] = got["territories"][:, 6 + K:6 + 2 * K][:, order]
        np.testing.assert_array_equal(_bits(t), _bits(want))
        a = got["adjacency"].copy()
        a[:, 2] = [to_table[v] for v in a[:, 2]]
        a[:, 3] = [to_table[v] for v in a[:, 3]]
        np.testing.assert_array_equal(a, tabs["adjacency"][:, 1:])
        assert got["territories_columns"][0] == "label" and len(got["territories_columns"]) == t.shape[1]
    pipe.synchronize()
