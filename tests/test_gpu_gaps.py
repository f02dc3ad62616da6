"""Edge-to-edge gaps on the device (csrc/gaps.hip, gaps.py) against the brute-force restatements of tests/gaps_reference.py:
the nearest OTHER label on the shapes and contents at which the two-candidate column pass and the row search can go wrong,
the gap table, its independence of what outputs and workspace held before, ``FramePipeline.gaps`` and the drop-in helper
``get_cell_gaps``.  Every comparison is equality, the um columns by their bits."""
import numpy as np
import pytest

import gaps_reference as gr
import output_cases as oc
from test_gaps_cpu import CAP, contents, hand_made

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SCALE_TABLE = 512.0 / 19.0
# tests/test_gpu_territory.py's: the 32-row seams, the 64- and 256-column block edges, the 1024-column trip, degenerate frames
SHAPES = [(1, 67), (67, 1), (2, 2), (33, 70), (37, 83), (64, 64), (5, 1030), (300, 5), (67, 130)]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _unaligned(labs):
    B, H, W = labs.shape
    buf = torch.empty((B * H * W + 1,), dtype=torch.int32, device="cuda")
    t = buf[1:].view(B, H, W)  # 4 bytes past a 16-byte boundary
    t.copy_(_dev(labs))
    assert t.data_ptr() % 16 == 4
    return t


@pytest.mark.parametrize("shape", SHAPES)
def test_nearest_other_label_shapes_and_contents(shape):
    """every content as one batch of different frames, from an unaligned base pointer; with and without a selection"""
    _need_gpu()
    from particle_col_image_segmentation_amd import gaps
    H, W = shape
    frames = list(contents(H, W, 100 * H + W).items())
    labs = np.stack([f for _, f in frames])
    B = labs.shape[0]
    t = _unaligned(labs)
    sel = np.random.default_rng(7).random((B, CAP)) < 0.7
    for s in (None, sel):
        d2, near = gaps.nearest_other_label(t, None if s is None else torch.from_numpy(s).cuda(), cap=CAP)
        d2, near = d2.cpu().numpy(), near.cpu().numpy()
        for b, (name, lab) in enumerate(frames):
            want = gr.nearest_other_label(lab, None if s is None else s[b], CAP)
            for got, w, what in zip((d2[b], near[b]), want, ("d2", "near")):
                np.testing.assert_array_equal(got, w, err_msg="%s %s %s sel=%s" % (shape, name, what, s is not None))
    # three different frames of the batch alone (B = 3)
    d3 = gaps.nearest_other_label(t[3:6].contiguous(), cap=CAP)
    for b in range(3):
        w = gr.nearest_other_label(labs[3 + b], None, CAP)
        np.testing.assert_array_equal(d3[0][b].cpu().numpy(), w[0])
        np.testing.assert_array_equal(d3[1][b].cpu().numpy(), w[1])


@pytest.mark.parametrize("density", [0.1, 0.4, 0.9, 1.0])
def test_random_small_frames(density):
    _need_gpu()
    from particle_col_image_segmentation_amd import gaps
    rng = np.random.default_rng(int(10 * density))
    labs = np.where(rng.random((256, 9, 11)) < density, rng.integers(1, 5, (256, 9, 11)), 0).astype(np.int32)
    sel = rng.random((256, 4)) < 0.7
    d2, near = (v.cpu().numpy() for v in gaps.nearest_other_label(_dev(labs), torch.from_numpy(sel).cuda()))
    for b in range(256):
        w = gr.nearest_other_label(labs[b], sel[b], 4)
        np.testing.assert_array_equal(d2[b], w[0], err_msg="frame %d" % b)
        np.testing.assert_array_equal(near[b], w[1], err_msg="frame %d" % b)


@pytest.mark.parametrize("W", [2046, 2047, 8200])
def test_rows_per_block_by_width(W):
    """four rows per block up to 2046 columns, one beyond, and a stage above 64 KB beyond 8190"""
    _need_gpu()
    from particle_col_image_segmentation_amd import gaps
    H = 6
    rng = np.random.default_rng(W)
    lab = np.zeros((2, H, W), np.int32)
    for b in range(2):
        for l in range(1, 13):
            lab[b, rng.integers(0, H), rng.integers(0, W)] = l
        lab[b, 2, 5:40] = 3
    lab[1, 1, 1000:1003], lab[1, 0, 1001], lab[1, 2, 1001], lab[1, 1, 1001] = 0, 9, 4, 9  # upper and lower site equally far
    d2, near = gaps.nearest_other_label(_dev(lab))
    for b in range(2):
        w = gr.nearest_other_label(lab[b], None, 12)
        np.testing.assert_array_equal(d2[b].cpu().numpy(), w[0])
        np.testing.assert_array_equal(near[b].cpu().numpy(), w[1])


def test_reach_at_below_and_above_the_true_distances():
    _need_gpu()
    from particle_col_image_segmentation_amd import gaps
    frames = contents(37, 83, 3)
    labs = np.stack([frames[k] for k in ("two labels", "ring", "sparse", "runs", "one label")])
    t = _dev(labs)
    true = [gr.nearest_other_label(lab, None, CAP) for lab in labs]
    seen = sorted(set(int(v) for d, _ in true for v in d[d > 0]))
    for r2 in sorted(set([0, 1, 2] + [seen[len(seen) // 2] + k for k in (-1, 0, 1)] + [seen[-1] + k for k in (-1, 0, 1)])):
        d2, near = (v.cpu().numpy() for v in gaps.nearest_other_label(t, cap=CAP, r2=r2))
        for b, (d, n) in enumerate(true):
            inside = (d >= 0) & (d <= r2)  # a site at exactly r2 counts
            np.testing.assert_array_equal(d2[b], np.where(inside, d, -1), err_msg="r2 = %d" % r2)
            np.testing.assert_array_equal(near[b], np.where(inside, n, 0), err_msg="r2 = %d" % r2)
            w = gr.nearest_other_label(labs[b], None, CAP, r2)
            np.testing.assert_array_equal(d2[b], w[0])
    d2, near = gaps.nearest_other_label(t, cap=CAP, r2=1 << 40)  # above every int32: unbounded
    np.testing.assert_array_equal(d2.cpu().numpy(), np.stack([d for d, _ in true]))


def _table_case(seed, H, W, cap):
    """labels 1 .. cap in blobs (some in several, some touching), labels that are not live, slots 0 .. 4"""
    rng = np.random.default_rng(seed)
    lab = np.zeros((H, W), np.int32)
    for l in list(range(1, cap - 1)) * 2:  # (cap - 1 and cap keep no pixel ... mostly)
        r, c = rng.integers(0, H), rng.integers(0, W)
        lab[max(r - rng.integers(0, 3), 0):r + rng.integers(1, 4), max(c - rng.integers(0, 4), 0):c + rng.integers(1, 5)] = l
    lab[rng.integers(0, H), rng.integers(0, W)] = cap + 3   # above cap
    lab[rng.integers(0, H), rng.integers(0, W)] = -2
    live = rng.random(cap) < 0.8
    slot_of = rng.integers(0, 5, cap).astype(np.uint8)      # with K < 5: slots without a type
    slot_of[slot_of == 1] = 0                                # slot 1 has no label at all
    return lab, live, slot_of


@pytest.mark.parametrize("K", [1, 2, 4])
def test_label_gaps_against_the_brute_force(K):
    _need_gpu()
    from particle_col_image_segmentation_amd import gaps
    cap = 14
    cases = [_table_case(s, H, W, cap) for s, (H, W) in enumerate([(33, 70), (33, 70), (33, 70)])]
    hm = hand_made()
    pad = np.zeros((33, 70), np.int32)
    pad[:7, :12] = hm[0]
    cases.append((pad, np.r_[hm[1], np.zeros(cap - 6, bool)], np.r_[hm[2], np.full(cap - 6, 9, np.uint8)]))
    labs, live, slot_of = (np.stack([c[k] for c in cases]) for k in range(3))
    args = (_unaligned(labs), torch.from_numpy(live).cuda(), _dev(slot_of, np.uint8), K)
    for r2 in (-1, 10):
        gap2, partner = gaps.label_gaps(*args, r2=r2)
        again = gaps.label_gaps(*args, r2=r2)
        assert torch.equal(gap2, again[0]) and torch.equal(partner, again[1])  # bit-identical when called twice
        gap2, partner = gap2.cpu().numpy(), partner.cpu().numpy()
        assert gap2.dtype == np.int32 and gap2.shape == (4, cap, K)
        n_sym = 0
        for b in range(4):
            for table in (gr.label_gaps, gr.label_gaps_by_transform):
                w = table(labs[b], live[b], slot_of[b], K, r2)
                np.testing.assert_array_equal(gap2[b], w[0], err_msg="frame %d K %d r2 %d" % (b, K, r2))
                np.testing.assert_array_equal(partner[b], w[1], err_msg="frame %d K %d r2 %d" % (b, K, r2))
            assert (gap2[b][~live[b]] == -1).all() and (partner[b][~live[b]] == 0).all()
            n_sym += gr.check_symmetry(gap2[b], partner[b], live[b], slot_of[b], K)
        assert n_sym > 0
        if K >= 2:
            assert (gap2[:3, :, 1] == -1).all()  # a slot without any label (the random frames)


def test_label_gaps_many_labels_past_the_slot_table():
    """more labels in a block than its 256 LDS slots, and labels that collide in them"""
    _need_gpu()
    from particle_col_image_segmentation_amd import gaps
    H, W, cap = 40, 300, 700
    lab = np.zeros((1, H, W), np.int32)
    k = 0
    for r in range(0, H, 3):
        for c in range(0, W, 3):
            k += 1
            lab[0, r:r + 2, c] = 1 + (k * 257) % cap
    live = np.ones((1, cap), bool)
    slot_of = (np.arange(cap) % 2).astype(np.uint8)[None]
    gap2, partner = gaps.label_gaps(_dev(lab), torch.from_numpy(live).cuda(), _dev(slot_of, np.uint8), 2)
    w = gr.label_gaps_by_transform(lab[0], live[0], slot_of[0], 2)
    np.testing.assert_array_equal(gap2[0].cpu().numpy(), w[0])
    np.testing.assert_array_equal(partner[0].cpu().numpy(), w[1])


def test_results_do_not_depend_on_prior_contents(monkeypatch):
    """outputs and workspace starting as zeros, as every byte 0xFF and as every element 1: identical results, no byte written
    outside them, and the rows of labels that are not live read -1 / 0"""
    _need_gpu()
    from device_helpers import OutputHooks
    from particle_col_image_segmentation_amd import gaps, ops
    hooks = OutputHooks([ops, gaps], monkeypatch)  # (the workspace is ops._ws's torch.empty: padded and filled like the outputs)
    lab, live, slot_of = _table_case(5, 37, 83, 14)
    labs, lives, slots = _dev(lab[None]), torch.from_numpy(live[None]).cuda(), _dev(slot_of[None], np.uint8)
    results = []
    for state in oc.OUTPUT_STATES:
        hooks.begin(state)
        out = gaps.nearest_other_label(labs, lives, r2=200) + gaps.label_gaps(labs, lives, slots, 4)
        assert not hooks.finish(), hooks.finish()
        assert {h.wrapper for h in hooks.handed} >= {"nearest_other_label", "label_gaps", "_ws"}
        results.append([v.cpu().numpy().copy() for v in out])
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert a.tobytes() == b.tobytes()
    d2, near, gap2, partner = results[0]
    w = gr.nearest_other_label(lab, live, 14, 200)
    np.testing.assert_array_equal(d2[0], w[0])
    np.testing.assert_array_equal(near[0], w[1])
    assert (~live).any() and (gap2[0][~live] == -1).all() and (partner[0][~live] == 0).all()
    np.testing.assert_array_equal(gap2[0], gr.label_gaps(lab, live, slot_of, 4)[0])


# ------------------------------------------------------------------ the pipeline
@pytest.mark.parametrize("of", ["cells", "refined"])
def test_pipeline_gaps(of):
    _need_gpu()
    from particle_col_image_segmentation_amd import gaps, ops, synth
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    pipe = FramePipeline(dict(synth.CELL_TYPES_5))
    res = pipe.run(torch.from_numpy(synth.gen_batch(9, 2, 128, 128)).cuda())
    pipe.synchronize()
    before = {k: v.cpu().numpy().tobytes() for k, v in res.items() if isinstance(v, torch.Tensor)}
    fid = [11, 5]
    got = pipe.gaps(res, of=of, frame_ids=fid)
    names = list(pipe.tables_.slot_names)
    K = len(names)
    assert got["gaps_columns"] == gaps.gap_columns(names) and got["gaps"].shape[1] == 3 + 3 * K and got["gaps"].dtype == np.float64
    tabs = pipe.tables(res, frame_ids=fid, neighbours=True, refined=True, territory=True, check=False)
    prefix = "" if of == "cells" else "refined_"
    np.testing.assert_array_equal(got["gaps"][:, :3], tabs[prefix + "neighbours"][:, :3])  # rows, order and slots
    # the restatement on the downloaded labels, live rows and slots
    if of == "cells":
        rows = ops.class_rows(res)
    else:
        pos = torch.arange(2, dtype=torch.int64, device="cuda")
        _, d = ops._dense_tables(res, res.get("groups") or {}, pos, 5, (), True)
        rt = ops.refined_tables(res, pos, pipe.tables_, d.ws, (d.n_roi, d.n_cell), check=True)
        rows = ops.refined_rows(res, rt["kind_r"], rt["slot_r"])
    labs, live, slot_of = rows.labels.cpu().numpy(), rows.live.cpu().numpy().astype(bool), rows.slot_of.cpu().numpy()
    want = gr.gap_rows(fid, labs, live, slot_of, K, SCALE_TABLE, table=gr.label_gaps_by_transform)
    assert want.shape[0] > 3
    np.testing.assert_array_equal(_bits(got["gaps"]), _bits(want))
    # touching along an edge, as the territories table counts it
    terr, cols = tabs[prefix + "territories"], tabs[prefix + "territories_columns"]
    np.testing.assert_array_equal(terr[:, :3], got["gaps"][:, :3])
    px2 = got["gaps"][:, 3 + 2 * K:]
    for t, n in enumerate(names):
        np.testing.assert_array_equal(px2[:, t] == 1, terr[:, cols.index("n_contact_%s" % n)] > 0, err_msg=n)
    if of == "cells":  # 8-connected components of one class never come closer than two pixels
        own = got["gaps"][:, 2].astype(int)
        same = px2[np.arange(len(own))[own >= 0], own[own >= 0]]
        assert ((same == -1) | (same >= 4)).all()
    else:
        assert (px2 == 1).any()  # ROIs flooded against each other
    # a reach turns the gaps beyond it into NaN / -1 and changes nothing else
    finite = np.sort(got["gaps"][:, 3:3 + K][np.isfinite(got["gaps"][:, 3:3 + K])])
    reach = float(finite[len(finite) // 2])  # a gap of exactly the reach is beyond it
    near = pipe.gaps(res, of=of, reach=reach, frame_ids=fid)["gaps"]
    keep = got["gaps"][:, 3:3 + K] < reach
    assert keep.any() and (~keep & np.isfinite(got["gaps"][:, 3:3 + K])).any()
    masked = got["gaps"].copy()
    masked[:, 3:3 + K][~keep], masked[:, 3 + K:3 + 2 * K][~keep], masked[:, 3 + 2 * K:][~keep] = np.nan, -1.0, -1.0
    np.testing.assert_array_equal(_bits(near), _bits(masked))
    pipe.synchronize()
    after = {k: v.cpu().numpy().tobytes() for k, v in res.items() if isinstance(v, torch.Tensor)}
    assert len(before) > 5 and set(after) == set(before) and all(after[k] == v for k, v in before.items())  # res is only read


def test_get_cell_gaps_equals_the_reference():
    _need_gpu()
    from particle_col_image_segmentation_amd import synth
    from particle_col_image_segmentation_amd import tiff_analysis as ta
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    ct = dict(synth.CELL_TYPES_5)
    pipe = FramePipeline(ct)
    res = pipe.run(torch.from_numpy(synth.gen_batch(9, 1, 128, 128)).cuda())
    z = res["denoised"][0].cpu().numpy()
    pipe.synchronize()
    cell_pos, cell_clusters, _, _ = ta.get_cell_positions_and_areas(z, dict(ct))
    for reach in (None, 0.3):
        got = ta.get_cell_gaps(cell_pos, cell_clusters, reach=reach, px_to_um=SCALE_TABLE)
        names = got["names"]
        K = len(names)
        assert got["gaps_columns"][:2] == ["label", "slot"] and len(got["gaps_columns"]) == got["gaps"].shape[1] == 2 + 3 * K
        regs = [(t, r) for t, n in enumerate(names) for r in list(cell_pos.get(n, [])) + list(cell_clusters.get(n, []))]
        lab = regs[0][1]._im.dev.cpu().numpy()
        cap = max(r.label for _, r in regs)
        live, slot_of = np.zeros(cap, bool), np.full(cap, 255, np.uint8)
        for t, r in regs:
            live[r.label - 1], slot_of[r.label - 1] = True, t
        from particle_col_image_segmentation_amd import ops
        r2 = ops.reach_um_r2(reach, SCALE_TABLE)
        want = gr.gap_rows([0], [lab], [live], [slot_of], K, SCALE_TABLE, r2=r2, table=gr.label_gaps_by_transform)
        assert want.shape[0] == len(regs) > 3
        np.testing.assert_array_equal(_bits(got["gaps"]), _bits(want[:, 1:]))
    assert ta.get_cell_gaps({}, {})["gaps"].shape == (0, 2)
