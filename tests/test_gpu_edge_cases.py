"""Degenerate inputs (the edge cases the reference's libraries define): tiny frames, empty / full masks, no markers,
constant images, single-pixel objects -- every kernel against the oracle."""
import numpy as np
import pytest

from oracle import oracle as orc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == bool:
        a = a.astype(np.uint8)
    return torch.from_numpy(a).cuda()


SHAPES = [(1, 1), (1, 7), (6, 1), (2, 3), (5, 70), (33, 2), (64, 64), (65, 63)]


@pytest.mark.parametrize("shape", SHAPES)
def test_tiny_and_degenerate(shape):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    from particle_col_image_segmentation_amd import ops
    H, W = shape
    rng = np.random.default_rng(H * 100 + W)
    variants = {
        "zeros": np.zeros(shape, np.uint8),
        "ones": np.ones(shape, np.uint8),
        "rand": (rng.random(shape) < 0.5).astype(np.uint8),
        "classes": rng.integers(0, 4, shape).astype(np.uint8),
    }
    for name, a in variants.items():
        x = _dev(a)[None]
        np.testing.assert_array_equal(ops.median5(x)[0].cpu().numpy(), orc.median_filter(a), err_msg=name)
        lab, cnt = ops.label_equal8(x)
        exp, n = orc.label(a, return_num=True)
        np.testing.assert_array_equal(lab[0].cpu().numpy(), exp, err_msg=name)
        assert int(cnt[0]) == n
        lab4, cnt4 = ops.label_bool4(x)
        exp4, n4 = orc.label(a > 0, connectivity=1, return_num=True)
        np.testing.assert_array_equal(lab4[0].cpu().numpy(), exp4, err_msg=name)
        m = a > 0
        np.testing.assert_array_equal(ops.edt_sq(_dev(m)[None])[0].cpu().numpy(), orc.edt_sq(m), err_msg=name)
        np.testing.assert_array_equal(ops.fill_holes(_dev(m)[None])[0].cpu().numpy().astype(bool),
                                      orc.binary_fill_holes(m), err_msg=name)
        np.testing.assert_array_equal(ops.dilate_disk(x, 1 << 1, 2)[0].cpu().numpy().astype(bool),
                                      orc.binary_dilation_disk(a == 1, 2), err_msg=name)
        np.testing.assert_array_equal(ops.dilated_roots(x, 1 << 1, 2)[0].cpu().numpy() >= 0,
                                      orc.binary_dilation_disk(a == 1, 2), err_msg=name)
        d2 = orc.edt_sq(m)
        is_max, markers, nm = ops.local_maxima(_dev(d2)[None])
        lm = orc.local_maxima(d2)
        np.testing.assert_array_equal(is_max[0].cpu().numpy().astype(bool), lm, err_msg=name)
        np.testing.assert_array_equal(markers[0].cpu().numpy(), orc.label(lm), err_msg=name)
        # watershed on the class image as "elevation": with markers from the maxima, with no marker at all, no mask
        img = rng.random(shape).astype(np.float32)
        for mk, ms in ((orc.label(lm), m), (np.zeros(shape, np.int32), m), (orc.label(lm), np.zeros(shape, bool))):
            for mode in (0, 1):
                out, _ = ops.watershed(_dev(img)[None], _dev(mk.astype(np.int32))[None], _dev(ms)[None], mode=mode)
                np.testing.assert_array_equal(out[0].cpu().numpy(), orc.watershed(img, mk, ms), err_msg=name)
        out, area = ops.fill_particle(x, 2, 1, 2, 20, 2)
        exp, ov = orc.fill_particle_area(a, 2, 1, 2)
        np.testing.assert_array_equal(out[0].cpu().numpy(), exp, err_msg=name)
        assert int(area[0]) == ov
        if n:
            stats, _, _, _ = ops.region_reduce(lab, cnt, cap=n)
            np.testing.assert_array_equal(stats[0, :n].cpu().numpy(), orc.region_table(exp_lab := orc.label(a)), err_msg=name)


def test_pipeline_on_empty_and_uniform_frames():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    from particle_col_image_segmentation_amd import synth
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    ct = dict(synth.CELL_TYPES_5)
    H = W = 48
    st = np.full((3, 5, H, W), 0.1, np.float32)
    st[0, 4] = 0.6                      # all background: no cells, no particle, boundary plane constant
    st[1, 2] = 0.6                      # all particle
    st[2, 3] = 0.9                      # all boundary: the refine mask is empty
    res = FramePipeline(ct).run(torch.from_numpy(st).cuda())
    res.check()
    for b in range(3):
        ref = orc.segment_frame(st[b], ct)
        np.testing.assert_array_equal(res["labels"][b].cpu().numpy(), ref["label_im"])
        np.testing.assert_array_equal(res["ws_labels"][b].cpu().numpy(), ref["refine"]["labels"])
        np.testing.assert_array_equal(res["recreated"][b].cpu().numpy(), ref["recreated"])
        assert int(res["particle_area"][b]) == ref["particle_area"]
    tabs = FramePipeline(ct).tables(res)
    assert tabs["cells"].shape[0] == 0


def test_watershed_long_winding_path_finishes_in_the_tail_kernel():
    """The minimax relaxation enqueues a fixed number of grid rounds and leaves the rest to a per-frame tail kernel
    (no host polling).  A serpentine corridor whose only marker sits at one end needs one round per tile crossing --
    far more than the grid rounds -- so this result comes out of the tail kernel; a second frame of plain noise rides in
    the same launch."""
    import torch
    from particle_col_image_segmentation_amd import ops
    H, W = 448, 448
    rng = np.random.default_rng(7)
    mask = np.zeros((H, W), bool)
    img = np.full((H, W), 0.9, np.float32)
    # corridor: horizontal runs every 8 rows joined alternately at the right / left end
    rows = list(range(4, H - 4, 8))
    order = []
    for k, r in enumerate(rows):
        cols = range(4, W - 4) if k % 2 == 0 else range(W - 5, 3, -1)
        order += [(r, c) for c in cols]
        if k + 1 < len(rows):
            cend = W - 5 if k % 2 == 0 else 4
            order += [(rr, cend) for rr in range(r + 1, rows[k + 1])]
    for i, (r, c) in enumerate(order):
        mask[r, c] = True
        img[r, c] = 0.05 + 0.4 * i / len(order)  # strictly increasing along the corridor: tie-free
    markers = np.zeros((H, W), np.int32)
    markers[order[0]] = 1
    markers[order[len(order) // 2]] = 2
    img2 = rng.random((H, W)).astype(np.float32)
    mask2 = img2 < 0.8
    mk2 = np.zeros((H, W), np.int32)
    for k in range(1, 40):
        r, c = rng.integers(0, H), rng.integers(0, W)
        if mask2[r, c]:
            mk2[r, c] = k
    imgs = np.stack([img, img2])
    out, flags = ops.watershed(torch.from_numpy(imgs).cuda(), torch.from_numpy(np.stack([markers, mk2])).cuda(),
                               torch.from_numpy(np.stack([mask, mask2]).astype(np.uint8)).cuda())
    np.testing.assert_array_equal(out[0].cpu().numpy(), orc.watershed(img, markers, mask))
    np.testing.assert_array_equal(out[1].cpu().numpy(), orc.watershed(img2, mk2, mask2))
    lab = out[0].cpu().numpy()
    assert lab[order[-1]] == 2 and lab[order[len(order) // 2 - 1]] == 1  # the far end was reached


def test_exact_flood_with_more_frames_than_cus():
    """A call with more frames than CUs runs the heap emulation with the small LDS share (heap levels 0..6 in LDS, the
    rest in the workspace; several frames per CU) -- the variant the benchmark's quantised leg uses.  300 small frames
    full of ties, mode 1 (exact flood for every frame), each against the oracle."""
    import torch
    from particle_col_image_segmentation_amd import ops
    rng = np.random.default_rng(11)
    B, H, W = 300, 40, 56
    img = (rng.integers(0, 6, (B, H, W)) / 8.0).astype(np.float32)       # six levels: plateaus and equal seeds everywhere
    mask = rng.random((B, H, W)) < 0.9
    markers = np.zeros((B, H, W), np.int32)
    for b in range(B):
        for k in range(1, 9):
            markers[b, rng.integers(0, H), rng.integers(0, W)] = k
    out, flags = ops.watershed(torch.from_numpy(img).cuda(), torch.from_numpy(markers).cuda(),
                               torch.from_numpy(mask.astype(np.uint8)).cuda(), mode=1)
    got = out.cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(got[b], orc.watershed(img[b], markers[b], mask[b]), err_msg="frame %d" % b)
    # and through the default mode (parallel flood first, exact flood only where it cannot be proven)
    out0, flags0 = ops.watershed(torch.from_numpy(img).cuda(), torch.from_numpy(markers).cuda(),
                                 torch.from_numpy(mask.astype(np.uint8)).cuda(), mode=0)
    assert torch.equal(out0, out)
    assert int(flags0.sum()) > 0


def test_corrupted_root_image_raises_the_flag_not_a_fault():
    """The label passes walk parent entries to their roots.  A well-formed union-find image only ever points at an earlier
    pixel of the same frame, and every walk is FENCED to exactly that (csrc/union_find.h, walk_ok): a deliberately corrupted
    root image -- an entry far past the frame, a forward pointer, a two-cycle -- must come back as counts[b] = -1 for that
    frame, with the other frames of the call labelled as usual, and never as a wild load (round-3 review: the fault in
    profiles/r03/exp_graph_r3a.log came from a parent array rewritten under a running chain)."""
    from particle_col_image_segmentation_amd import ops
    rng = np.random.default_rng(11)
    H, W = 96, 128
    masks = (rng.random((5, H, W)) < 0.55).astype(np.uint8)
    labels = np.stack([orc.label(m.astype(bool)) for m in masks])
    roots = np.zeros((5, H, W), np.int32)
    for b in range(5):  # root image = linear index of each component's first pixel + 1
        flat = labels[b].ravel()
        first = np.full(int(flat.max()) + 1, -1, np.int64)
        idx = np.arange(flat.size)
        order = np.argsort(flat, kind="stable")
        lab_sorted = flat[order]
        starts = np.r_[0, np.flatnonzero(np.diff(lab_sorted)) + 1]
        first[lab_sorted[starts]] = idx[order][starts]
        r = first[flat] + 1
        r[flat == 0] = 0
        roots[b] = r.reshape(H, W)
    bad = roots.copy()
    n = H * W
    fg1 = np.flatnonzero(bad[1].ravel())
    bad[1].reshape(-1)[fg1[len(fg1) // 2]] = 2_000_000_000          # far past the frame (and the whole buffer)
    fg3 = np.flatnonzero(bad[3].ravel())
    i, j = int(fg3[10]), int(fg3[-10])
    bad[3].reshape(-1)[i] = j + 1                                    # forward pointer ...
    bad[3].reshape(-1)[j] = i + 1                                    # ... closing a two-cycle
    bad[4].reshape(-1)[n - 1] = n + 5                                # one past the frame's end, at its last pixel
    good_l, good_c = ops.compact_labels(torch.from_numpy(roots).cuda())
    got_l, got_c = ops.compact_labels(torch.from_numpy(bad).cuda())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(good_l.cpu().numpy(), labels)
    assert good_c.cpu().tolist() == [int(l.max()) for l in labels]
    assert got_c.cpu().tolist()[1] == -1 and got_c.cpu().tolist()[3] == -1 and got_c.cpu().tolist()[4] == -1
    for b in (0, 2):  # untouched frames of the same call
        assert int(got_c[b]) == int(labels[b].max())
        np.testing.assert_array_equal(got_l[b].cpu().numpy(), labels[b])
