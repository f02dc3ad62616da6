"""Grayscale reconstruction and the h-maxima markers on the device (csrc/reconstruct.hip) against scikit-image
(tests/golden/reconstruct.npz) and the numpy restatement of tests/test_reconstruct_cpu.py -- every comparison is equality,
float64 by value --: every fixture case, batches whose frames end at different times, a level across every seam of the tiling
in each of the eight directions, the seed-above-mask flag, and the marker chain through ``refine_boundaries`` and
``FramePipeline(marker_h=...)``, eagerly and as a captured graph."""
import functools

import numpy as np
import pytest

from test_reconstruct_cpu import (boundary_map, h_extrema_np, label8_np, load_fixture, reconstruct_np, serpentine)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TW, TH = 64, 32  # csrc/reconstruct.hip: tile width and height (REC_TW, REC_TH); six grid rounds, then the per-frame tail kernel


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")


@functools.lru_cache(maxsize=None)
def _fixture():
    return load_fixture()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _reconstruct(seed, mask, method="dilation", conn=8, check=True):
    """numpy (H, W) or (B, H, W) -> (numpy result of the same rank, flags list)"""
    from particle_col_image_segmentation_amd import ops
    single = np.ndim(mask) == 2
    s, m = (np.asarray(a)[None] if single else np.asarray(a) for a in (seed, mask))
    out, flags = ops.reconstruct(_dev(s), _dev(m), method=method, conn=conn, check=check)
    out = out.cpu().numpy()
    return (out[0] if single else out), flags.cpu().tolist()


def test_geometry_is_what_the_sizes_assume():
    from particle_col_image_segmentation_amd import ops
    assert ops.RECONSTRUCT_TILE == (TW, TH)
    # 70 x 130 and 134 x 134 end in tiles of 6 rows and of 2 / 6 columns; 20 x 40 is smaller than a tile
    assert (70 % TH, 130 % TW, 134 % TH, 134 % TW) == (6, 2, 6, 6) and 20 < TH and 40 < TW


def test_every_fixture_reconstruction_equals_skimage():
    _need_gpu()
    for name, seed, mask, method, conn, want in _fixture()["rec"]:
        got, flags = _reconstruct(seed, mask, method, conn)
        assert got.dtype == mask.dtype and flags == [0], name
        np.testing.assert_array_equal(got, want, err_msg=name)


def test_float32_is_widened():
    _need_gpu()
    name, seed, mask, method, conn, want = next(c for c in _fixture()["rec"] if c[0] == "rf_37x70_dil_c8")
    got, _ = _reconstruct(seed.astype(np.float32), mask.astype(np.float32), method, conn)  # (multiples of 1 / 1024: exact)
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, want)


def test_integer_h_maxima_and_h_minima_equal_skimage():
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    for name, image, h, minima, want in _fixture()["int"]:
        fn = ops.h_minima if minima else ops.h_maxima
        got = fn(_dev(image[None]), h)
        assert got.dtype == torch.uint8
        np.testing.assert_array_equal(got[0].cpu().numpy(), want, err_msg=name)
    image = _dev(_fixture()["int"][0][1][None])
    np.testing.assert_array_equal(ops.h_maxima(image, 3.0).cpu().numpy(), ops.h_maxima(image, 3).cpu().numpy())
    with pytest.raises(ValueError, match="float64 image"):
        ops.h_maxima(image, 0.5)
    for h in (0, -1, 0.0):
        with pytest.raises(ValueError):
            ops.h_maxima(image, h)
        with pytest.raises(ValueError):
            ops.h_minima(image.to(torch.float64), h)


def test_float64_h_extrema_of_a_batch_are_per_frame():
    """frames of different range in one batch: the range test and the result are the frame's own"""
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    rng = np.random.default_rng(7)
    a = rng.integers(-40, 40, (3, 37, 70)) / 8.0
    a[1] = 0.25 * a[1]          # range below h: nothing
    a[2] = a[2] - 1000.0
    for h in (7.0, 2.5):
        for minima, fn in ((False, ops.h_maxima), (True, ops.h_minima)):
            got = fn(_dev(a), h).cpu().numpy()
            for b in range(3):
                np.testing.assert_array_equal(got[b], h_extrema_np(a[b], h, minima=minima), err_msg="h %s frame %d" % (h, b))
    assert not ops.h_maxima(_dev(a), 7.0)[1].any() and ops.h_maxima(_dev(a), 7.0)[0].any()


def test_edt_maxima_equal_skimage_h_maxima_of_the_distance():
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    d2_of = {}
    for name, binary, h, want, n in _fixture()["edt"]:
        key = name.rsplit("_", 1)[0]
        if key not in d2_of:
            d2_of[key] = ops.edt_sq(_dev(binary.astype(np.uint8)[None]))
        d2 = d2_of[key]
        is_max, markers, counts, flags = ops.edt_maxima(d2, h)
        np.testing.assert_array_equal(is_max[0].cpu().numpy(), want, err_msg=name)
        np.testing.assert_array_equal(markers[0].cpu().numpy(), label8_np(want), err_msg=name)
        assert counts.cpu().tolist() == [n] and flags.cpu().tolist() == [0], name
        # the float64 image given directly
        direct = ops.h_maxima(torch.sqrt(d2.to(torch.float64)), h)
        np.testing.assert_array_equal(direct[0].cpu().numpy(), want, err_msg=name + " float64")
    none, markers, counts, _ = ops.edt_maxima(d2, 1.0, want_mask=False)
    assert none is None and markers is not None
    is_max, none, counts, _ = ops.edt_maxima(d2, 1.0, want_markers=False)
    assert none is None and counts is None and is_max is not None


def _uneven_batch():
    """(seed, mask), 3 x 70 x 130 int32: frame 0 a serpentine seeded at its first pixel, frame 1 constant, frame 2 random"""
    H, W = 70, 130
    rng = np.random.default_rng(11)
    mask = np.stack([serpentine(H, W), np.full((H, W), 4, np.int32), rng.integers(-3, 6, (H, W)).astype(np.int32)])
    seed = np.stack([np.zeros((H, W), np.int32), np.full((H, W), 1, np.int32), mask[2] - rng.integers(0, 5, (H, W)).astype(np.int32)])
    seed[0, 0, 0] = 3
    return seed, mask


def test_frames_of_one_batch_end_at_different_times():
    """frame 0 a serpentine (hundreds of tail rounds), frame 1 constant (none), frame 2 random: each equals its own result"""
    _need_gpu()
    seed, mask = _uneven_batch()
    for dtype in (np.int32, np.float64):
        for conn in (8, 4):
            s, m = seed.astype(dtype), mask.astype(dtype)
            got, flags = _reconstruct(s, m, conn=conn)
            assert flags == [0, 0, 0]
            for b in range(3):
                alone, _ = _reconstruct(s[b], m[b], conn=conn)
                np.testing.assert_array_equal(got[b], alone, err_msg="frame %d" % b)
                np.testing.assert_array_equal(got[b], reconstruct_np(s[b], m[b], conn=conn), err_msg="frame %d" % b)
    assert (got[0] == 3).sum() == (mask[0] == 5).sum() == 4585


GRID_ROUNDS = 6  # csrc/reconstruct.hip: REC_GRID_ROUNDS


def _serpentine_round_bound(H, W):
    """(C, L) for the serpentine: its corridor is a simple path, so the seed's level enters the tiles in the order the path
    does, C seam crossings in all.  A crossing into a tile takes a visit of that tile that loads after the tile before stored,
    and a round visits a tile once: the crossings of one round enter different tiles, at most L = the longest run of
    consecutive crossings into distinct tiles.  (With 8 neighbours the level cuts the corners at the row ends; those lie in
    the tile of the pixels next to them.)  After k rounds at most k L crossings are made, whatever the order of the visits."""
    path = []
    for k, r in enumerate(range(0, H, 2)):
        cols = range(W) if k % 2 == 0 else range(W - 1, -1, -1)
        path += [(r, c) for c in cols]
        if r + 1 < H:
            path.append((r + 1, path[-1][1]))
    assert len(path) == (serpentine(H, W) == 5).sum() and all(serpentine(H, W)[p] == 5 for p in path)
    tiles = [(r // TH, c // TW) for r, c in path]
    entered = [t for s, t in zip(tiles, tiles[1:]) if s != t]
    longest = max(n for i in range(len(entered)) for n in range(1, len(entered) - i + 1) if len(set(entered[i:i + n])) == n)
    return len(entered), longest


def _rounds_with_a_change(seed, mask, conn):
    """rounds of the tiling that change a pixel when every tile reads the halo the round before left (the slowest order: values
    only rise, so a visit that reads anything newer is no further from the fixed point).  The round after the last of them
    finds nothing to do and marks nothing, so the frame has no mark left after that many + 1 rounds at the most."""
    H, W = mask.shape
    R = np.minimum(seed, mask)
    for rounds in range(1000):
        new = R.copy()
        for r0 in range(0, H, TH):
            for c0 in range(0, W, TW):
                ra, rb, ca, cb = max(r0 - 1, 0), min(r0 + TH + 1, H), max(c0 - 1, 0), min(c0 + TW + 1, W)
                m = R[ra:rb, ca:cb].copy()      # the halo cannot rise: its mask is its value
                m[r0 - ra:r0 - ra + TH, c0 - ca:c0 - ca + TW] = mask[r0:r0 + TH, c0:c0 + TW]
                local = reconstruct_np(R[ra:rb, ca:cb], m, conn=conn)
                new[r0:r0 + TH, c0:c0 + TW] = local[r0 - ra:r0 - ra + TH, c0 - ca:c0 - ca + TW]
        if (new == R).all():
            np.testing.assert_array_equal(R, reconstruct_np(seed, mask, conn=conn))
            return rounds
        R = new
    raise AssertionError("no fixed point")


def test_the_round_cap_flags_the_frame_that_reaches_it_and_no_other():
    """max_rounds = 2: the tail gives up on a frame that still has a mark after GRID_ROUNDS + 2 rounds.  The serpentine of frame 0
    does (its level has C = 72 seams to cross and crosses at most L = 6 a round); frames 1 and 2 are done within the grid rounds
    (no round, 3 rounds change a pixel of them) and are results.  The call is bounded: the cap is what ends it."""
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    seed, mask = _uneven_batch()
    crossings, per_round = _serpentine_round_bound(*mask[0].shape)
    print("serpentine: %d seam crossings, at most %d a round" % (crossings, per_round))
    assert (GRID_ROUNDS + 2) * per_round < crossings
    for b in (1, 2):
        n = _rounds_with_a_change(seed[b], mask[b], 8)
        print("frame %d: %d rounds change a pixel" % (b, n))
        assert n + 1 < GRID_ROUNDS
    out, flags, _ = ops._reconstruct(_dev(seed), _dev(mask), "dilation", 8, max_rounds=2)
    assert flags.cpu().tolist() == [ops.RECONSTRUCT_NOT_CONVERGED, 0, 0]
    for b in (1, 2):
        np.testing.assert_array_equal(out[b].cpu().numpy(), reconstruct_np(seed[b], mask[b], conn=8), err_msg="frame %d" % b)
    with pytest.raises(RuntimeError, match=r"did not converge in frame\(s\) \[0\]"):
        ops._check_reconstruct_flags(flags)


DIRECTIONS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))


def _seam_paths():
    """(8, 2 TH, 2 TW) masks: a path of value 7 that crosses the seam between the four tiles in direction (dr, dc) -- the
    straight ones away from the corner, the diagonal ones through it -- seeded with 5 at its first pixel"""
    H, W = 2 * TH, 2 * TW
    mask = np.zeros((8, H, W), np.int32)
    seed = np.zeros((8, H, W), np.int32)
    ends = []
    for k, (dr, dc) in enumerate(DIRECTIONS):
        # the pixel before the seam: on the near side of the row / column seam, or at a fixed place for the other axis
        r = (TH - 1 if dr > 0 else TH) if dr else 10
        c = (TW - 1 if dc > 0 else TW) if dc else 20
        pts = [(r + j * dr, c + j * dc) for j in range(-3, 5)]
        for p in pts:
            mask[k][p] = 7
        seed[k][pts[0]] = 5
        ends.append(pts[-1])
        assert (pts[3][0] // TH, pts[3][1] // TW) != (pts[4][0] // TH, pts[4][1] // TW)  # steps 3 -> 4 change tile
    return seed, mask, ends


def test_a_level_crosses_every_seam_in_each_of_the_eight_directions():
    _need_gpu()
    seed, mask, ends = _seam_paths()
    for dtype in (np.int32, np.float64):
        s, m = seed.astype(dtype), mask.astype(dtype)
        for conn in (8, 4):
            got, flags = _reconstruct(s, m, conn=conn)
            ero, eflags = _reconstruct(-s, -m, "erosion", conn)
            assert flags == eflags == [0] * 8
            for k, (dr, dc) in enumerate(DIRECTIONS):
                np.testing.assert_array_equal(got[k], reconstruct_np(s[k], m[k], conn=conn), err_msg="direction %s" % ((dr, dc),))
                np.testing.assert_array_equal(ero[k], -got[k], err_msg="erosion, direction %s" % ((dr, dc),))
                # the level arrives at the far end, except along a diagonal path without diagonal neighbours
                assert got[k][ends[k]] == (5 if conn == 8 or dr * dc == 0 else 0), (dtype, conn, dr, dc)


def test_seed_above_the_mask_raises_or_is_clamped_and_flagged():
    _need_gpu()
    from particle_col_image_segmentation_amd import ops
    rng = np.random.default_rng(5)
    mask = rng.integers(0, 9, (2, 37, 70)).astype(np.int32)
    seed = mask - rng.integers(0, 5, (2, 37, 70)).astype(np.int32)
    seed[0, 36, 69] = mask[0, 36, 69] + 2
    for dtype in (np.int32, np.float64):
        s, m = seed.astype(dtype), mask.astype(dtype)
        with pytest.raises(ValueError, match="less than that of the mask image for reconstruction by dilation"):
            _reconstruct(s, m)
        got, flags = _reconstruct(s, m, check=False)
        assert flags == [ops.RECONSTRUCT_SEED_BEYOND_MASK, 0]
        for b in range(2):
            np.testing.assert_array_equal(got[b], reconstruct_np(np.minimum(s[b], m[b]), m[b]))
        with pytest.raises(ValueError, match="greater than that of the mask image for reconstruction by erosion"):
            _reconstruct(-s, -m, "erosion")
        got, flags = _reconstruct(-s, -m, "erosion", check=False)
        assert flags == [ops.RECONSTRUCT_SEED_BEYOND_MASK, 0]
        np.testing.assert_array_equal(got[0], reconstruct_np(np.maximum(-s[0], -m[0]), -m[0], "erosion"))
    with pytest.raises(ValueError, match="one of 'erosion' or 'dilation'"):
        ops.reconstruct(_dev(seed), _dev(mask), method="closing")
    with pytest.raises(ValueError):
        ops.reconstruct(_dev(seed), _dev(mask), conn=6)


def test_the_extremes_of_int32_are_values_like_any_other():
    _need_gpu()
    lo, hi = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    mask = np.full((TH + 3, TW + 3), hi, np.int32)
    mask[:, TW - 1] = lo          # a wall of the type's minimum next to the seam
    mask[5, TW - 1] = hi - 1      # ... with one door
    seed = np.full_like(mask, lo)
    seed[0, 0] = hi
    for conn in (8, 4):
        got, _ = _reconstruct(seed, mask, conn=conn)
        np.testing.assert_array_equal(got, reconstruct_np(seed, mask, conn=conn))
        assert got[0, 0] == hi and got[7, TW + 1] == hi - 1 and got[9, TW - 1] == lo
        ero, _ = _reconstruct(-1 - seed, -1 - mask, "erosion", conn)   # (-1 - x maps lo <-> hi without overflow)
        np.testing.assert_array_equal(ero, -1 - got)


def test_refine_boundaries_with_marker_h_equals_the_skimage_chain():
    _need_gpu()
    from particle_col_image_segmentation_amd.refine_boundaries import refine_boundaries
    for s, h, markers, labels, count in _fixture()["chain"]:
        bm = boundary_map(s, 96, 80)
        st = refine_boundaries(bm, marker_h=h, return_stages=True)
        np.testing.assert_array_equal(st["local_max"], markers > 0, err_msg="seed %d h %s" % (s, h))
        np.testing.assert_array_equal(st["markers"], markers, err_msg="seed %d h %s" % (s, h))
        np.testing.assert_array_equal(st["labels"], labels, err_msg="seed %d h %s" % (s, h))
        np.testing.assert_array_equal(refine_boundaries(bm, marker_h=h), labels)
        assert int(st["markers"].max()) == count


def test_pipeline_with_marker_h_eager_and_graph():
    _need_gpu()
    from particle_col_image_segmentation_amd import synth
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    from particle_col_image_segmentation_amd.refine_boundaries import refine_boundaries
    dev = torch.device("cuda")
    stack = synth.gen_batch_torch(4242, 2, 128, 128, dev)
    pipe = FramePipeline(dict(synth.CELL_TYPES_5), marker_h=1.0)
    res = pipe.run(stack)
    res.synchronize()
    assert res["marker_flags"].cpu().tolist() == [0, 0]
    n = res["n_markers"].cpu().tolist()
    for b in range(2):
        st = refine_boundaries(stack[b, pipe.boundary_plane], marker_h=1.0, return_stages=True)
        assert torch.equal(res["markers"][b], st["markers"]) and torch.equal(res["ws_labels"][b], st["labels"])
        assert n[b] == int(st["markers"].max()) > 0
    tabs = pipe.tables(res, refined=True)
    assert [int((tabs["refined"][:, 0] == b).sum()) for b in range(2)] == n
    plain = FramePipeline(dict(synth.CELL_TYPES_5)).run(stack)
    assert "marker_flags" not in plain and plain["n_markers"].sum().item() > sum(n)
    graph = FramePipeline(dict(synth.CELL_TYPES_5), marker_h=1.0, graph=True)
    for _ in range(3):  # one capture per lane, then a replay
        gres = graph.run(stack)
        gres.synchronize()
        for k in ("markers", "n_markers", "ws_labels", "marker_flags", "tie_flags"):
            assert torch.equal(gres[k], res[k]), k
    pipe.synchronize()


def test_h_maxima_markers_are_fewer_than_local_maxima():
    """the behaviour the switch is for: on the 256 x 256 frame of seed 1, scikit-image finds 78 maxima that rise one pixel
    above their surroundings among the 161 local maxima of the distance map"""
    _need_gpu()
    from particle_col_image_segmentation_amd.refine_boundaries import refine_boundaries_batch
    want = next(c[4] for c in _fixture()["edt"] if c[0].startswith("edt_s1_256x256_") and c[2] == 1.0)
    bm = _dev(boundary_map(1, 256, 256).astype(np.float32)[None])
    with_h = refine_boundaries_batch(bm, marker_h=1.0)
    without = refine_boundaries_batch(bm)
    assert with_h["marker_flags"].cpu().tolist() == [0] and "marker_flags" not in without
    n_h, n_all = int(with_h["n_markers"][0].item()), int(without["n_markers"][0].item())
    print("markers with marker_h=1.0: %d, with every local maximum: %d" % (n_h, n_all))
    assert n_h == want == 78
    assert n_h < n_all
    assert int(with_h["labels"].max().item()) == n_h
