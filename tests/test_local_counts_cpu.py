"""Local neighbourhoods (include/pcseg_local.h, local.py, FramePipeline.neighbourhoods) without a GPU: the numpy restatements of
tests/local_reference.py against closed forms, against tests/window_reference.py and against tests/mixing_reference.py, the
header's exports and their refusals through ctypes, the argument contract of the public functions of ``local``
(``ops._on_device`` replaced, as tests/test_ops_contract_cpu.py does) and the table's arithmetic on CPU tensors with the two
device entries replaced by their restatements.  Every comparison is by equality."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import local_reference as lr
import mixing_reference as mr
import ops_contract_cases as cc
import window_reference as wr
from test_window_pairs_cpu import masks

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATTICE = np.array([0, 1, 2, 4, 5, 25, 50, 81], np.int64)  # the thresholds of [0, 1, sqrt 2, 2, sqrt 5, 5, sqrt 50, 9] at scale 1


def ring_lattice_points(H, W, pr, pc, thr):
    """the lattice points of every ring around (pr, pc) clipped to the H x W rectangle, row by row with integer square roots"""
    def disk(t):  # points with d2 < t
        n = 0
        for y in range(H):
            rest = t - 1 - (y - pr) ** 2
            if rest >= 0:
                h = math.isqrt(rest)
                n += max(0, min(pc + h, W - 1) - max(pc - h, 0) + 1)
        return n
    cum = [disk(int(t)) for t in thr]
    return np.diff(np.array(cum, np.int64))


@pytest.mark.parametrize("H,W", [(1, 1), (2, 33), (9, 65), (7, 70)])
def test_full_mask_rings_are_clipped_lattice_rings(H, W):
    planes = np.full((1, H, W), 0xFF, np.uint8)
    queries = np.array([(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2), (-1, -1), (H, W // 2), (H // 2, -3),
                        (H + 100, W + 100)], np.int64)
    for thr in (LATTICE, np.array([0, 1], np.int64), np.array([0, 3, (H + W) ** 2 + 5], np.int64)):
        counts, area = lr.disk_counts(planes, queries, [0, len(queries)], thr, 2)
        assert area.tolist() == [[H * W, H * W]]
        for i, (pr, pc) in enumerate(queries):
            want = ring_lattice_points(H, W, int(pr), int(pc), thr)
            np.testing.assert_array_equal(counts[i, 0], want, err_msg=str((pr, pc)))
            np.testing.assert_array_equal(counts[i, 1], want)
    inside = lr.disk_counts(planes, queries[:5], [0, 5], np.array([0, 1], np.int64), 1)[0]
    assert inside.reshape(-1).tolist() == [1] * 5  # ring 0 of [0, 1): the query pixel itself
    assert lr.disk_counts(planes, queries[5:6], [0, 1], np.array([0, 1, 3], np.int64), 1)[0].reshape(-1).tolist() == [0, 1]  # (-1, -1): (0, 0) at d2 = 2


@pytest.mark.parametrize("H,W", [(1, 31), (5, 64), (9, 65), (17, 32)])
def test_all_window_pixels_as_queries_give_the_window_histogram(H, W):
    for name, M in masks(H, W, seed=3).items():
        queries = np.argwhere(M)
        for thr in (LATTICE, np.array([0, 3, (H + W) ** 2 + 5], np.int64)):
            counts, area = lr.disk_counts(M[None].astype(np.uint8), queries, [0, len(queries)], thr, 1)
            want = wr.window_hist(M, thr)
            np.testing.assert_array_equal(counts[:, 0].sum(axis=0), want[1:-1], err_msg=name)
            assert area[0, 0] == want[0]


def test_sets_are_independent_bits_and_higher_bits_are_ignored():
    rng = np.random.default_rng(5)
    planes = rng.integers(0, 256, (2, 9, 33)).astype(np.uint8)
    queries = np.array([(4, 16), (0, 0), (8, 32), (3, 3)], np.int64)
    foff = [0, 3, 4]
    all8, area8 = lr.disk_counts(planes, queries, foff, LATTICE, 8)
    for c in range(8):
        one, area1 = lr.disk_counts(((planes >> c) & 1).astype(np.uint8) | 0xFE, queries, foff, LATTICE, 1)
        np.testing.assert_array_equal(all8[:, c], one[:, 0])
        np.testing.assert_array_equal(area8[:, c], area1[:, 0])
    three, _ = lr.disk_counts(planes, queries, foff, LATTICE, 3)
    np.testing.assert_array_equal(three, all8[:, :3])
    assert (all8[3] != lr.disk_counts(planes, queries[3:], [0, 1, 1], LATTICE, 8)[0][0]).any()  # query 3 counts in frame 1


def _points(seed, sizes, K, extent=12):
    rng = np.random.default_rng([seed, K])
    n = sum(sizes)
    xy = rng.integers(0, 2 * extent, (n, 2)).astype(np.float64) / 2.0  # a half-pixel lattice: duplicates and exact edge distances
    slot = rng.integers(-1, K + 1, n).astype(np.int32)
    xy[1], slot[:2] = xy[0], 0  # a duplicate position: a pair at distance 0
    return xy, slot, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_point_counts_sum_to_the_pair_histogram(K):
    xy, slot, foff = _points(7, (40, 0, 1, 23), K)
    edges = np.array([0.0, 0.5, 1.0, np.sqrt(2.0), 2.5, 5.0])
    for scale in (1.0, 1.5):
        got = lr.point_counts(xy, slot, foff, K, scale, edges)
        typed = (slot >= 0) & (slot < K)
        assert (got[~typed] == -1).all() and (got[typed] >= 0).all() and got[typed][:, :, 0].sum() > 0
        brute = mr.mixing(xy, slot, foff, K, scale, edges, 0)[:, 0]  # (B, Q, m): the observed labelling
        np.testing.assert_array_equal(brute, lr.pair_hist_bins(xy, slot, foff, K, scale, edges))
        q = 0
        for a in range(K):
            for b in range(a, K):
                for f in range(len(foff) - 1):
                    sel = np.arange(len(slot))
                    sel = sel[(sel >= foff[f]) & (sel < foff[f + 1]) & (slot[sel] == a)]
                    np.testing.assert_array_equal(got[sel][:, b].sum(axis=0), brute[f, q] * (2 if a == b else 1))
                q += 1


def test_exports_and_binding():
    from particle_col_image_segmentation_amd import _lib, local, spatial
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pcseg_local.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(pcseg_\w+)\s*\(", text)))
    assert names == sorted(local.SIGNATURES) == ["pcseg_disk_counts", "pcseg_disk_counts_workspace_bytes", "pcseg_local_bins",
                                                 "pcseg_local_point_tile", "pcseg_local_rows", "pcseg_point_counts",
                                                 "pcseg_point_counts_workspace_bytes"]
    assert not set(names) & set(_lib.SIGNATURES) and not set(names) & set(_lib.WORKSPACE) and not set(names) & set(spatial.SIGNATURES)
    lib = local._load()
    assert lib is _lib.load()
    for name, (res, args) in local.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)  # the header's argument counts
        assert len([a for a in decl.split(",") if a.strip() != "void"]) == len(args), name
    assert local.local_rows() == lib.pcseg_local_rows() >= 1 and local.local_bins() == lib.pcseg_local_bins() >= 1
    assert local.local_point_tile() == lib.pcseg_local_point_tile() >= 1


def test_what_the_new_method_leaves_as_it_was():
    from particle_col_image_segmentation_amd import _lib, local, ops, spatial
    from particle_col_image_segmentation_amd.pipeline import OPTIONAL_TABLES, FramePipeline, TableSwitches
    assert not any("neighbourhood" in t.name for t in OPTIONAL_TABLES) and not any("neighbourhood" in f for f in TableSwitches._fields)
    assert not any("disk_counts" in n or "point_counts" in n for n in list(_lib.SIGNATURES) + list(_lib.WORKSPACE))
    assert not set(local.SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.WORKSPACE))
    assert not any("disk_counts" in n or "point_counts" in n or "neighbourhood" in n for n in cc.public_functions(ops))
    assert cc.public_functions(spatial) == ["clustering_columns", "pair_expectation", "window_pair_counts", "window_reach", "window_rows"]
    assert cc.public_functions(local) == ["disk_counts", "local_bins", "local_point_tile", "local_rows", "neighbourhood_columns",
                                          "neighbourhood_tables", "point_counts", "set_planes", "window_queries"]
    assert callable(FramePipeline.neighbourhoods) and callable(FramePipeline.clustering)


@pytest.fixture(scope="module")
def lib():
    from particle_col_image_segmentation_amd import local
    return local._load()


def _rejected(lib, rc, code=-1, text=None):
    assert rc == code, (rc, lib.pcseg_last_error())
    assert lib.pcseg_last_error() and (text is None or text in lib.pcseg_last_error().decode())


def test_the_library_refuses_bad_arguments(lib):
    from particle_col_image_segmentation_amd import spatial
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)  # never dereferenced: every call is refused before any launch
    e = (ctypes.c_double * 3)(0.0, 1.0, 2.0)
    many = (ctypes.c_double * 1026)(*np.arange(1026.0))
    far = (ctypes.c_double * 2)(0.0, spatial.MAX_REACH + 1.5)  # reach MAX_REACH + 1
    near = (ctypes.c_double * 2)(0.0, spatial.MAX_REACH + 0.5)
    # ---- disk_counts: the size query
    q = lib.pcseg_disk_counts_workspace_bytes
    nbytes = q(2, 3, 40, 70, 3, 1)
    assert nbytes >= 2 * 3 * 40 * 4 * 8 and q(2, 4, 40, 70, 3, 1) > nbytes and q(2, 3, 40, 70, 3, spatial.MAX_REACH) > nbytes
    for bad in ((0, 3, 40, 70, 3, 1), (2, 0, 40, 70, 3, 1), (2, 9, 40, 70, 3, 1), (2, 3, 0, 70, 3, 1), (2, 3, 40, 0, 3, 1),
                (70000, 3, 40, 70, 3, 1), (2, 3, 40, 70, 1, 1), (2, 3, 40, 70, 1027, 1), (2, 3, 40, 70, 3, -1),
                (2, 3, 40, 70, 3, spatial.MAX_REACH + 1), (1, 3, 40000, 40000, 3, 1)):
        assert q(*bad) == 0, bad

    def run(**k):
        return lib.pcseg_disk_counts(k.get("planes", p), k.get("B", 2), k.get("C", 3), k.get("H", 40), k.get("W", 70), k.get("queries", p),
                                     k.get("foff", p), k.get("n", 5), k.get("scale", 1.0), k.get("edges", e), k.get("n_edges", 3),
                                     k.get("counts", p), k.get("area", p), k.get("ws", p), k.get("nbytes", nbytes), None)

    for bad in (dict(planes=null), dict(queries=null), dict(foff=null), dict(counts=null), dict(area=null), dict(ws=null), dict(B=0),
                dict(B=70000), dict(C=0), dict(C=9), dict(H=0), dict(W=0), dict(n=-1), dict(n=1 << 31), dict(scale=0.0),
                dict(scale=float("inf")), dict(edges=null), dict(n_edges=1), dict(edges=many, n_edges=1026),
                dict(edges=(ctypes.c_double * 3)(0.0, 1.0, 1.0)), dict(edges=(ctypes.c_double * 3)(0.0, 2.0, 1.0)),
                dict(edges=(ctypes.c_double * 3)(0.1, 1.0, 2.0)), dict(edges=(ctypes.c_double * 3)(0.0, 1.0, float("nan")))):
        _rejected(lib, run(**bad), text="bad arguments")
    _rejected(lib, run(edges=far, n_edges=2, nbytes=1 << 40), text="PCSEG_WINDOW_MAX_REACH")
    _rejected(lib, run(nbytes=nbytes - 1), -3, "workspace too small")
    _rejected(lib, run(edges=near, n_edges=2, nbytes=q(2, 3, 40, 70, 2, spatial.MAX_REACH) - 1), -3, "workspace too small")
    # ---- point_counts
    q = lib.pcseg_point_counts_workspace_bytes
    nbytes = q(10, 2, 3, 3)
    assert nbytes >= 3 * 8
    for bad in ((-1, 2, 3, 3), (1 << 24, 2, 3, 3), (10, 0, 3, 3), (10, 2, 0, 3), (10, 2, 5, 3), (10, 2, 3, 1), (10, 2, 3, 0), (10, 2, 3, 1027)):
        assert q(*bad) == 0, bad

    def run(**k):
        return lib.pcseg_point_counts(k.get("xy", p), k.get("slot", p), k.get("foff", p), k.get("n", 10), k.get("B", 2), k.get("K", 3),
                                      k.get("scale", 1.0), k.get("edges", e), k.get("n_edges", 3), k.get("counts", p), k.get("ws", p),
                                      k.get("nbytes", nbytes), None)

    for bad in (dict(xy=null), dict(slot=null), dict(foff=null), dict(counts=null), dict(ws=null), dict(n=-1), dict(n=1 << 24), dict(B=0),
                dict(K=0), dict(K=5), dict(scale=0.0), dict(scale=float("nan")), dict(edges=null), dict(edges=null, n_edges=0),
                dict(n_edges=1), dict(edges=many, n_edges=1026), dict(edges=(ctypes.c_double * 3)(0.0, 1.0, 1.0)),
                dict(edges=(ctypes.c_double * 3)(0.5, 1.0, 2.0))):
        _rejected(lib, run(**bad), text="bad arguments")
    _rejected(lib, run(nbytes=nbytes - 1), -3, "workspace too small")


# ------------------------------------------------------------------ the argument contract of local's public functions
@pytest.fixture
def backend(monkeypatch):
    from particle_col_image_segmentation_amd import ops
    cc.install(ops, monkeypatch)
    monkeypatch.setattr(ops, "_on_device", lambda t: isinstance(t, torch.Tensor) and t.device.type == "cpu")
    return cc.Backend(ops, "cpu", "meta")


E3 = [0.0, 1.0, 2.5, 4.0]
# function name -> (tensor arguments name -> (dtype, shape), the other arguments)
CONTRACT = {
    "disk_counts": ({"planes": (torch.uint8, (2, 9, 11)), "queries": (torch.int32, (7, 2)), "frame_offsets": (torch.int64, (3,))},
                    dict(edges=E3, scale=1.0)),
    "point_counts": ({"xy": (torch.float64, (7, 2)), "slot": (torch.int32, (7,)), "frame_offsets": (torch.int64, (3,))},
                     dict(K=2, scale=1.0, edges=E3)),
}


def _arguments(backend, fn, **swap):
    tensors, rest = CONTRACT[fn]
    kw = {k: backend.tensor(*spec) for k, spec in tensors.items()}
    kw.update(rest)
    kw.update(swap)
    return kw


def test_valid_calls_pass_the_checks(backend):
    from particle_col_image_segmentation_amd import local
    for fn in CONTRACT:
        with pytest.raises(cc.Reached) as info:
            getattr(local, fn)(**_arguments(backend, fn))
        assert info.value.entry == fn
    with pytest.raises(cc.Reached):  # bool is read as uint8
        local.disk_counts(**_arguments(backend, "disk_counts", planes=torch.zeros((2, 9, 11), dtype=torch.bool)))
    with pytest.raises(cc.Reached):  # no query: the areas are still counted
        local.disk_counts(**_arguments(backend, "disk_counts", queries=torch.zeros((0, 2), dtype=torch.int32)))


@pytest.mark.parametrize("fn,arg", [(fn, arg) for fn, (tensors, _) in CONTRACT.items() for arg in tensors])
def test_mutated_calls_are_refused_before_the_library(backend, fn, arg):
    from particle_col_image_segmentation_amd import local
    dtype, shape = CONTRACT[fn][0][arg]
    other = cc.NEIGHBOURS[dtype][0]
    for kind, value, raises in (("foreign", backend.foreign(dtype, shape), TypeError),
                                ("numpy", np.zeros(shape, cc.NUMPY[dtype]), TypeError),
                                ("dtype", backend.tensor(other, shape), TypeError),
                                ("rank+", backend.tensor(dtype, (1,) + shape), ValueError),
                                ("rank-", backend.tensor(dtype, shape[1:]), ValueError)):
        with pytest.raises(raises) as info:
            getattr(local, fn)(**_arguments(backend, fn, **{arg: value}))
        assert info.type is raises, (kind, info.value)
    if arg in ("queries", "xy"):  # (n, 3)
        with pytest.raises(ValueError):
            getattr(local, fn)(**_arguments(backend, fn, **{arg: backend.tensor(dtype, (7, 3))}))
    if arg == "slot":
        with pytest.raises(ValueError):
            local.point_counts(**_arguments(backend, fn, slot=backend.tensor(dtype, (8,))))
    if fn == "disk_counts" and arg == "frame_offsets":  # B + 1 entries
        with pytest.raises(ValueError):
            local.disk_counts(**_arguments(backend, fn, frame_offsets=backend.tensor(dtype, (4,))))


def test_a_non_contiguous_input_is_copied_not_refused(backend, monkeypatch):
    from particle_col_image_segmentation_amd import local, ops
    seen = []

    def hook(entry, *args, **kwargs):
        seen.append(args)
        raise cc.Reached(entry)

    monkeypatch.setattr(ops, "_call", hook)
    planes = backend.strided(torch.uint8, (2, 9, 11))
    planes[1, 2, 3] = 5
    with pytest.raises(cc.Reached):
        local.disk_counts(**_arguments(backend, "disk_counts", planes=planes))
    assert seen[0][0].is_contiguous() and seen[0][0].data_ptr() != planes.data_ptr() and torch.equal(seen[0][0], planes)
    xy = backend.strided(torch.float64, (7, 2))
    with pytest.raises(cc.Reached):
        local.point_counts(**_arguments(backend, "point_counts", xy=xy))
    assert seen[1][0].is_contiguous() and seen[1][0].data_ptr() != xy.data_ptr()


def test_edges_reach_and_sizes_are_refused_before_the_library(backend):
    from particle_col_image_segmentation_amd import local, spatial
    bad_edges = ([0.0], [0.0, 0.0], [0.5, 1.0], [0.0, 2.0, 1.0], [0.0, float("nan")], np.arange(1026.0), None)
    for edges in bad_edges + ([0.0, spatial.MAX_REACH + 1.5], [0.0, 1e300]):
        with pytest.raises(ValueError):
            local.disk_counts(**_arguments(backend, "disk_counts", edges=edges))
    for edges in bad_edges:
        with pytest.raises(ValueError):
            local.point_counts(**_arguments(backend, "point_counts", edges=edges))
    for fn in CONTRACT:
        with pytest.raises(ValueError):
            getattr(local, fn)(**_arguments(backend, fn, scale=0.0))
    for sets in (0, 9):
        with pytest.raises(ValueError):
            local.disk_counts(sets=sets, **_arguments(backend, "disk_counts"))
    for K in (0, 5):
        with pytest.raises(ValueError):
            local.point_counts(**_arguments(backend, "point_counts", K=K))
    with pytest.raises(cc.Reached):
        local.disk_counts(**_arguments(backend, "disk_counts", edges=[0.0, spatial.MAX_REACH + 0.5]))  # at the limit
    with pytest.raises(cc.Reached):
        local.point_counts(**_arguments(backend, "point_counts", edges=[0.0, 1e300]))  # point distances know no reach


def test_empty_batches_return_without_a_launch(backend):
    from particle_col_image_segmentation_amd import local
    counts, area = local.disk_counts(backend.tensor(torch.uint8, (0, 9, 11)), backend.tensor(torch.int32, (0, 2)),
                                     backend.tensor(torch.int64, (1,)), E3, 1.0, sets=3)
    assert tuple(counts.shape) == (0, 3, 3) and tuple(area.shape) == (0, 3) and counts.dtype == torch.int32 and area.dtype == torch.int64
    got = local.point_counts(backend.tensor(torch.float64, (0, 2)), backend.tensor(torch.int32, (0,)), backend.tensor(torch.int64, (3,)), 2,
                             1.0, E3)
    assert tuple(got.shape) == (0, 2, 3) and got.dtype == torch.int32
    got = local.point_counts(backend.tensor(torch.float64, (0, 2)), backend.tensor(torch.int32, (0,)), backend.tensor(torch.int64, (1,)), 2,
                             1.0, E3)
    assert tuple(got.shape) == (0, 2, 3)
    with pytest.raises(ValueError):  # points, but no frame to hold them
        local.point_counts(backend.tensor(torch.float64, (7, 2)), backend.tensor(torch.int32, (7,)), backend.tensor(torch.int64, (1,)), 2,
                           1.0, E3)


def test_set_planes(monkeypatch):
    from particle_col_image_segmentation_amd import local, ops
    monkeypatch.setattr(ops, "_on_device", lambda t: isinstance(t, torch.Tensor))
    slot = np.full(256, 255, np.uint8)
    slot[[1, 2, 9, 200]] = [0, 1, 1, 3]
    cm = torch.tensor([[[0, 1, 2, 9], [200, 5, 255, 1]]], dtype=torch.uint8)
    window = torch.tensor([[[0, 7, 0, 1], [1, 1, 0, 0]]], dtype=torch.uint8)
    got = local.set_planes(window, cm, slot)
    assert got.dtype == torch.uint8 and got.tolist() == [[[0, 1 | 2, 4, 1 | 4], [1 | 16, 1, 0, 2]]]
    with pytest.raises(ValueError):
        local.set_planes(window, cm[:, :1], slot)


# ------------------------------------------------------------------ the table
def _table_case(seed=3, K=3):
    rng = np.random.default_rng(seed)
    B, H, W = 3, 14, 19
    planes = rng.integers(0, 1 << (1 + K), (B, H, W)).astype(np.uint8)
    planes[0] |= 1
    planes[2] &= 0xFE  # frame 2: an empty window
    sizes = (9, 6, 4)
    n = sum(sizes)
    rc = rng.uniform(-1.0, 15.0, (n, 2))
    rc[:, 1] = rng.uniform(-1.0, 20.0, n)
    rc[1] = rc[0]  # a duplicate position
    slot = rng.integers(-1, K + 1, n).astype(np.int32)
    slot[:2] = 0
    ids = np.arange(1, n + 1).astype(np.int32)
    foff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    xy = np.stack([rc[:, 1] + 1.0, rc[:, 0] + 1.0], axis=1)
    return planes, xy, rc, slot, ids, foff


def test_the_table_equals_the_restatement(monkeypatch):
    """``neighbourhood_tables`` on CPU tensors with the two device entries replaced by their restatements: the float expressions,
    in their order, the NaN placement and the row order"""
    from particle_col_image_segmentation_amd import local, ops
    K, scale = 3, 2.0
    planes, xy, rc, slot, ids, foff = _table_case(K=K)
    edges = np.array([0.0, 0.5, 1.0, 1.5, 2.5, 4.0])
    thr = np.array([0, 1, 4, 9, 25, 64], np.int64)  # sqrt(n) / 2 >= e: n >= (2 e)^2
    monkeypatch.setattr(ops, "_on_device", lambda t: isinstance(t, torch.Tensor))

    def point_counts(xy_t, slot_t, foff_t, K_, scale_, edges_):
        return torch.from_numpy(lr.point_counts(xy_t.numpy(), slot_t.numpy(), foff_t.numpy(), K_, scale_, np.asarray(edges_)).astype(np.int32))

    def disk_counts(planes_t, queries_t, foff_t, edges_, scale_, sets=8):
        counts, area = lr.disk_counts(planes_t.numpy(), queries_t.numpy(), foff_t.numpy(), thr, sets)
        return torch.from_numpy(counts.astype(np.int32)), torch.from_numpy(area)

    monkeypatch.setattr(local, "point_counts", point_counts)
    monkeypatch.setattr(local, "disk_counts", disk_counts)
    points = ops.Points(torch.from_numpy(xy), torch.from_numpy(slot), torch.from_numpy(ids), torch.from_numpy(foff))
    got = local.neighbourhood_tables(points, torch.from_numpy(rc), torch.from_numpy(planes), edges, scale, K, np.array([7, 3, 11]))
    got = got["neighbourhoods"].numpy()
    want = lr.neighbourhood_rows([7, 3, 11], xy, rc, slot, ids, foff, planes, edges, scale, thr, K)
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
    cols = local.neighbourhood_columns(["a", "b", "c"], edges)
    assert cols == lr.columns(["a", "b", "c"]) and got.shape == (int(((slot >= 0) & (slot < K)).sum()) * 5, len(cols))
    seen = got[:, cols.index("in_window")] == 1
    assert seen.any() and (~seen).any() and np.isnan(got[~seen][:, 7:]).all() and not np.isnan(got[seen][:, 7:9]).any()
    assert (got[got[:, 0] == 11.0][:, 3] == 0).all()  # the empty window: every point is outside
    first = got[:5]  # point 0 and its duplicate: the duplicate counts in bin 0 when both are in the window
    if first[0, 3] == 1:
        assert first[0, cols.index("n_a")] >= 1 and first[-1, cols.index("own_frac")] > 0
    assert np.isfinite(got[seen][:, cols.index("expected_a")]).all()
    # hand arithmetic on one row: expected = (N * win_px) / A
    i = int(np.nonzero(seen)[0][0])
    b = [7, 3, 11].index(int(got[i, 0]))
    A = float((planes[b] & 1).sum())
    typed_in = lambda t: sum(1 for j in range(len(slot)) if foff[b] <= j < foff[b + 1] and slot[j] == t and
                             got[(got[:, 1] == ids[j]) & (got[:, 0] == got[i, 0])][0, 3] == 1)
    N = typed_in(1) - (1 if got[i, 2] == 1 else 0)
    assert got[i, cols.index("expected_b")] == (float(N) * got[i, 7]) / A


def test_neighbourhoods_refuses_bad_arguments_and_names_its_columns():
    from particle_col_image_segmentation_amd import local
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    pipe = FramePipeline()
    res = {"shape": (2, 5, 16, 16)}  # every refusal below comes before the result's tensors are touched
    e = [0.0, 1.0, 2.0]
    for bad in (dict(window="disc"), dict(window=""), dict(of="rois"), dict(of="components"), dict(frame_ids=[1]), dict(frame_ids=[1, 2, 3]),
                dict(frame_ids=[[1, 2]])):
        with pytest.raises(ValueError):
            pipe.neighbourhoods(res, e, **bad)
    for edges in ([0.0, 0.0], [1.0, 2.0], [0.0, 1e300]):
        with pytest.raises(ValueError):
            pipe.neighbourhoods(res, edges, window="frame" if edges[-1] < 10 else "particle")
    with pytest.raises(TypeError):
        pipe.neighbourhoods(res, e, window=np.ones((2, 16, 16), np.uint8))
    assert local.neighbourhood_columns(2) == ["frame", "label", "slot", "in_window", "bin", "r_lo_um", "r_hi_um", "win_px", "cum_win_px",
                                              "n_0", "cum_n_0", "px_0", "cum_px_0", "expected_0", "cum_expected_0",
                                              "n_1", "cum_n_1", "px_1", "cum_px_1", "expected_1", "cum_expected_1", "own_frac", "own_px_frac"]
    assert local.neighbourhood_columns([]) == list(local.NEIGHBOURHOOD_COLUMNS) + ["own_frac", "own_px_frac"]
    assert "lattice" in FramePipeline.neighbourhoods.__doc__
    from particle_col_image_segmentation_amd import tiff_analysis as ta
    with pytest.raises(ValueError):
        ta.get_cell_neighbourhoods(np.zeros((4, 4), np.uint8), {}, {}, {}, None)
    with pytest.raises(ValueError):
        ta.get_cell_neighbourhoods(np.zeros((4, 4), np.uint8), {}, {}, {}, e, window="disc")
