"""Window pair counts (include/pcseg_spatial.h, spatial.py, FramePipeline.clustering) without a GPU: the two numpy
restatements against each other and against closed forms, the header's exports and their refusals through ctypes, the argument
contract of the three public functions of ``spatial`` (``ops._on_device`` replaced, as tests/test_ops_contract_cpu.py does) and
the refusals and column lists of the tables.  Every comparison is by equality."""
import ctypes
import os
import re

import numpy as np
import pytest

import ops_contract_cases as cc
import window_reference as wr

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def blob_with_hole(H, W):
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    cy, cx = (H - 1) / 2.0, (W - 1) / 2.0
    r2 = ((yy - cy) / max(0.45 * H, 1.0)) ** 2 + ((xx - cx) / max(0.45 * W, 1.0)) ** 2
    h2 = ((yy - 0.6 * cy) / max(0.12 * H, 0.6)) ** 2 + ((xx - 1.2 * cx) / max(0.15 * W, 0.6)) ** 2
    return (r2 <= 1.0) & (h2 > 1.0)


def masks(H, W, seed=0):
    """name -> (H, W) bool: the masks every shape is checked on"""
    rng = np.random.default_rng([seed, H, W])
    one = np.zeros((H, W), bool)
    one[H // 2, W // 3] = True
    corners = np.zeros((H, W), bool)
    corners[0, 0] = corners[H - 1, W - 1] = True
    last = np.zeros((H, W), bool)
    last[:, W - 1] = True
    return {"empty": np.zeros((H, W), bool), "full": np.ones((H, W), bool), "one": one, "corners": corners, "last_column": last,
            "checkerboard": (np.add.outer(np.arange(H), np.arange(W)) % 2).astype(bool), "random60": rng.random((H, W)) < 0.6,
            "blob": blob_with_hole(H, W)}


def full_table(H, W, R):
    dy = np.arange(R + 1)[:, None]
    dx = np.abs(np.arange(-R, R + 1))[None, :]
    return (np.clip(H - dy, 0, None) * np.clip(W - dx, 0, None)).astype(np.int64)


SMALL = [(1, 1), (1, 31), (2, 33), (5, 64), (9, 65), (7, 70), (17, 32), (6, 129)]  # at most ~800 px: the brute table is all pairs


@pytest.mark.parametrize("H,W", SMALL)
def test_the_two_restatements_agree_and_match_the_closed_forms(H, W):
    for R in (0, 1, 7, max(H, W) + 3):
        for name, M in masks(H, W).items():
            brute, fft = wr.lag_table_brute(M, R), wr.lag_table_fft(M, R)
            np.testing.assert_array_equal(fft, brute, err_msg="%s R=%d" % (name, R))
            assert brute[0, R] == M.sum()  # gamma(0, 0) = A
            if name == "full":
                np.testing.assert_array_equal(brute, full_table(H, W, R))
    for name, M in masks(H, W).items():
        for thr in ([0, 1], [0, 1, 2, 4, 5, 25, 50], [0, 3, (H + W) ** 2 + 5]):
            h = wr.window_hist(M, thr)
            A = int(M.sum())
            assert h[0] == A and h[1:].sum() == A * A and (h >= 0).all(), (name, thr)
            np.testing.assert_array_equal(wr.window_hist(M, thr, table=wr.lag_table_fft(M, wr.reach(thr))), h)
        assert wr.window_hist(M, [0, 3, (H + W) ** 2 + 5])[-1] == 0  # a last edge beyond the diagonal: nothing is over
        assert wr.window_hist(M, [0, 1])[1] == M.sum()  # the zero lag alone


def test_clustering_rows_on_hand_made_integers():
    obs = np.array([[[2, 0, 1], [1, 1, 0], [0, 0, 0]], [[0, 0, 0]] * 3], np.int64)
    window = np.array([[10, 10, 20, 30, 40], [0, 0, 0, 0, 0]], np.int64)
    rows = wr.clustering_rows([7, 9], [0.0, 1.0, 2.0, 3.0], obs, [[3, 4], [0, 1]], [[1, 0], [0, 2]], window)
    assert rows.shape == (2 * 3 * 3, 18)
    np.testing.assert_array_equal(rows[0], [7, 0, 0, 0, 0.0, 1.0, 3, 3, 1, 1, 2, 10, (3.0 * 10) / 100.0, 2 / ((3.0 * 10) / 100.0),
                                            2, 10, 0.3, 2 / 0.3])
    np.testing.assert_array_equal(rows[4][[1, 2, 3, 6, 7, 10, 11, 12, 14, 15, 16]], [0, 1, 1, 3, 4, 1, 20, (12.0 * 20) / 100.0, 2, 30, 3.6])
    assert np.isnan(rows[9:, 12:14]).all() and np.isnan(rows[9:, 16:]).all()  # A == 0
    np.testing.assert_array_equal(rows[6:9, 10:14], [[0, 10, 0.6, 0], [0, 20, 1.2, 0], [0, 30, 1.8, 0]])  # pair (1, 1): npairs 6


def test_exports_and_binding():
    from particle_col_image_segmentation_amd import _lib, spatial
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pcseg_spatial.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(pcseg_window_\w+)\s*\(", text)))
    assert names == sorted(spatial.SIGNATURES) == ["pcseg_window_pairs", "pcseg_window_pairs_workspace_bytes", "pcseg_window_reach",
                                                   "pcseg_window_rows"]
    assert not set(names) & set(_lib.SIGNATURES) and not set(names) & set(_lib.WORKSPACE)
    lib = spatial._load()
    assert lib is _lib.load()
    for name, (res, args) in spatial.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    for name, (_, args) in spatial.SIGNATURES.items():  # the header's argument counts
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len([a for a in decl.split(",") if a.strip() != "void"]) == len(args), name
    limit = int(re.search(r"#define\s+PCSEG_WINDOW_MAX_REACH\s+(\d+)", text).group(1))
    assert limit == spatial.MAX_REACH >= 1024
    assert spatial.window_rows() == lib.pcseg_window_rows() >= 1


@pytest.fixture(scope="module")
def lib():
    from particle_col_image_segmentation_amd import spatial
    return spatial._load()


def _rejected(lib, rc, code=-1, text=None):
    assert rc == code, (rc, lib.pcseg_last_error())
    assert lib.pcseg_last_error() and (text is None or text in lib.pcseg_last_error().decode())


@pytest.mark.parametrize("scale", [1.0, 9.95, 512.0 / 19.0])
def test_window_reach_against_the_reference(lib, scale):
    from particle_col_image_segmentation_amd import ops, spatial
    rng = np.random.default_rng(3)
    lattice = np.sqrt(np.array([1, 2, 4, 5, 25, 50, 4096, 4097, 10000.0])) / scale
    for last in list(lattice) + list(rng.uniform(0.01, 1500.0 / scale, 40)) + [1e-12, 2048.0 / scale, 2049.5 / scale, 1e6]:
        e = [0.0, last]
        thr = ops.surface_thresholds(e, scale)
        R = spatial.window_reach(e, scale)
        assert R == wr.reach(thr), (last, thr)
        # the definition itself: the largest lag along an axis that lies below the last edge
        assert np.sqrt(float(R * R)) / scale < last and not np.sqrt(float((R + 1) * (R + 1))) / scale < last
    assert spatial.window_reach([0.0, 1.0, 5.0], 1.0) == 4 and spatial.window_reach([0.0, 1.0], 1.0) == 0


def test_the_library_refuses_bad_arguments(lib):
    from particle_col_image_segmentation_amd import spatial
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)  # never dereferenced: every call is refused before any launch
    e = (ctypes.c_double * 3)(0.0, 1.0, 2.0)
    many = (ctypes.c_double * 1026)(*np.arange(1026.0))
    far = (ctypes.c_double * 2)(0.0, spatial.MAX_REACH + 1.5)  # reach MAX_REACH + 1
    near = (ctypes.c_double * 2)(0.0, spatial.MAX_REACH + 0.5)  # reach MAX_REACH
    out = ctypes.c_int64(-7)
    # ---- reach (host only)
    assert lib.pcseg_window_reach(e, 3, 1.0, ctypes.byref(out)) == 0 and out.value == 1
    assert lib.pcseg_window_reach(far, 2, 1.0, ctypes.byref(out)) == 0 and out.value == spatial.MAX_REACH + 1  # no limit of its own
    assert lib.pcseg_window_reach(near, 2, 1.0, ctypes.byref(out)) == 0 and out.value == spatial.MAX_REACH
    for bad in ((null, 3, 1.0, ctypes.byref(out)), (e, 3, 1.0, null), (e, 1, 1.0, ctypes.byref(out)), (e, 3, 0.0, ctypes.byref(out)),
                (e, 3, float("nan"), ctypes.byref(out)), ((ctypes.c_double * 3)(0.0, 2.0, 2.0), 3, 1.0, ctypes.byref(out)),
                ((ctypes.c_double * 3)(0.0, 2.0, 1.0), 3, 1.0, ctypes.byref(out)), ((ctypes.c_double * 3)(0.5, 2.0, 3.0), 3, 1.0, ctypes.byref(out)),
                (many, 1026, 1.0, ctypes.byref(out))):
        _rejected(lib, lib.pcseg_window_reach(*bad), text="bad arguments")
    # ---- the size query
    q = lib.pcseg_window_pairs_workspace_bytes
    nbytes = q(2, 40, 70, 3, 1)
    assert nbytes >= 2 * 40 * 3 * 4 + 2 * 2 * 3 * 4 and q(2, 40, 70, 3, 5) > nbytes
    assert q(2, 40, 70, 3, 500) == q(2, 40, 70, 3, 69) and q(2, 40, 70, 3, spatial.MAX_REACH) > 0  # larger than the image: clamped
    assert q(1, 64, 4096, 2, 1024) > 0  # the limit is at least 1024 px at W = 4096
    for bad in ((0, 40, 70, 3, 1), (2, 0, 70, 3, 1), (2, 40, 0, 3, 1), (70000, 40, 70, 3, 1), (2, 40, 70, 1, 1), (2, 40, 70, 1027, 1),
                (2, 40, 70, 3, -1), (2, 40, 70, 3, spatial.MAX_REACH + 1), (1, 40000, 40000, 3, 1)):
        assert q(*bad) == 0, bad
    # ---- the entry

    def run(**k):
        return lib.pcseg_window_pairs(k.get("mask", p), k.get("B", 2), k.get("H", 40), k.get("W", 70), k.get("scale", 1.0),
                                      k.get("edges", e), k.get("n_edges", 3), k.get("hist", p), k.get("lags", null), k.get("ws", p),
                                      k.get("nbytes", nbytes), None)

    for bad in (dict(mask=null), dict(hist=null), dict(ws=null), dict(B=0), dict(B=70000), dict(H=0), dict(W=0), dict(scale=0.0),
                dict(scale=float("inf")), dict(edges=null), dict(n_edges=1), dict(edges=many, n_edges=1026),
                dict(edges=(ctypes.c_double * 3)(0.0, 1.0, 1.0)), dict(edges=(ctypes.c_double * 3)(0.0, 2.0, 1.0)),
                dict(edges=(ctypes.c_double * 3)(0.1, 1.0, 2.0)), dict(edges=(ctypes.c_double * 3)(0.0, 1.0, float("nan")))):
        _rejected(lib, run(**bad), text="bad arguments")
    _rejected(lib, run(edges=far, n_edges=2, nbytes=1 << 40), text="PCSEG_WINDOW_MAX_REACH")
    _rejected(lib, run(nbytes=nbytes - 1), -3, "workspace too small")
    _rejected(lib, run(nbytes=nbytes - 1, lags=p), -3, "workspace too small")
    _rejected(lib, run(edges=near, n_edges=2, nbytes=q(2, 40, 70, 2, spatial.MAX_REACH) - 1), -3, "workspace too small")


# ------------------------------------------------------------------ the argument contract of spatial's public functions
@pytest.fixture
def backend(monkeypatch):
    from particle_col_image_segmentation_amd import ops
    cc.install(ops, monkeypatch)
    monkeypatch.setattr(ops, "_on_device", lambda t: isinstance(t, torch.Tensor) and t.device.type == "cpu")
    return cc.Backend(ops, "cpu", "meta")


E3 = [0.0, 1.0, 2.5, 4.0]
# function name -> (tensor arguments name -> (dtype, shape), the other arguments)
CONTRACT = {
    "window_pair_counts": ({"mask": (torch.uint8, (2, 9, 11))}, dict(edges=E3, scale=1.0)),
    "pair_expectation": ({"pair_hist": (torch.int64, (2, 3, 5)), "slot_counts": (torch.int64, (2, 2)), "window_hist": (torch.int64, (2, 5))}, {}),
}


def _arguments(backend, fn, **swap):
    tensors, rest = CONTRACT[fn]
    kw = {k: backend.tensor(*spec) for k, spec in tensors.items()}
    kw.update(rest)
    kw.update(swap)
    return kw


def test_public_functions_of_spatial():
    from particle_col_image_segmentation_amd import spatial
    public = cc.public_functions(spatial)
    assert public == ["clustering_columns", "pair_expectation", "window_pair_counts", "window_reach", "window_rows"]
    # window_reach / window_rows / clustering_columns: host only, no tensor argument


def test_valid_calls_pass_the_checks(backend):
    from particle_col_image_segmentation_amd import spatial
    with pytest.raises(cc.Reached) as info:
        spatial.window_pair_counts(**_arguments(backend, "window_pair_counts"))
    assert info.value.entry == "window_pairs"
    with pytest.raises(cc.Reached):
        spatial.window_pair_counts(lags=True, **_arguments(backend, "window_pair_counts"))
    with pytest.raises(cc.Reached):  # bool is read as uint8
        spatial.window_pair_counts(**_arguments(backend, "window_pair_counts", mask=torch.zeros((2, 9, 11), dtype=torch.bool)))
    out = spatial.pair_expectation(**_arguments(backend, "pair_expectation"))  # (device arithmetic only: nothing to reach)
    assert out["expected"].shape == (2, 3, 3) and torch.isnan(out["expected"]).all()


@pytest.mark.parametrize("fn,arg", [(fn, arg) for fn, (tensors, _) in CONTRACT.items() for arg in tensors])
def test_mutated_calls_are_refused_before_the_library(backend, fn, arg):
    from particle_col_image_segmentation_amd import spatial
    dtype, shape = CONTRACT[fn][0][arg]
    other = cc.NEIGHBOURS[dtype][0]
    for kind, value, raises in (("foreign", backend.foreign(dtype, shape), TypeError),
                                ("numpy", np.zeros(shape, cc.NUMPY[dtype]), TypeError),
                                ("dtype", backend.tensor(other, shape), TypeError),
                                ("rank+", backend.tensor(dtype, (1,) + shape), ValueError),
                                ("rank-", backend.tensor(dtype, shape[1:]), ValueError)):
        with pytest.raises(raises) as info:
            getattr(spatial, fn)(**_arguments(backend, fn, **{arg: value}))
        assert info.type is raises, (kind, info.value)
    if fn == "pair_expectation":  # the three arguments are tied to each other
        for bad in ((3,) + shape[1:], shape[:-1] + (shape[-1] + 1,)):
            with pytest.raises(ValueError):
                spatial.pair_expectation(**_arguments(backend, fn, **{arg: backend.tensor(dtype, bad)}))


def test_a_non_contiguous_mask_is_copied_not_refused(backend, monkeypatch):
    from particle_col_image_segmentation_amd import ops, spatial
    seen = []

    def hook(entry, *args, **kwargs):
        seen.append(args[0])
        raise cc.Reached(entry)

    monkeypatch.setattr(ops, "_call", hook)
    mask = backend.strided(torch.uint8, (2, 9, 11))
    mask[1, 2, 3] = 1
    with pytest.raises(cc.Reached):
        spatial.window_pair_counts(mask, E3, 1.0)
    assert seen[0].is_contiguous() and seen[0].data_ptr() != mask.data_ptr() and torch.equal(seen[0], mask)


def test_edges_and_reach_are_refused_before_the_library(backend):
    from particle_col_image_segmentation_amd import spatial
    mask = backend.tensor(torch.uint8, (1, 8, 8))
    for edges in ([0.0], [0.0, 0.0], [0.5, 1.0], [0.0, 2.0, 1.0], [0.0, float("nan")], np.arange(1026.0), None,
                  [0.0, spatial.MAX_REACH + 1.5], [0.0, 1e300]):
        with pytest.raises(ValueError):
            spatial.window_pair_counts(mask, edges, 1.0)
    with pytest.raises(ValueError):
        spatial.window_pair_counts(mask, E3, 0.0)
    with pytest.raises(cc.Reached):
        spatial.window_pair_counts(mask, [0.0, spatial.MAX_REACH + 0.5], 1.0)  # at the limit, far larger than the image


# ------------------------------------------------------------------ the tables
def test_pair_expectation_equals_the_restatement():
    """the float expressions, in their order, on CPU tensors (``ops._on_device`` is not asked on this path's arithmetic)"""
    from particle_col_image_segmentation_amd import ops, spatial
    rng = np.random.default_rng(11)
    B, K, m = 3, 3, 6
    Q = K * (K + 1) // 2
    pair_hist = rng.integers(0, 50, (B, Q, m + 2))
    slot_counts = rng.integers(0, 40, (B, K))
    slot_counts[1] = [0, 1, 2]  # npairs 0 on the diagonal: expected 0 -> NaN
    window = rng.integers(0, 10 ** 9, (B, m + 2))
    window[:, 0] = [28268, 10 ** 6, 0]
    window[0, 2] = 0  # an empty bin: expected 0 -> NaN
    real = ops._on_device
    ops._on_device = lambda t: isinstance(t, torch.Tensor)
    try:
        ex = spatial.pair_expectation(torch.from_numpy(pair_hist), torch.from_numpy(slot_counts), torch.from_numpy(window))
    finally:
        ops._on_device = real
    want = wr.clustering_rows(np.arange(B), np.arange(m + 1.0), pair_hist[:, :, 1:-1], slot_counts, np.zeros((B, K)), window)
    got = np.stack([ex[k].to(torch.float64).numpy().reshape(-1) for k in spatial.CLUSTERING_COLUMNS[10:]], axis=1)
    np.testing.assert_array_equal(got, want[:, 10:])
    assert np.isnan(got[:, 2]).any() and not np.isnan(got[:, 2]).all()


def test_clustering_refuses_bad_arguments_and_names_its_columns():
    from particle_col_image_segmentation_amd import spatial
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    pipe = FramePipeline()
    res = {"shape": (2, 5, 16, 16)}  # every refusal below comes before the result's tensors are touched
    e = [0.0, 1.0, 2.0]
    for bad in (dict(window="disc"), dict(window=""), dict(of="rois"), dict(of="components"), dict(frame_ids=[1]), dict(frame_ids=[1, 2, 3]),
                dict(frame_ids=[[1, 2]])):
        with pytest.raises(ValueError):
            pipe.clustering(res, e, **bad)
    for edges in ([0.0, 0.0], [1.0, 2.0], [0.0, 1e300]):
        with pytest.raises(ValueError):
            pipe.clustering(res, edges, window="frame" if edges[-1] < 10 else "particle")
    with pytest.raises(TypeError):
        pipe.clustering(res, e, window=np.ones((2, 16, 16), np.uint8))
    cols = spatial.clustering_columns(e)
    assert cols["window_pairs"] == ["frame", "n_px", "bin_0", "bin_1", "over"]
    assert cols["clustering"] == ["frame", "slot_a", "slot_b", "bin", "r_lo_um", "r_hi_um", "n_a", "n_b", "n_out_a", "n_out_b", "obs",
                                  "window_pairs", "expected", "ratio", "cum_obs", "cum_window_pairs", "cum_expected", "cum_ratio"]
    assert len(spatial.clustering_columns(np.linspace(0, 3, 1025))["window_pairs"]) == 1024 + 3
