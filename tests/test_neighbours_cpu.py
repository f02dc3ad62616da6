"""CPU checks of the per-strain neighbour tables (refine_boundaries.py:8-12, goal 3): column schemas, the host epilogue
and the gather's sort of the new tables, and argument rejection by the new C exports (no device is touched)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

CT3 = {1: "3D05", 2: "6B07", 3: "Particle", 4: "C3M10", 5: "Background"}


@pytest.fixture(scope="module")
def lib():
    from particle_col_image_segmentation_amd import build
    build.build()
    from particle_col_image_segmentation_amd import _lib
    return _lib.load()


def _pipe(ct=None):
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    return FramePipeline(ct)


def test_table_columns_for_two_and_three_strains():
    edges = [0.0, 1.0, 2.5, 4.0]
    two = _pipe().table_columns(5, neighbours=True, pair_edges=edges)
    assert two["neighbours"] == ["frame", "label", "slot", "nn_um_3D05", "nn_um_6B07", "nn_label_3D05", "nn_label_6B07"]
    assert two["pair_hist"] == ["frame", "slot_a", "slot_b", "n_pairs", "bin_0", "bin_1", "bin_2", "over"]
    three = _pipe(CT3).table_columns(5, neighbours=True, pair_edges=np.linspace(0, 10, 65))
    assert three["neighbours"][3:] == ["nn_um_3D05", "nn_um_6B07", "nn_um_C3M10", "nn_label_3D05", "nn_label_6B07",
                                       "nn_label_C3M10"]
    assert len(three["pair_hist"]) == 4 + 64 + 1
    # without the keywords: the schema of the tables that existed before
    assert set(_pipe().table_columns(5)) == {"cells", "rois", "frames", "distances", "groups"}
    assert "pair_hist" not in _pipe().table_columns(5, neighbours=True)
    assert "neighbours" not in _pipe().table_columns(5, pair_edges=edges)


def test_empty_device_tables_carry_the_new_tables():
    pipe = _pipe(CT3)
    e = [0.0, 1.0, 2.0]
    dt = pipe.empty_device_tables(5, device="cpu", neighbours=True, pair_edges=e)
    assert dt["neighbours"].shape == (0, 9) and dt["pair_hist"].shape == (0, 4 + 2 + 1)
    assert set(pipe.empty_device_tables(5, device="cpu")) == {"rois", "cells", "groups", "frames_rec", "distances"}


def test_host_tables_carry_neighbours_and_pair_hist():
    pipe = _pipe()
    C, e = 5, [0.0, 1.0, 2.0, 3.0]
    cols = pipe.table_columns(C, neighbours=True, pair_edges=e)
    z = lambda k, n: torch.zeros((n, len(cols[k])), dtype=torch.float64)
    nb = torch.arange(2 * 7, dtype=torch.float64).reshape(2, 7)
    ph = torch.arange(3 * 8, dtype=torch.float64).reshape(3, 8)
    dt = {"rois": z("rois", 0), "cells": z("cells", 2), "groups": z("groups", 0),
          "frames_rec": torch.zeros((1, 18), dtype=torch.float64), "distances": torch.zeros((0, 3), dtype=torch.float64),
          "neighbours": nb, "pair_hist": ph}
    out = pipe.host_tables(dt, C, neighbours=True, pair_edges=e)
    np.testing.assert_array_equal(out["neighbours"], nb.numpy())
    np.testing.assert_array_equal(out["pair_hist"], ph.numpy())
    assert out["neighbours_columns"] == cols["neighbours"] and out["pair_hist_columns"] == cols["pair_hist"]
    plain = pipe.host_tables({k: v for k, v in dt.items() if k not in ("neighbours", "pair_hist")}, C)
    assert "neighbours" not in plain and "pair_hist" not in plain and "pair_hist_columns" not in plain
    with pytest.raises(ValueError):
        pipe.host_tables({k: v for k, v in dt.items() if k != "pair_hist"}, C, pair_edges=e)


def test_gather_tables_sorts_pair_hist_by_frame_and_slot_pair():
    from particle_col_image_segmentation_amd.distributed import _SORT_COLS, TABLE_KEYS, gather_tables
    assert _SORT_COLS["pair_hist"] == (0, 1, 2)
    assert TABLE_KEYS == ("cells", "rois", "frames", "groups", "distances")
    rng = np.random.default_rng(3)
    rows = np.array([(f, a, b) for f in range(4) for a in range(3) for b in range(a, 3)], np.float64)
    table = np.concatenate([rows, rng.integers(0, 100, (rows.shape[0], 5)).astype(np.float64)], axis=1)
    out = gather_tables({"pair_hist": table[rng.permutation(table.shape[0])]})
    np.testing.assert_array_equal(out["pair_hist"], table)


def _nb_call(lib, K=2, scale=1.0, edges=None, n_edges=None, null=False, hist=True):
    p = ctypes.c_void_p(0 if null else 4096)  # never dereferenced: the arguments are rejected first
    e = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64)
    ep = ctypes.c_void_p(e.ctypes.data) if e is not None else ctypes.c_void_p(0)
    ne = (0 if e is None else e.shape[0]) if n_edges is None else n_edges
    hp = p if (hist and e is not None) else ctypes.c_void_p(0)
    return lib.pcseg_point_neighbours(p, p, p, p, 10, 1, K, scale, ep, ne, p, p, hp, p, 1 << 20, None)


def test_point_neighbours_rejects_bad_arguments(lib):
    ok = [0.0, 1.0, 2.0]
    checks = [dict(null=True), dict(K=5), dict(K=0), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")),
              dict(edges=[0.5, 1.0, 2.0]), dict(edges=[0.0, 2.0, 1.0]), dict(edges=[0.0, 1.0, 1.0]),
              dict(edges=[0.0]), dict(edges=np.linspace(0, 1, 1026)), dict(edges=[0.0, float("inf")]),
              dict(edges=ok, hist=False), dict(edges=ok, n_edges=0)]
    for kw in checks:
        rc = _nb_call(lib, **kw)
        assert rc == -1 and b"bad arguments" in lib.pcseg_last_error(), kw
    assert lib.pcseg_neighbours_workspace_bytes(1000, 2, 5, 0) == 0
    assert lib.pcseg_neighbours_workspace_bytes(1000, 2, 3, 65) >= 1000 * (16 + 4 + 4 + 3 * 12)
    rc = lib.pcseg_neighbours_pack_cells(None, 20, None, 1, None, 0, None, None, None, None, None)
    assert rc == -1 and b"bad arguments" in lib.pcseg_last_error()
