"""CPU checks of the refined-cell tables (refine_boundaries.py:1-12, goal 2): column schemas, the empty tables, the host
epilogue and the gather's sort of the new tables, and argument rejection by the new C exports (no device is touched)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

CT3 = {1: "3D05", 2: "6B07", 3: "Particle", 4: "C3M10", 5: "Background"}
REFINED = ["frame", "label", "parent", "parent_px", "n_overlap", "class", "kind", "cells", "area", "centroid_row",
           "centroid_col"]
RESOLUTION = ["frame", "label", "children", "resolved", "cells_integrated"]


@pytest.fixture(scope="module")
def lib():
    from particle_col_image_segmentation_amd import build
    build.build()
    from particle_col_image_segmentation_amd import _lib
    return _lib.load()


def _pipe(ct=None):
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    return FramePipeline(ct)


def _frames_refined(names):
    return ["frame", "refined_nan_flag"] + [c % n for n in names for c in ("%s_refined_cells", "%s_refined_clusters",
                                                                          "%s_resolved", "%s_residual", "%s_count_integrated")]


@pytest.mark.parametrize("three", [False, True])
def test_table_columns_with_refined(three):
    pipe = _pipe(CT3 if three else None)
    names = ["3D05", "6B07", "C3M10"] if three else ["3D05", "6B07"]
    edges = [0.0, 1.0, 2.5]
    base = pipe.table_columns(5)
    cols = pipe.table_columns(5, refined=True)
    assert set(cols) == set(base) | {"refined", "cell_resolution", "frames_refined"}
    for k in base:
        assert cols[k] == base[k]
    assert cols["refined"] == REFINED and cols["cell_resolution"] == RESOLUTION
    assert cols["frames_refined"] == _frames_refined(names)
    full = pipe.table_columns(5, neighbours=True, pair_edges=edges, refined=True)
    assert full["refined_neighbours"] == full["neighbours"] and full["refined_pair_hist"] == full["pair_hist"]
    only_nb = pipe.table_columns(5, neighbours=True, refined=True)
    assert "refined_neighbours" in only_nb and "refined_pair_hist" not in only_nb
    only_e = pipe.table_columns(5, pair_edges=edges, refined=True)
    assert "refined_pair_hist" in only_e and "refined_neighbours" not in only_e
    assert not any(k.startswith("refined") for k in pipe.table_columns(5, neighbours=True, pair_edges=edges))


def test_empty_device_tables_carry_the_refined_tables():
    pipe = _pipe(CT3)
    dt = pipe.empty_device_tables(5, device="cpu", refined=True, neighbours=True, pair_edges=[0.0, 1.0, 2.0])
    assert dt["refined"].shape == (0, 11) and dt["cell_resolution"].shape == (0, 5)
    assert dt["frames_refined"].shape == (0, 2 + 5 * 3)
    assert dt["refined_neighbours"].shape == (0, 9) and dt["refined_pair_hist"].shape == (0, 7)
    assert set(pipe.empty_device_tables(5, device="cpu")) == {"rois", "cells", "groups", "frames_rec", "distances"}


def test_host_tables_carry_the_refined_tables():
    pipe = _pipe()
    C, e = 5, [0.0, 1.0, 2.0]
    cols = pipe.table_columns(C, neighbours=True, pair_edges=e, refined=True)
    z = lambda k, n: torch.zeros((n, len(cols[k])), dtype=torch.float64)
    ar = lambda k, n: torch.arange(n * len(cols[k]), dtype=torch.float64).reshape(n, len(cols[k]))
    dt = {"rois": z("rois", 3), "cells": z("cells", 2), "groups": z("groups", 0),
          "frames_rec": torch.zeros((1, 18), dtype=torch.float64), "distances": torch.zeros((0, 3), dtype=torch.float64),
          "neighbours": ar("neighbours", 2), "pair_hist": ar("pair_hist", 3), "refined": ar("refined", 3),
          "cell_resolution": ar("cell_resolution", 2), "frames_refined": ar("frames_refined", 1),
          "refined_neighbours": ar("refined_neighbours", 4), "refined_pair_hist": ar("refined_pair_hist", 3)}
    out = pipe.host_tables(dt, C, neighbours=True, pair_edges=e, refined=True)
    for k in ("refined", "cell_resolution", "frames_refined", "refined_neighbours", "refined_pair_hist"):
        np.testing.assert_array_equal(out[k], dt[k].numpy())
        assert out[k + "_columns"] == cols[k]
    plain = pipe.host_tables({k: v for k, v in dt.items() if not k.startswith(("refined", "cell_res", "frames_ref"))}, C)
    assert not any(k.startswith(("refined", "cell_resolution", "frames_refined")) for k in plain)
    with pytest.raises(ValueError):
        pipe.host_tables({k: v for k, v in dt.items() if k != "cell_resolution"}, C, refined=True)


def test_gather_tables_sorts_refined_pair_hist():
    from particle_col_image_segmentation_amd.distributed import _SORT_COLS, TABLE_KEYS, gather_tables
    assert _SORT_COLS["refined_pair_hist"] == (0, 1, 2)
    assert TABLE_KEYS == ("cells", "rois", "frames", "groups", "distances")
    rng = np.random.default_rng(5)
    rows = np.array([(f, a, b) for f in range(5) for a in range(3) for b in range(a, 3)], np.float64)
    table = np.concatenate([rows, rng.integers(0, 100, (rows.shape[0], 4)).astype(np.float64)], axis=1)
    refined = np.array([(f, l) for f in range(3) for l in range(1, 6)], np.float64)
    refined = np.concatenate([refined, rng.integers(0, 9, (refined.shape[0], 9)).astype(np.float64)], axis=1)
    out = gather_tables({"refined_pair_hist": table[rng.permutation(table.shape[0])],
                         "refined": refined[rng.permutation(refined.shape[0])]})
    np.testing.assert_array_equal(out["refined_pair_hist"], table)
    np.testing.assert_array_equal(out["refined"], refined)


def test_label_parent_rejects_bad_arguments(lib):
    p = ctypes.c_void_p(4096)  # never dereferenced: the arguments are rejected first
    z = ctypes.c_void_p(0)

    def call(B=2, H=8, W=8, cap=4, null=None, nbytes=1 << 20):
        args = [p] * 11
        if null is not None:
            args[null] = z
        return lib.pcseg_label_parent(*args, B, H, W, cap, p, nbytes, None)

    for kw in (dict(B=0), dict(B=-1), dict(cap=0), dict(cap=-3), dict(H=0), dict(W=0), dict(null=0), dict(null=1),
               dict(null=2), dict(null=5), dict(null=6), dict(null=7), dict(null=9)):
        assert call(**kw) == -1 and b"bad arguments" in lib.pcseg_last_error(), kw
    assert lib.pcseg_label_parent_workspace_bytes(0, 8, 8, 4) == 0
    assert lib.pcseg_label_parent_workspace_bytes(2, 8, 8, 0) == 0
    need = lib.pcseg_label_parent_workspace_bytes(2, 8, 8, 4)
    assert need >= 2 * 4 * (8 * 4 + 4 + 4)
    rc = call(nbytes=need - 1)
    assert rc != 0 and b"workspace too small" in lib.pcseg_last_error()


def test_refined_table_exports_reject_bad_arguments(lib):
    from particle_col_image_segmentation_amd import _lib
    p = ctypes.c_void_p(4096)
    ri = _lib.RefinedInputs()
    for name, _ in _lib.RefinedInputs._fields_[3:]:
        setattr(ri, name, 4096)
    ri.B, ri.cap, ri.n_slots = 2, 16, 2
    assert lib.pcseg_refined_workspace_bytes(0, 16) == 0 and lib.pcseg_refined_workspace_bytes(2, 0) == 0
    need = lib.pcseg_refined_workspace_bytes(2, 16)
    assert need >= 3 * 4 * 2 * 16
    for bad in (dict(B=0), dict(cap=0), dict(n_slots=5), dict(n_slots=-1), dict(parent=None), dict(kind_r=None),
                dict(ws_stats=None)):
        r = _lib.RefinedInputs()
        ctypes.pointer(r)[0] = ri
        for k, v in bad.items():
            setattr(r, k, v)
        assert lib.pcseg_refined_layout(ctypes.byref(r), p, p, need, None) == -1, bad
        assert b"bad arguments" in lib.pcseg_last_error()
        assert lib.pcseg_refined_table_write(ctypes.byref(r), p, 1 << 20, p, p, p, None, None, None, None, p, need, None) == -1
    assert lib.pcseg_refined_layout(None, p, p, need, None) == -1
    assert lib.pcseg_refined_layout(ctypes.byref(ri), p, p, need - 1, None) != 0
    assert b"workspace too small" in lib.pcseg_last_error()
    # the points come all together or not at all; null outputs are refused
    assert lib.pcseg_refined_table_write(ctypes.byref(ri), p, 1 << 20, p, p, p, p, None, p, p, p, need, None) == -1
    assert lib.pcseg_refined_table_write(ctypes.byref(ri), p, 1 << 20, None, p, p, None, None, None, None, p, need, None) == -1
    assert lib.pcseg_refined_table_write(ctypes.byref(ri), None, 0, p, p, p, None, None, None, None, p, need, None) == -1
    assert lib.pcseg_refined_table_write(ctypes.byref(ri), p, 8, p, p, p, None, None, None, None, p, need, None) != 0
