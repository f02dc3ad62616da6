"""CPU checks of the boundary: the C-ABI library loads and exports every symbol include/pcseg.h declares, the
ctypes table covers the header one to one, argument validation fails loudly, and no product module touches oracle/."""
import os
import re

import pytest

from conftest import ROOT


def _header_functions():
    text = open(os.path.join(ROOT, "include", "pcseg.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pcseg_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    from particle_col_image_segmentation_amd import build
    build.build()
    from particle_col_image_segmentation_amd import _lib
    return _lib.load()


def test_library_exports_every_declared_symbol(lib):
    from particle_col_image_segmentation_amd import _lib
    names = _header_functions()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(_lib.SIGNATURES) == names  # the ctypes binding covers the header exactly


def test_workspace_queries_and_argument_errors(lib):
    assert lib.pcseg_version() >= 100
    assert lib.pcseg_ccl_workspace_bytes(2, 64, 64) >= 2 * 64 * 64 * 4
    assert lib.pcseg_edt_workspace_bytes(1, 100, 100) > 0
    assert lib.pcseg_watershed_workspace_bytes(1, 64, 64) >= 64 * 64 * 20
    assert lib.pcseg_ccl_workspace_bytes(0, 64, 64) == 0
    rc = lib.pcseg_median5_u8(None, None, 1, 8, 8, None)
    assert rc == -1 and b"bad arguments" in lib.pcseg_last_error()
    rc = lib.pcseg_watershed4_f32(None, 0, None, None, None, None, 1, 8, 8, 0, None, 0, None)
    assert rc == -1


def test_workspace_table_names_a_query_for_every_entry_that_takes_a_workspace(lib):
    """_lib.WORKSPACE (entry point -> size query) against the signatures: every key is an entry point and every value an
    exported query; no query is left without an entry; and every entry point with a (void *, size_t) pair among its
    arguments is a key, or one of the few that are only ever handed another call's workspace."""
    import ctypes
    from particle_col_image_segmentation_amd import _lib
    queries = {n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes")}
    assert len(_lib.WORKSPACE) >= 40 and set(_lib.WORKSPACE) <= set(_lib.SIGNATURES) - queries
    named = {"pcseg_%s_workspace_bytes" % q for q in _lib.WORKSPACE.values()}
    assert named == queries
    for q in named:
        assert hasattr(lib, q), q
    # (c_size_t and c_uint64 are one ctypes type here, so a (pointer, 64-bit class set) pair looks the same in the argtypes: the
    # header's parameter names tell them apart, and the argtypes must hold the pair wherever the header names one)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pcseg.h")).read(), flags=re.S)
    takes = {m.group(1) for m in re.finditer(r"\b(pcseg_[a-z0-9_]+)\s*\(([^;]*)\)\s*;", text) if "workspace_bytes" in m.group(2)}
    assert takes == set(_lib.WORKSPACE) | set(_lib.WORKSPACE_HANDED_ON)
    pairs = {n for n, (_, args) in _lib.SIGNATURES.items()
             if any(a is ctypes.c_void_p and b is ctypes.c_size_t for a, b in zip(args, args[1:]))}
    assert takes <= pairs and pairs - takes == {"pcseg_region_sums2", "pcseg_region_reduce_sel"}


def test_workspace_size_is_what_the_entry_point_carves(lib):
    """A size query and its entry point run the same carve function: one byte less than the query's answer is refused, with
    PCSEG_ERR_WORKSPACE and the message "<who>: workspace too small (<given> < <needed>)".  Every entry point whose argument
    and workspace checks come before its first device call is listed (the device pointers are never dereferenced; what an
    entry reads on the host -- bin edges, list slots, the input structs -- is real); they are never called with `need` bytes.
    Each is held against the query that _lib.WORKSPACE names for it.  Left out: pcseg_classmap_label_f32, which answers a short
    workspace as an argument error (-1) -- every other entry point that takes a workspace is here (pcseg_table_layout among
    the readers of the head, below)."""
    import ctypes
    from particle_col_image_segmentation_amd import _lib
    ERR_WORKSPACE = -3
    p, q, r = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(12288)
    B, H, W, cap = 2, 96, 80, 16
    shape = (B, H, W)
    pc, npt, K = 64, 100, 2  # pair_cap; points and type slots of the point tables
    edges = (ctypes.c_double * 3)(0.0, 1.0, 2.0)
    slots = (ctypes.c_int32 * 4)(0, 0, 0, 0)

    def inputs(cls):  # a table / refined input struct with every pointer set
        t = cls()
        for name, kind in cls._fields_:
            if kind is ctypes.c_void_p:
                setattr(t, name, 4096)
        t.B, t.cap = B, cap
        return t

    tin, rin = inputs(_lib.TableInputs), inputs(_lib.RefinedInputs)
    tref, rref = ctypes.byref(tin), ctypes.byref(rin)
    cases = [
        (shape, "pcseg_ccl8_equal_u8", lambda ws, n: (p, p, p, B, H, W, ws, n, None)),
        (shape, "pcseg_ccl8_bool", lambda ws, n: (p, p, p, B, H, W, ws, n, None)),
        (shape, "pcseg_ccl4_bool", lambda ws, n: (p, p, p, B, H, W, ws, n, None)),
        (shape, "pcseg_compact_labels", lambda ws, n: (p, q, p, B, H, W, ws, n, None)),
        (shape, "pcseg_dilate_ccl_roots_u8", lambda ws, n: (p, 2, 2, p, B, H, W, ws, n, None)),
        (shape, "pcseg_dilate_ccl_runs_u8", lambda ws, n: (p, 2, 2, p, p, B, H, W, ws, n, None)),
        ((3 * B, H, W), "pcseg_dilate_ccl_runs_multi_u8", lambda ws, n: (p, p, 3, 2, p, p, B, H, W, ws, n, None)),
        (shape, "pcseg_fill_holes", lambda ws, n: (p, p, B, H, W, ws, n, None)),
        (shape, "pcseg_local_maxima_i32", lambda ws, n: (p, p, p, p, B, H, W, ws, n, None)),
        (shape, "pcseg_remove_overlapping", lambda ws, n: (p, p, 0.5, p, B, H, W, ws, n, None)),
        (shape, "pcseg_edt_sq_u8", lambda ws, n: (p, p, B, H, W, -1, ws, n, None)),
        (shape, "pcseg_edt_sq_lt_f32", lambda ws, n: (p, 0, 0.5, p, p, B, H, W, ws, n, None)),
        (shape, "pcseg_dilate_disk_u8", lambda ws, n: (p, 2, 2, q, B, H, W, ws, n, None)),
        (shape, "pcseg_fill_particle", lambda ws, n: (p, q, 1, 2, 3, 2, 2, p, B, H, W, ws, n, None)),
        (shape, "pcseg_watershed4_f32", lambda ws, n: (p, 0, p, p, p, p, B, H, W, 0, ws, n, None)),
        ((B, cap), "pcseg_merge_groups", lambda ws, n: (p, 0, p, p, p, p, p, B, H, W, cap, cap, ws, n, None)),
        ((B, cap), "pcseg_merge_groups_runs", lambda ws, n: (p, p, p, p, p, p, p, B, H, W, cap, cap, ws, n, None)),
        ((B, cap), "pcseg_merge_groups_fused", lambda ws, n: (p, p, p, p, p, 0, 1, p, p, p, B, H, W, cap, ws, n, None)),
        ((3 * B, cap), "pcseg_merge_groups_fused_multi",
         lambda ws, n: (p, p, p, p, p, slots, 3, 1, p, p, p, B, H, W, cap, ws, n, None)),
        # the pair tables: both calls of each, and the merge on the border table
        ((B, pc), "pcseg_territory_pairs", lambda ws, n: (p, p, -1, pc, p, p, p, B, H, W, ws, n, None)),
        ((B, pc), "pcseg_territory_pairs_write", lambda ws, n: (pc, p, None, 0, 0, p, p, p, None, B, ws, n, None)),
        ((B, pc), "pcseg_territory_pairs_write", lambda ws, n: (pc, p, p, cap, 2, p, p, p, p, B, ws, n, None)),
        ((B, pc), "pcseg_label_contingency", lambda ws, n: (p, p, cap, cap, pc, p, p, p, B, H, W, ws, n, None)),
        ((B, pc), "pcseg_contingency_write", lambda ws, n: (pc, p, p, p, p, B, ws, n, None)),
        ((B, pc, cap), "pcseg_label_borders", lambda ws, n: (p, p, H * W, cap, 8, pc, p, p, p, B, H, W, ws, n, None)),
        ((B, pc, cap), "pcseg_label_borders_write", lambda ws, n: (pc, cap, p, p, p, p, p, p, B, ws, n, None)),
        ((B, pc, cap), "pcseg_border_merge", lambda ws, n: (pc, cap, p, 0.5, 0, p, p, p, B, ws, n, None)),
        (shape, "pcseg_nearest_label_i32", lambda ws, n: (p, None, cap, p, p, None, B, H, W, ws, n, None)),
        (shape, "pcseg_reconstruct_i32", lambda ws, n: (p, q, r, p, B, H, W, 8, 0, 0, ws, n, None)),
        (shape, "pcseg_reconstruct_f64", lambda ws, n: (p, q, r, p, B, H, W, 4, 1, 0, ws, n, None)),
        (shape, "pcseg_region_shape", lambda ws, n: (p, p, p, p, B, H, W, cap, ws, n, None)),
        (shape + (cap,), "pcseg_region_hull", lambda ws, n: (p, p, p, p, p, B, H, W, cap, ws, n, None)),
        (shape, "pcseg_thin_labels", lambda ws, n: (p, p, p, B, H, W, -1, ws, n, None)),
        (shape + (cap,), "pcseg_region_skeleton", lambda ws, n: (p, p, p, p, B, H, W, cap, ws, n, None)),
        ((npt, B, K, 3, 4, 0), "pcseg_pair_label_mixing",
         lambda ws, n: (p, p, p, p, npt, B, K, 1.0, edges, 3, 4, 7, p, p, ws, n, None)),
        ((npt, B, K, 3, 4, 1), "pcseg_pair_label_mixing",
         lambda ws, n: (p, p, p, p, npt, B, K, 1.0, edges, 3, 4, 7, None, p, ws, n, None)),
        ((npt, B, K, 0), "pcseg_point_neighbours",
         lambda ws, n: (p, p, p, p, npt, B, K, 1.0, None, 0, p, p, None, ws, n, None)),
        ((npt, B, K, 3), "pcseg_point_neighbours",
         lambda ws, n: (p, p, p, p, npt, B, K, 1.0, edges, 3, p, p, p, ws, n, None)),
        (shape, "pcseg_surface_points", lambda ws, n: (p, 2, p, p, p, p, None, 0, B, H, W, ws, n, None)),
        (shape, "pcseg_surface_distances",
         lambda ws, n: (p, None, p, npt, p, p, None, B, H, W, 1.0, None, 0, 0, p, p, None, None, None, ws, n, None)),
        (shape, "pcseg_surface_shells", lambda ws, n: (p, p, p, B, H, W, 1.0, edges, 3, p, ws, n, None)),
        (shape + (cap,), "pcseg_label_parent",
         lambda ws, n: (p, p, p, None, None, p, p, p, None, p, None, B, H, W, cap, ws, n, None)),
        ((B, cap), "pcseg_table_write", lambda ws, n: (tref, p, p, p, p, ws, n, None)),
        ((B, cap), "pcseg_refined_layout", lambda ws, n: (rref, p, ws, n, None)),
        ((B, cap), "pcseg_refined_table_write", lambda ws, n: (rref, p, 1 << 20, p, p, p, None, None, None, None, ws, n, None)),
    ]
    assert {entry for _, entry, _ in cases} == set(_lib.WORKSPACE) - {"pcseg_classmap_label_f32", "pcseg_table_layout"}
    for qargs, entry, args in cases:
        query = _lib.WORKSPACE[entry]
        need = getattr(lib, "pcseg_%s_workspace_bytes" % query)(*qargs)
        assert need > 0 and need % 256 == 0, (query, need)
        assert entry in _lib.SIGNATURES
        rc = getattr(lib, entry)(*args(p, need - 1))
        assert rc == ERR_WORKSPACE, (entry, rc, lib.pcseg_last_error())
        assert lib.pcseg_last_error().endswith(b": workspace too small (%d < %d)" % (need - 1, need)), (entry, lib.pcseg_last_error())
    # the readers of a table workspace's head (the frames' row counts and offsets: two 256-byte aligned regions of 3 B int64,
    # what pcseg_table_layout writes) carve the head alone; no size query answers it
    head = 2 * ((3 * 8 * B + 255) // 256 * 256)
    class_slot = (ctypes.c_uint8 * 256)()
    for entry, who, args in [
        ("pcseg_table_layout", "table_layout", lambda ws, n: (tref, p, ws, n, None)),
        ("pcseg_cell_distances", "cell_distances", lambda ws, n: (p, 10, 14, class_slot, 19.0, 1.0, p, B, ws, n, None)),
        ("pcseg_neighbours_pack_cells", "neighbours_pack_cells", lambda ws, n: (p, 14, class_slot, B, ws, n, p, p, p, p, None)),
        ("pcseg_surface_pack_cells", "surface_pack_cells", lambda ws, n: (p, 14, class_slot, B, ws, n, p, p, p, p, None)),
        ("pcseg_refined_table_write", "refined_table_write",
         lambda ws, n: (rref, ws, n, p, p, p, None, None, None, None, p, 1 << 20, None)),
    ]:
        rc = getattr(lib, entry)(*args(p, head - 1))
        assert rc == ERR_WORKSPACE, (entry, rc, lib.pcseg_last_error())
        assert lib.pcseg_last_error() == ("%s: workspace too small (%d < %d)" % (who, head - 1, head)).encode(), (entry, lib.pcseg_last_error())
    # a null workspace is refused as an argument, whatever its stated size
    assert lib.pcseg_fill_holes(p, p, B, H, W, None, 1 << 30, None) == -1
    # shapes a size query rejects
    for name in ("ccl", "dilate_ccl", "dilate_ccl_runs", "fill_holes", "local_maxima", "overlap", "classmap_label", "edt", "watershed"):
        f = getattr(lib, "pcseg_%s_workspace_bytes" % name)
        assert f(0, 8, 8) == 0 and f(1, 0, 8) == 0 and f(1, 8, 0) == 0, name
    for name in ("merge_groups", "table", "refined"):
        f = getattr(lib, "pcseg_%s_workspace_bytes" % name)
        assert f(0, 4) == 0 and f(2, 0) == 0, name


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import numpy as np
    from particle_col_image_segmentation_amd import tiff_analysis as ta
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ta.median_filter(np.ones((8, 8), np.uint8))


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "particle_col_image_segmentation_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in text.replace("oracle interpreter", ""), os.path.join(dirpath, f)
