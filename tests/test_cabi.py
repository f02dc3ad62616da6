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


def test_workspace_size_is_what_the_entry_point_carves(lib):
    """A size query and its entry point run the same carve function: one byte less than the query's answer is refused.
    Only entry points whose argument and workspace checks come before their first device call are listed (the pointers are
    never dereferenced); they are never called with `need` bytes."""
    import ctypes
    from particle_col_image_segmentation_amd import _lib
    ERR_WORKSPACE = -3
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    B, H, W, cap = 2, 96, 80, 16
    shape = (B, H, W)
    cases = [
        ("ccl", shape, "pcseg_ccl8_equal_u8", lambda ws, n: (p, p, p, B, H, W, ws, n, None)),
        ("ccl", shape, "pcseg_ccl8_bool", lambda ws, n: (p, p, p, B, H, W, ws, n, None)),
        ("ccl", shape, "pcseg_ccl4_bool", lambda ws, n: (p, p, p, B, H, W, ws, n, None)),
        ("ccl", shape, "pcseg_compact_labels", lambda ws, n: (p, q, p, B, H, W, ws, n, None)),
        ("dilate_ccl", shape, "pcseg_dilate_ccl_roots_u8", lambda ws, n: (p, 2, 2, p, B, H, W, ws, n, None)),
        ("dilate_ccl_runs", shape, "pcseg_dilate_ccl_runs_u8", lambda ws, n: (p, 2, 2, p, p, B, H, W, ws, n, None)),
        ("dilate_ccl_runs", (3 * B, H, W), "pcseg_dilate_ccl_runs_multi_u8", lambda ws, n: (p, p, 3, 2, p, p, B, H, W, ws, n, None)),
        ("fill_holes", shape, "pcseg_fill_holes", lambda ws, n: (p, p, B, H, W, ws, n, None)),
        ("local_maxima", shape, "pcseg_local_maxima_i32", lambda ws, n: (p, p, p, p, B, H, W, ws, n, None)),
        ("overlap", shape, "pcseg_remove_overlapping", lambda ws, n: (p, p, 0.5, p, B, H, W, ws, n, None)),
        ("edt", shape, "pcseg_edt_sq_u8", lambda ws, n: (p, p, B, H, W, -1, ws, n, None)),
        ("edt", shape, "pcseg_edt_sq_lt_f32", lambda ws, n: (p, 0, 0.5, p, p, B, H, W, ws, n, None)),
        ("edt", shape, "pcseg_dilate_disk_u8", lambda ws, n: (p, 2, 2, q, B, H, W, ws, n, None)),
        ("edt", shape, "pcseg_fill_particle", lambda ws, n: (p, q, 1, 2, 3, 2, 2, p, B, H, W, ws, n, None)),
        ("watershed", shape, "pcseg_watershed4_f32", lambda ws, n: (p, 0, p, p, p, p, B, H, W, 0, ws, n, None)),
        ("merge_groups", (B, cap), "pcseg_merge_groups", lambda ws, n: (p, 0, p, p, p, p, p, B, H, W, cap, cap, ws, n, None)),
        ("merge_groups", (B, cap), "pcseg_merge_groups_runs", lambda ws, n: (p, p, p, p, p, p, p, B, H, W, cap, cap, ws, n, None)),
    ]
    for query, qargs, entry, args in cases:
        need = getattr(lib, "pcseg_%s_workspace_bytes" % query)(*qargs)
        assert need > 0 and need % 256 == 0, (query, need)
        assert entry in _lib.SIGNATURES
        rc = getattr(lib, entry)(*args(p, need - 1))
        assert rc == ERR_WORKSPACE and b"workspace too small" in lib.pcseg_last_error(), (entry, rc, lib.pcseg_last_error())
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
