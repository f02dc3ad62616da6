"""CPU checks of the surface-distance tables (HCN_nanosims_rois_activity_distance_5iso_YG.m:271-309): column schemas,
the empty tables and the host epilogue, the gather's sort keys, argument rejection by every new C export (rejection
happens before any launch, so no device is touched) and the host-only integer thresholds of the shell histogram
against numpy for every squared distance a frame can hold."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")

CT3 = {1: "3D05", 2: "6B07", 3: "Particle", 4: "C3M10", 5: "Background"}
NEW = ("surface", "frames_surface", "surface_hist", "surface_shells", "refined_surface", "refined_surface_hist")
OLD = {"cells", "rois", "frames", "distances", "groups"}


@pytest.fixture(scope="module")
def lib():
    from particle_col_image_segmentation_amd import build
    build.build()
    from particle_col_image_segmentation_amd import _lib
    return _lib.load()


def _pipe(ct=None):
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    return FramePipeline(ct)


@pytest.mark.parametrize("three", [False, True])
def test_table_columns_with_surface(three):
    pipe = _pipe(CT3 if three else None)
    e = [0.0, 1.0, 2.5, 4.0]
    row = ["frame", "label", "slot", "inside", "surface_um", "nearest_row", "nearest_col"]
    assert set(pipe.table_columns(5)) == OLD  # without the keywords: exactly the tables that existed before
    cols = pipe.table_columns(5, surface=True)
    assert set(cols) == OLD | {"surface", "frames_surface"}
    assert cols["surface"] == row and cols["frames_surface"] == ["frame", "surface_px", "filled_area"]
    cols = pipe.table_columns(5, surface=True, surface_edges=e)
    assert set(cols) == OLD | {"surface", "frames_surface", "surface_hist", "surface_shells"}
    assert cols["surface_hist"] == ["frame", "side", "slot", "n", "bin_0", "bin_1", "bin_2", "over"]
    assert cols["surface_shells"] == ["frame", "side", "n_px", "bin_0", "bin_1", "bin_2", "over"]
    assert set(pipe.table_columns(5, surface_edges=e)) == OLD | {"surface_hist", "surface_shells"}
    cols = pipe.table_columns(5, refined=True, surface=True, surface_edges=np.linspace(0, 8, 33))
    assert set(cols) == OLD | {"refined", "cell_resolution", "frames_refined"} | set(NEW)
    assert cols["refined_surface"] == row and cols["refined_surface_hist"] == cols["surface_hist"]
    assert len(cols["surface_hist"]) == 4 + 32 + 1 and len(cols["surface_shells"]) == 3 + 32 + 1
    assert not set(pipe.table_columns(5, refined=True, neighbours=True, pair_edges=e)) & set(NEW)


def test_empty_device_tables_carry_the_surface_tables():
    pipe = _pipe(CT3)
    e = [0.0, 1.0, 2.0]
    dt = pipe.empty_device_tables(5, device="cpu", surface=True, surface_edges=e, refined=True)
    assert dt["surface"].shape == (0, 7) and dt["frames_surface"].shape == (0, 3) and dt["refined_surface"].shape == (0, 7)
    assert dt["surface_hist"].shape == (0, 7) and dt["surface_shells"].shape == (0, 6) and dt["refined_surface_hist"].shape == (0, 7)
    assert set(pipe.empty_device_tables(5, device="cpu")) == {"rois", "cells", "groups", "frames_rec", "distances"}


def test_host_tables_carry_the_surface_tables():
    pipe = _pipe()
    C, e = 5, [0.0, 1.0, 2.0, 3.0]
    cols = pipe.table_columns(C, surface=True, surface_edges=e)
    z = lambda k, n: torch.zeros((n, len(cols[k])), dtype=torch.float64)
    base = {"rois": z("rois", 0), "cells": z("cells", 2), "groups": z("groups", 0),
            "frames_rec": torch.zeros((1, 18), dtype=torch.float64), "distances": torch.zeros((0, 3), dtype=torch.float64)}
    new = {k: torch.arange(float((i + 2) * len(cols[k])), dtype=torch.float64).reshape(i + 2, len(cols[k]))
           for i, k in enumerate(("surface", "frames_surface", "surface_hist", "surface_shells"))}
    out = pipe.host_tables({**base, **new}, C, surface=True, surface_edges=e)
    for k, v in new.items():
        np.testing.assert_array_equal(out[k], v.numpy())
        assert out[k + "_columns"] == cols[k]
    with pytest.raises(ValueError, match="surface"):  # a dict made without the tables is rejected, not padded
        pipe.host_tables(base, C, surface=True)
    with pytest.raises(ValueError, match="surface_hist"):
        pipe.host_tables({**base, "surface": new["surface"], "frames_surface": new["frames_surface"]}, C, surface=True,
                         surface_edges=e)
    assert not set(pipe.host_tables(base, C)) & set(NEW)


def test_lexsort_keys_of_the_surface_tables():
    from particle_col_image_segmentation_amd.distributed import _SORT_COLS, _lexsort_rows, gather_tables
    keys = {k: _SORT_COLS.get(k, (0, 1)) for k in NEW}
    assert keys == {"surface": (0, 1), "frames_surface": (0,), "surface_hist": (0, 1, 2), "surface_shells": (0, 1),
                    "refined_surface": (0, 1), "refined_surface_hist": (0, 1, 2)}
    rng = np.random.default_rng(3)
    rows = np.array([(f, s, t, rng.integers(0, 9)) for f in range(4) for s in range(2) for t in range(3)], np.float64)
    shuffled = rows[rng.permutation(len(rows))]
    np.testing.assert_array_equal(_lexsort_rows(torch.from_numpy(shuffled), (0, 1, 2)).numpy(), rows)
    out = gather_tables({"surface_hist": shuffled, "surface_shells": shuffled[:, [0, 1, 3]][shuffled[:, 2] == 0]})
    np.testing.assert_array_equal(out["surface_hist"], rows)
    np.testing.assert_array_equal(out["surface_shells"], rows[rows[:, 2] == 0][:, [0, 1, 3]])


def _gloo_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    from particle_col_image_segmentation_amd.distributed import gather_tables
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        frames = list(range(rank, 5, world))  # round-robin ownership, as run_sharded shards
        hist = np.array([(f, s, t, 100 * f + 10 * s + t) for f in frames for s in range(2) for t in range(2)], np.float64)
        shells = np.array([(f, s, 7 * f + s) for f in frames for s in range(2)], np.float64)
        surf = np.array([(f, l, 0, 1, 0.5 * l, f, l) for f in frames for l in (1, 2, 5)], np.float64)
        fs = np.array([(f, 10 + f, 20 + f) for f in frames], np.float64)
        out = gather_tables({"surface_hist": hist.reshape(-1, 4), "surface_shells": shells.reshape(-1, 3),
                             "surface": surf.reshape(-1, 7), "frames_surface": fs.reshape(-1, 3)})
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
    finally:
        dist.destroy_process_group()


def test_gloo_world_of_two_sorts_the_surface_tables(tmp_path):
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_gloo_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a, b = (np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(2))
    frames = range(5)
    want = {"surface_hist": np.array([(f, s, t, 100 * f + 10 * s + t) for f in frames for s in range(2) for t in range(2)], np.float64),
            "surface_shells": np.array([(f, s, 7 * f + s) for f in frames for s in range(2)], np.float64),
            "surface": np.array([(f, l, 0, 1, 0.5 * l, f, l) for f in frames for l in (1, 2, 5)], np.float64),
            "frames_surface": np.array([(f, 10 + f, 20 + f) for f in frames], np.float64)}
    for k, v in want.items():
        np.testing.assert_array_equal(a[k], v, err_msg=k)
        np.testing.assert_array_equal(b[k], v, err_msg=k)


def _rejected(lib, rc, code=-1):
    assert rc == code, (rc, lib.pcseg_last_error())
    assert lib.pcseg_last_error()


def test_surface_exports_reject_bad_arguments(lib):
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is rejected before any launch
    null = ctypes.c_void_p(0)
    assert lib.pcseg_surface_workspace_bytes(2, 64, 70) >= 2 * 64 * 3 * 4 and lib.pcseg_surface_workspace_bytes(0, 64, 64) == 0
    assert lib.pcseg_surface_shells_workspace_bytes(2, 64, 70) >= 2 * 64 * 70 * 5 and lib.pcseg_surface_shells_workspace_bytes(1, 0, 4) == 0
    big = 1 << 30
    # ---- surface_points
    pts = lambda **k: lib.pcseg_surface_points(k.get("x", p), 2, k.get("bits", p), k.get("counts", p), k.get("offsets", p), p,
                                               k.get("points", null), k.get("cap", 0), k.get("B", 1), k.get("H", 8), k.get("W", 8),
                                               k.get("ws", p), k.get("nbytes", big), None)
    for bad in (dict(x=null), dict(bits=null), dict(counts=null), dict(offsets=null), dict(ws=null), dict(B=0), dict(H=0), dict(W=-1),
                dict(cap=5), dict(points=p, cap=-1)):
        _rejected(lib, pts(**bad))
    _rejected(lib, pts(nbytes=16), -3)
    # ---- surface_distances
    e = (ctypes.c_double * 3)(0.0, 1.0, 2.0)

    def dst(**k):
        edges = k.get("edges", null)
        return lib.pcseg_surface_distances(k.get("rc", p), k.get("slot", null), k.get("foff", p), k.get("n", 4), k.get("bits", p), null,
                                           k.get("mask", null), k.get("B", 1), k.get("H", 8), k.get("W", 8), k.get("scale", 1.0),
                                           edges, k.get("n_edges", 0), k.get("K", 2), k.get("dist", p), k.get("near", p), null,
                                           k.get("hist", null), null, k.get("ws", p), k.get("nbytes", big), None)

    for bad in (dict(rc=null), dict(foff=null), dict(bits=null), dict(dist=null), dict(near=null), dict(ws=null), dict(n=-1), dict(B=0),
                dict(H=0), dict(W=0), dict(scale=0.0), dict(scale=float("nan")), dict(hist=p), dict(edges=e), dict(n_edges=3)):
        _rejected(lib, dst(**bad))
    full = dict(edges=e, n_edges=3, hist=p, slot=p, mask=p)
    for bad in (dict(slot=null), dict(mask=null), dict(hist=null), dict(K=0), dict(K=5), dict(n_edges=1), dict(n_edges=1026),
                dict(edges=(ctypes.c_double * 3)(0.5, 1.0, 2.0)), dict(edges=(ctypes.c_double * 3)(0.0, 1.0, 1.0)),
                dict(edges=(ctypes.c_double * 3)(0.0, 2.0, 1.0)), dict(edges=(ctypes.c_double * 3)(0.0, 1.0, float("inf")))):
        _rejected(lib, dst(**{**full, **bad}))
    _rejected(lib, dst(nbytes=16), -3)
    # ---- surface_shells
    shl = lambda **k: lib.pcseg_surface_shells(k.get("bits", p), k.get("counts", p), k.get("mask", p), k.get("B", 1), k.get("H", 8),
                                               k.get("W", 8), k.get("scale", 1.0), k.get("edges", e), k.get("n_edges", 3),
                                               k.get("shells", p), k.get("ws", p), k.get("nbytes", big), None)
    many = (ctypes.c_double * 1026)(*np.arange(1026.0))
    for bad in (dict(bits=null), dict(counts=null), dict(mask=null), dict(shells=null), dict(ws=null), dict(B=0), dict(B=70000), dict(H=0),
                dict(W=0), dict(scale=-1.0), dict(edges=null), dict(n_edges=1), dict(edges=many, n_edges=1026),
                dict(edges=(ctypes.c_double * 3)(1.0, 2.0, 3.0)), dict(edges=(ctypes.c_double * 3)(0.0, 0.0, 1.0))):
        _rejected(lib, shl(**bad))
    _rejected(lib, shl(nbytes=16), -3)
    # ---- thresholds (host only)
    out = (ctypes.c_int64 * 4)()
    for bad in ((null, 3, 1.0, out), (e, 3, 1.0, null), (e, 1, 1.0, out), (e, 3, 0.0, out), (e, 3, float("inf"), out),
                ((ctypes.c_double * 3)(0.0, 2.0, 2.0), 3, 1.0, out), ((ctypes.c_double * 3)(0.1, 2.0, 3.0), 3, 1.0, out),
                (many, 1026, 1.0, out)):
        _rejected(lib, lib.pcseg_surface_thresholds(*bad))
    # ---- the pack exports
    slots = (ctypes.c_uint8 * 256)()
    pk = lambda **k: lib.pcseg_surface_pack_cells(k.get("cells", p), k.get("ncol", 21), k.get("slots", slots), k.get("B", 1), k.get("tws", p),
                                                  k.get("nbytes", big), k.get("rc", p), k.get("slot", p), k.get("id", p), k.get("foff", p), None)
    for bad in (dict(cells=null), dict(slots=None), dict(tws=null), dict(rc=null), dict(slot=null), dict(id=null), dict(foff=null),
                dict(B=0), dict(ncol=13)):
        _rejected(lib, pk(**bad))
    _rejected(lib, pk(nbytes=8), -3)
    pr = lambda **k: lib.pcseg_surface_pack_refined(k.get("st", p), k.get("cap", 16), k.get("id", p), k.get("foff", p), k.get("n", 3),
                                                    k.get("B", 1), k.get("rc", p), None)
    for bad in (dict(st=null), dict(id=null), dict(foff=null), dict(rc=null), dict(cap=0), dict(n=-1), dict(B=0)):
        _rejected(lib, pr(**bad))


@pytest.mark.parametrize("scale", [1.0, 512.0 / 19.0, 9.95])
def test_surface_thresholds_match_searchsorted_for_every_squared_distance(lib, scale):
    """bin of an integer squared distance by the integer thresholds == numpy's bin of sqrt(n) / scale by the edges, for
    EVERY n up to 2 * 1024^2, with edges that are exact lattice distances (which is what pins the [lo, hi) convention)"""
    from particle_col_image_segmentation_amd import ops
    n = np.arange(2 * 1024 * 1024 + 1, dtype=np.int64)
    d = np.sqrt(n.astype(np.float64)) / scale
    lattice = np.array([1, 2, 4, 5, 8, 9, 10, 13, 25, 50, 100, 101, 1000, 4096, 65536, 1000000, 2 * 1024 * 1024], np.float64)
    rng = np.random.default_rng(17)
    for edges in (np.concatenate([[0.0], np.sqrt(lattice) / scale]),
                  np.linspace(0.0, 1500.0 / scale, 1025),
                  np.concatenate([[0.0], np.sort(rng.uniform(0.01, 1400.0 / scale, 63))]),
                  np.array([0.0, 5000.0 / scale])):
        thr = ops.surface_thresholds(edges, scale)
        assert thr[0] == 0 and (np.diff(thr) >= 0).all()
        want = np.searchsorted(edges, d, side="right") - 1
        got = np.searchsorted(thr, n, side="right") - 1
        np.testing.assert_array_equal(got, want)
    on_edge = ops.surface_thresholds(np.concatenate([[0.0], np.sqrt(lattice) / scale]), scale)[1:]
    np.testing.assert_array_equal(on_edge, lattice.astype(np.int64))  # a distance exactly on an edge belongs to the bin above
    assert ops.surface_thresholds([0.0, 1e300], 1.0)[1] == np.iinfo(np.int64).max


def test_surface_kernels_compile_for_gfx950(tmp_path):
    """a COMPILE of csrc/surface.hip for gfx950 (no run): no scratch in any of its kernels"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "particle_col_image_segmentation_amd", "csrc", "surface.hip")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Rpass-analysis=kernel-resource-usage",
                          "-c", src, "-o", str(tmp_path / "surface.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert "sf_search_kernel" in out.stdout
    scratch = [line for line in out.stdout.splitlines() if "ScratchSize" in line]
    assert len(scratch) >= 10 and all(line.split("ScratchSize [bytes/lane]:")[1].split()[0] == "0" for line in scratch), out.stdout
