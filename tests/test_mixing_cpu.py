"""CPU checks of the random-labelling tables (csrc/mixing.hip): column schemas, the switches, the host epilogue, the
gather's sort key, argument rejection by the two C exports, and the numpy restatement's own invariants (no device is
touched)."""
import collections
import ctypes

import numpy as np
import pytest

import mixing_reference as mr

torch = pytest.importorskip("torch")

CT3 = {1: "3D05", 2: "6B07", 3: "Particle", 4: "C3M10", 5: "Background"}
COLS = ["frame", "slot_a", "slot_b", "bin", "r_lo_um", "r_hi_um", "n_perm", "obs", "mean", "lo", "hi", "n_le", "n_ge",
        "cum_obs", "cum_mean", "cum_lo", "cum_hi", "cum_n_le", "cum_n_ge"]


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
    two = _pipe().table_columns(5, pair_edges=edges, mixing=19)
    assert two["mixing"] == COLS and "refined_mixing" not in two and "pair_hist" in two
    three = _pipe(CT3).table_columns(5, pair_edges=np.linspace(0, 10, 65), mixing=199, mixing_seed=7, refined=True)
    assert three["mixing"] == COLS and three["refined_mixing"] == COLS
    from particle_col_image_segmentation_amd import tiff_analysis as ta
    assert ta.MIXING_COLUMNS == COLS


def test_tables_absent_without_the_switch():
    edges = [0.0, 1.0, 2.0]
    for kw in (dict(), dict(pair_edges=edges), dict(pair_edges=edges, mixing=0), dict(pair_edges=edges, mixing=None, refined=True)):
        cols = _pipe().table_columns(5, **kw)
        assert "mixing" not in cols and "refined_mixing" not in cols, kw


def test_mixing_without_pair_edges_raises():
    pipe = _pipe()
    with pytest.raises(ValueError):
        pipe.table_columns(5, mixing=19)
    with pytest.raises(ValueError):
        pipe.empty_device_tables(5, device="cpu", mixing=19)
    with pytest.raises(ValueError):
        pipe.host_tables({}, 5, mixing=19)
    with pytest.raises(ValueError):
        pipe.table_columns(5, pair_edges=[0.0, 1.0], mixing=65536)


def test_switch_and_table_positions():
    from particle_col_image_segmentation_amd.pipeline import OPTIONAL_TABLES, TableSwitches
    f = TableSwitches._fields
    assert f[f.index("pair_edges") + 1:f.index("pair_edges") + 3] == ("mixing", "mixing_seed")
    assert TableSwitches().mixing is None and TableSwitches().mixing_seed == 0
    names = [t.name for t in OPTIONAL_TABLES]
    assert names[names.index("pair_hist") + 1] == "mixing" and names[names.index("refined_pair_hist") + 1] == "refined_mixing"
    from particle_col_image_segmentation_amd.distributed import _SORT_COLS
    assert _SORT_COLS["mixing"] == (0, 1, 2, 3) and _SORT_COLS["refined_mixing"] == (0, 1, 2, 3)


def test_empty_device_tables_and_host_tables_widths():
    pipe = _pipe(CT3)
    e = [0.0, 1.0, 2.0]
    kw = dict(pair_edges=e, mixing=19, refined=True)
    dt = pipe.empty_device_tables(5, device="cpu", **kw)
    assert dt["mixing"].shape == (0, 19) and dt["refined_mixing"].shape == (0, 19)
    assert "mixing" not in pipe.empty_device_tables(5, device="cpu", pair_edges=e)
    C = 5
    cols = pipe.table_columns(C, pair_edges=e, mixing=19)
    z = lambda k, n: torch.zeros((n, len(cols[k])), dtype=torch.float64)
    mix = torch.arange(12 * 19, dtype=torch.float64).reshape(12, 19)
    dt = {"rois": z("rois", 0), "cells": z("cells", 2), "groups": z("groups", 0),
          "frames_rec": torch.zeros((1, 18), dtype=torch.float64), "distances": torch.zeros((0, 3), dtype=torch.float64),
          "pair_hist": z("pair_hist", 6), "mixing": mix}
    out = pipe.host_tables(dt, C, pair_edges=e, mixing=19)
    np.testing.assert_array_equal(out["mixing"], mix.numpy())
    assert out["mixing_columns"] == COLS
    with pytest.raises(ValueError):
        pipe.host_tables({k: v for k, v in dt.items() if k != "mixing"}, C, pair_edges=e, mixing=19)
    assert "mixing" not in pipe.host_tables({k: v for k, v in dt.items() if k != "mixing"}, C, pair_edges=e)


def test_gather_sorts_mixing_by_frame_pair_and_bin():
    from particle_col_image_segmentation_amd.distributed import gather_tables
    rng = np.random.default_rng(5)
    rows = np.array([(f, a, b, k) for f in range(3) for a in range(2) for b in range(a, 2) for k in range(4)], np.float64)
    table = np.concatenate([rows, rng.integers(0, 100, (rows.shape[0], 15)).astype(np.float64)], axis=1)
    out = gather_tables({"mixing": table[rng.permutation(table.shape[0])]})
    np.testing.assert_array_equal(out["mixing"], table)


def _mix_call(lib, K=2, scale=1.0, edges=(0.0, 1.0, 2.0), n_edges=None, P=19, null=None, n=10, ws=1 << 24):
    p = ctypes.c_void_p(4096)  # never dereferenced: the arguments are rejected first
    e = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64)
    ep = ctypes.c_void_p(e.ctypes.data) if e is not None else ctypes.c_void_p(0)
    ne = (0 if e is None else e.shape[0]) if n_edges is None else n_edges
    args = {k: p for k in ("xy", "slot", "foff", "keys", "counts", "env", "ws")}
    if null:
        args[null] = ctypes.c_void_p(0)
    return lib.pcseg_pair_label_mixing(args["xy"], args["slot"], args["foff"], args["keys"], n, 1, K, scale, ep, ne, P, 0,
                                       args["counts"], args["env"], args["ws"], ws, None)


def test_pair_label_mixing_rejects_bad_arguments(lib):
    checks = [dict(null="xy"), dict(null="slot"), dict(null="foff"), dict(null="keys"), dict(null="env"), dict(null="ws"),
              dict(K=0), dict(K=5), dict(P=-1), dict(P=65536), dict(scale=0.0), dict(scale=float("nan")), dict(edges=None),
              dict(edges=[0.5, 1.0]), dict(edges=[0.0, 2.0, 1.0]), dict(edges=[0.0]), dict(edges=np.linspace(0, 1, 1026)),
              dict(edges=[0.0, float("inf")]), dict(n=1 << 24), dict(n=-1)]
    for kw in checks:
        rc = _mix_call(lib, **kw)
        assert rc == -1 and b"bad arguments" in lib.pcseg_last_error(), kw
    assert _mix_call(lib, ws=64) == -3 and b"workspace too small" in lib.pcseg_last_error()
    wb = lib.pcseg_mixing_workspace_bytes
    assert wb(1000, 2, 5, 3, 19, 1) == 0 and wb(1000, 2, 0, 3, 19, 1) == 0 and wb(1000, 2, 2, 3, 65536, 1) == 0
    assert wb(1000, 2, 2, 1, 19, 1) == 0 and wb(1 << 24, 2, 2, 3, 19, 1) == 0 and wb(1000, 0, 2, 3, 19, 1) == 0
    own, given = wb(1000, 2, 3, 65, 199, 1), wb(1000, 2, 3, 65, 199, 0)
    assert given >= 1000 * (16 + 4 + 16 * 4) and own - given >= 8 * 2 * 200 * 6 * 64
    assert lib.pcseg_mixing_tile() >= 64


# ---- the restatement's own invariants
def test_reference_keeps_counts_and_observed_labelling():
    rng = np.random.default_rng(1)
    for K in (1, 2, 3, 4):
        slots = rng.integers(0, K, 57)
        lab = mr.labellings(slots, K, 40, key=3, seed=9)
        np.testing.assert_array_equal(lab[0], slots)
        want = np.bincount(slots, minlength=K)
        for row in lab:
            np.testing.assert_array_equal(np.bincount(row, minlength=K), want)
        assert K == 1 or len({tuple(r) for r in lab[1:]}) > 30
        assert K == 1 or not np.array_equal(lab, mr.labellings(slots, K, 40, key=4, seed=9))
        assert K == 1 or not np.array_equal(lab, mr.labellings(slots, K, 40, key=3, seed=10))
    # the key enters with its low 24 bits
    np.testing.assert_array_equal(mr.labellings(slots, 4, 5, key=3, seed=9), mr.labellings(slots, 4, 5, key=3 + (1 << 24), seed=9))


def test_reference_arrangements_are_near_uniform():
    """Four points in two strains: six arrangements, 6 000 draws.  A count is Binomial(6000, 1/6): mean 1000, standard
    deviation 28.9; all six within 4.5 standard deviations (870 .. 1130) fails by chance about 4e-5 of the time -- and the
    draws are fixed by key and seed, so the test is deterministic."""
    lab = mr.labellings([0, 0, 1, 1], 2, 6000, key=0, seed=0)
    hits = collections.Counter(map(tuple, lab[1:]))
    assert len(hits) == 6 and sum(hits.values()) == 6000
    assert 870 <= min(hits.values()) and max(hits.values()) <= 1130, sorted(hits.values())


def test_reference_detects_segregation():
    """Left / right segregated strains: every cross-strain bin of the observed histogram lies below all 199 shuffles."""
    rng = np.random.default_rng(0)
    xy = rng.uniform(0, 100, (300, 2))
    slot = (xy[:, 0] > 50).astype(np.int32)
    counts = mr.mixing(xy, slot, np.array([0, 300]), 2, 1.0, np.linspace(0, 10, 11), 199)
    env = mr.envelope(counts)
    assert (env["obs"][0, 1] < env["lo"][0, 1]).all() and (env["n_le"][0, 1] == 0).all() and (env["n_ge"][0, 1] == 199).all()
    # relabelling moves pairs between the rows, never between the bins
    np.testing.assert_array_equal(counts.sum(axis=2), np.broadcast_to(counts[:, :1].sum(axis=2), counts.sum(axis=2).shape))
    e0 = mr.envelope(counts[:, :1])
    assert all((e0[k] == 0).all() for k in e0 if k not in ("obs", "cum_obs"))
