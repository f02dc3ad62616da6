"""The row writer that the three per-frame pair tables share (csrc/pair_table.h: pair_write_kernel behind
pcseg_territory_pairs_write, pcseg_contingency_write and pcseg_label_borders_write) and the two-call protocol around it
(ops._pair_fill / ops._pair_rows), at the table sizes where the compaction can go wrong: a table that is exactly full, one
slot more, a whole number of 256-slot chunks, one slot past a chunk, and one slot too few.  Three frames of one pixel per
label, so the number of pairs of a frame is known in closed form and exceeds one chunk; the middle frame has no pair at
all (its rows are an empty range between two equal offsets).  The references are those of the tables' own tests."""
import functools

import numpy as np
import pytest

import borders_reference as bref
from test_agreement_cpu import pair_rows
from test_territory_cpu import adjacency_pairs, degrees

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

B, H, W = 3, 16, 24
CAP = H * W  # one label per pixel
K = 3        # type slots of the territory degrees (slot 3: no type)
N4 = H * (W - 1) + (H - 1) * W           # 4-neighbour pixel pairs: 728
N8 = N4 + 2 * (H - 1) * (W - 1)          # 8-neighbour pixel pairs: 1418
PAIRS = {"territory": N4, "contingency": CAP, "borders": N8}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")


@functools.lru_cache(maxsize=None)
def _inputs():
    """the label batch (frames 0 and 2: one label per pixel, in raster order and reversed; frame 1: empty), a strength
    image and the territories' type slots"""
    rng = np.random.default_rng(11)
    lab = np.zeros((B, H, W), np.int32)
    lab[0] = 1 + np.arange(CAP).reshape(H, W)
    lab[2] = CAP - np.arange(CAP).reshape(H, W)
    val = rng.random((B, H, W)).astype(np.float32)
    slot_of = rng.integers(0, K + 1, (B, CAP)).astype(np.uint8)
    return lab, val, slot_of


@functools.lru_cache(maxsize=None)
def _reference(table):
    """per frame: (keys int64 sorted, {column: values in that order}); for the territories also the degrees"""
    lab, val, slot_of = _inputs()
    out = []
    for b in range(B):
        if table == "territory":  # every pixel is its own site: near = the labels, d2 = 0 (-1 in the frame without site)
            p = adjacency_pairs(lab[b], np.where(lab[b] > 0, 0, -1), -1)
            out.append(((p[:, 0] << 32) | p[:, 1], {"counts": p[:, 2:4]}, degrees(p, slot_of[b], K)))
        elif table == "contingency":
            t, s, n, over = pair_rows(lab[b], lab[b], CAP, CAP)
            assert over == 0
            out.append(((t << 32) | s, {"n": n}, None))
        else:
            a, c, links, total, saddle, flags = bref.frame_borders(lab[b], val[b], 8, CAP)
            assert flags == 0
            out.append(((a << 32) | c, {"links": links, "sum": total, "saddle": bref.float_bits(saddle)}, None))
    n = PAIRS[table]
    assert [len(r[0]) for r in out] == [n, 0, n] and n > 256
    return out


def _run(table, pair_cap):
    """both calls of one table through the protocol's helpers: (state of the fill, rows, n_overflow, sorted rows, degree)"""
    from particle_col_image_segmentation_amd import ops
    lab, val, slot_of = _inputs()
    dev = torch.device("cuda")
    L = torch.from_numpy(lab).to(dev)
    degree = None
    if table == "territory":
        d2 = torch.where(L > 0, 0, -1).to(torch.int32)
        slots = torch.from_numpy(slot_of).to(dev)
        degree = torch.zeros((B, CAP, 2 * K), dtype=torch.int32, device=dev)
        query = (B, pair_cap)
        fill = ("territory_pairs", (L, d2, -1, pair_cap))
        columns = (("counts", torch.int32, (2,)),)
        write = lambda off, out, ws, n: ops._call(
            "territory_pairs_write", pair_cap, off, slots, CAP, K, out["key"], out["frame"], out["counts"], degree, B, ws=(ws, n))
    elif table == "contingency":
        query = (B, pair_cap)
        fill = ("label_contingency", (L, L, CAP, CAP, pair_cap))
        columns = (("n", torch.int64, ()),)
        write = lambda off, out, ws, n: ops._call(
            "contingency_write", pair_cap, off, out["key"], out["frame"], out["n"], B, ws=(ws, n))
    else:
        V = torch.from_numpy(val).to(dev)
        query = (B, pair_cap, CAP)
        fill = ("label_borders", (L, V, H * W, CAP, 8, pair_cap))
        columns = (("links", torch.int32, ()), ("sum", torch.int64, ()), ("saddle", torch.float32, ()))
        write = lambda off, out, ws, n: ops._call(
            "label_borders_write", pair_cap, CAP, off, out["key"], out["frame"], out["links"], out["sum"], out["saddle"], B, ws=(ws, n))
    st = ops._pair_fill(*fill, (B, H, W), dev, query)
    rows, n_over, r = ops._pair_rows(st, columns, write)
    torch.cuda.synchronize()
    return st, rows, n_over, {k: v.cpu().numpy() for k, v in r.items()}, degree


def _caps(n):
    m = (n // 256 + 1) * 256  # the next multiple of 256 above n
    return [n, n + 1, m, m + 1]


@pytest.mark.parametrize("which", range(4))
@pytest.mark.parametrize("table", sorted(PAIRS))
def test_every_row_and_counter_at_the_chunk_and_capacity_edges(table, which):
    """pair_cap = n (exactly full, no flag), n + 1, the next multiple of 256 and one past it: every row and counter equals
    the reference, offsets are the running sum of the frames' row counts and totals = (rows, 0)."""
    _need_gpu()
    n = PAIRS[table]
    pair_cap = _caps(n)[which]
    want = _reference(table)
    st, rows, n_over, r, degree = _run(table, pair_cap)
    assert (rows, n_over) == (2 * n, 0) and st["totals"].cpu().tolist() == [2 * n, 0]
    assert st["offsets"].cpu().tolist() == [0, n, n, 2 * n]
    assert st["overflow"].cpu().tolist() == [0, 0, 0]
    assert r["key"].dtype == np.int64 and r["frame"].dtype == np.int64 and r["key"].shape == (2 * n,)
    np.testing.assert_array_equal(r["frame"], np.repeat([0, 2], n))
    for b, lo in ((0, 0), (2, n)):
        keys, cols, deg = want[b]
        np.testing.assert_array_equal(r["key"][lo:lo + n], keys, err_msg="%s frame %d keys" % (table, b))
        for name, v in cols.items():
            got = r[name][lo:lo + n]
            got = bref.float_bits(got) if name == "saddle" else got
            np.testing.assert_array_equal(got, v, err_msg="%s frame %d %s" % (table, b, name))
    if table == "territory":
        for b in range(B):
            np.testing.assert_array_equal(degree[b].cpu().numpy(), want[b][2], err_msg="degree of frame %d" % b)


@pytest.mark.parametrize("table", sorted(PAIRS))
def test_one_slot_too_few(table):
    """pair_cap = n - 1: bit 1 on exactly the two frames with pairs, totals[1] = 2, and each of them has exactly pair_cap
    rows (a table is full before its flag goes up), every one a pair of the reference, none twice.  Counters are not
    compared: which pairs are dropped, and what was added to a pair before the flag went up, depends on the order of
    arrival."""
    _need_gpu()
    n = PAIRS[table]
    pair_cap = n - 1
    want = _reference(table)
    st, rows, n_over, r, _ = _run(table, pair_cap)
    assert (rows, n_over) == (2 * pair_cap, 2) and st["totals"].cpu().tolist() == [2 * pair_cap, 2]
    assert [v & 1 for v in st["overflow"].cpu().tolist()] == [1, 0, 1]
    assert st["offsets"].cpu().tolist() == [0, pair_cap, pair_cap, 2 * pair_cap]
    np.testing.assert_array_equal(r["frame"], np.repeat([0, 2], pair_cap))
    for b, lo in ((0, 0), (2, pair_cap)):
        keys = r["key"][lo:lo + pair_cap]
        assert (np.diff(keys) > 0).all(), (table, b)  # sorted by the helper: distinct
        assert np.isin(keys, want[b][0]).all(), (table, b)
