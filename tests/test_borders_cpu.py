"""The restatement of the border tables and of the merge (tests/borders_reference.py) on hand-made images whose answer is
written out here, its mean against fractions.Fraction, its groups against networkx, the derived bound between the fixed-point
mean and a float64 mean, and the C ABI's workspace sizes and argument errors.  No GPU here."""
import ctypes
from fractions import Fraction

import networkx as nx
import numpy as np
import pytest

import borders_reference as ref

F = np.float32
TWO32 = 2 ** 32


def rows(L, V, conn, cap=None):
    a, b, links, total, saddle, flags = ref.frame_borders(np.asarray(L), np.asarray(V, F), conn, cap)
    return {(int(x), int(y)): (int(n), int(s), float(m)) for x, y, n, s, m in zip(a, b, links, total, saddle)}, flags


def fixed(v):
    return int(np.rint(np.float64(F(v)) * TWO32))


def slow_links(L, V, conn):
    """Every link of a small frame by a plain loop over the pixels: {(a, b): [float32 link values]}."""
    L, V = np.asarray(L), ref.read_values(V)[0]
    H, W = L.shape
    out = {}
    for r in range(H):
        for c in range(W):
            for dr, dc in ref.STEPS[conn]:
                rr, cc = r + dr, c + dc
                if 0 <= rr < H and 0 <= cc < W and L[r, c] >= 1 and L[rr, cc] >= 1 and L[r, c] != L[rr, cc]:
                    key = (int(min(L[r, c], L[rr, cc])), int(max(L[r, c], L[rr, cc])))
                    out.setdefault(key, []).append(max(V[r, c], V[rr, cc]))
    return out


# ---- hand-made images
def test_two_stripes():
    L = [[1, 1, 2, 2]] * 3
    V = [[0.125, 0.25, 0.5, 0.75]] * 3
    got, flags = rows(L, V, 4)
    assert flags == 0 and got == {(1, 2): (3, 3 * 2 ** 31, 0.5)}  # one link per row, each max(0.25, 0.5)
    got, _ = rows(L, V, 8)
    assert got == {(1, 2): (7, 7 * 2 ** 31, 0.5)}  # and two diagonals per pair of rows, both ways


def test_four_labels_two_by_two():
    L = [[1, 2], [3, 4]]
    V = [[0.1, 0.2], [0.3, 0.4]]
    v = lambda x: (1, fixed(x), float(F(x)))
    got4, _ = rows(L, V, 4)
    assert got4 == {(1, 2): v(0.2), (1, 3): v(0.3), (2, 4): v(0.4), (3, 4): v(0.4)}
    got8, _ = rows(L, V, 8)
    assert got8 == {**got4, (1, 4): v(0.4), (2, 3): v(0.3)}  # the diagonal pairs exist only for conn = 8


def test_enclosed_label():
    L = np.ones((5, 5), np.int32)
    L[2, 2] = 2
    V = np.full((5, 5), 0.25, F)
    V[2, 2] = 0.125  # the ring is the ridge: every link's value is the ring's
    V[1, 1] = 0.75   # ... and one diagonal neighbour's is higher
    assert rows(L, V, 4)[0] == {(1, 2): (4, 4 * 2 ** 30, 0.25)}
    assert rows(L, V, 8)[0] == {(1, 2): (8, 7 * 2 ** 30 + 3 * 2 ** 30, 0.25)}


def test_a_line_of_zeros_separates():
    L = [[1, 1, 1], [0, 0, 0], [2, 2, 2]]
    V = np.full((3, 3), 0.5, F)
    assert rows(L, V, 4)[0] == {} and rows(L, V, 8)[0] == {}
    # a diagonal gap does not separate under conn = 8
    assert rows([[1, 0], [0, 2]], np.full((2, 2), 0.5, F), 4)[0] == {}
    assert rows([[1, 0], [0, 2]], np.full((2, 2), 0.5, F), 8)[0] == {(1, 2): (1, 2 ** 31, 0.5)}


def test_labels_and_values_outside_their_ranges():
    L = [[1, 2, 9, -3]]
    V = [[np.nan, -1.0, 2.0, 0.5]]
    got, flags = rows(L, V, 8, cap=2)
    assert flags == 2 | 4 and got == {(1, 2): (1, 0, 0.0)}  # 9 and -3 are background; NaN and -1 read 0
    got, flags = rows([[1, 2]], [[0.5, 2.0]], 4, cap=2)
    assert flags == 4 and got == {(1, 2): (1, TWO32, 1.0)}
    assert rows([[1, 2]], [[0.5, 1.0]], 4, cap=2)[1] == 0


# ---- against independent arithmetic
def test_against_a_plain_loop_and_fractions():
    rng = np.random.default_rng(3)
    for trial in range(12):
        H, W = rng.integers(1, 9, 2)
        L = rng.integers(0, 6, (H, W))
        V = rng.random((H, W), dtype=F)
        if trial % 3 == 0:
            V = V * F(2.0 ** -rng.integers(8, 34))  # values below 2^-9: rint matters
        for conn in (4, 8):
            got, _ = rows(L, V, conn)
            want = slow_links(L, V, conn)
            assert set(got) == set(want)
            for key, vals in want.items():
                n, s, m = got[key]
                assert n == len(vals) and m == float(min(vals))
                assert s == sum(int(np.rint(np.float64(v) * TWO32)) for v in vals)
                exact = Fraction(s, n * TWO32)
                assert np.float64(s) / (np.float64(n) * TWO32) == float(exact)  # the correctly rounded quotient (sum < 2^53)
                assert ref.exact_mean([s], [n])[0] == float(exact)


def test_fixed_point_mean_within_the_derived_bound():
    """Against a float64 mean of the float32 link values: a link's fixed value is off by at most 2^-33 (rint below 2^-9, exact
    above), so the exact quotient is within 2^-33 of the exact mean; the float64 sum of `links` terms and its division add at
    most links 2^-53 max(1, mean), the fixed-point quotient's own rounding is inside that.  k/100 maps: equal."""
    rng = np.random.default_rng(11)
    for trial in range(10):
        L = rng.integers(0, 5, (12, 10))
        V = rng.random((12, 10), dtype=F) * F(1.0 if trial % 2 else 2.0 ** -12)
        K = (rng.integers(0, 101, (12, 10)) / 100.0).astype(F)
        got, _ = rows(L, V, 8)
        gotk, _ = rows(L, K, 8)
        for key, vals in slow_links(L, V, 8).items():
            n, s, _ = got[key]
            mean64 = float(np.sum(np.asarray(vals, np.float64)) / len(vals))
            fixed_mean = s / (n * TWO32)
            assert abs(fixed_mean - mean64) <= 2.0 ** -33 + n * 2.0 ** -53 * max(1.0, mean64)
        for key, vals in slow_links(L, K, 8).items():
            n, s, _ = gotk[key]
            assert all(v >= 2.0 ** -9 or v == 0 for v in vals)
            assert s / (n * TWO32) == float(np.sum(np.asarray(vals, np.float64)) / len(vals))


def test_groups_equal_networkx():
    rng = np.random.default_rng(5)
    for trial in range(30):
        cap = int(rng.integers(1, 40))
        count = int(rng.integers(0, cap + 1))
        n = int(rng.integers(0, 60))
        a = rng.integers(1, cap + 1, n)
        b = rng.integers(1, cap + 1, n)
        a, b = np.minimum(a, b), np.maximum(a, b)
        keep = a != b
        a, b = a[keep], b[keep]
        join = rng.random(len(a)) < 0.5
        got, m = ref.group_map(a, b, join, count, cap)
        g = nx.Graph()
        g.add_nodes_from(range(1, count + 1))
        g.add_edges_from((int(x), int(y)) for x, y, j in zip(a, b, join) if j and x <= count and y <= count)
        comps = sorted(nx.connected_components(g), key=min)  # numbered by their smallest member
        assert m == len(comps)
        want = np.zeros(cap + 1, np.int32)
        for i, comp in enumerate(comps):
            want[list(comp)] = i + 1
        assert np.array_equal(got, want)
        assert got[0] == 0 and not got[count + 1:].any()


def test_merge_rule_is_strict_and_one_pass():
    # the pair's mean equals the threshold exactly: not joined; joined at the next float above
    L = np.array([[[1, 2]]])
    V = np.array([[[0.25, 0.37]]], F)
    t = float(F(0.37))
    assert ref.merge(L, V, t)[1][0] == 2
    assert ref.merge(L, V, float(np.nextafter(F(0.37), F(1))))[1][0] == 1
    assert ref.merge(L, V, t, by="saddle")[1][0] == 2 and ref.merge(L, V, float(np.nextafter(F(0.37), F(1))), by="saddle")[1][0] == 1
    # below = 0 joins nothing: the image comes back
    Lr = np.random.default_rng(2).integers(0, 6, (2, 7, 9))
    Vr = np.random.default_rng(3).random((2, 7, 9), dtype=F)
    merged, n, maps, _ = ref.merge(Lr, Vr, 0.0, cap=5)
    assert np.array_equal(merged, Lr) and n.tolist() == [5, 5] and np.array_equal(maps[0], np.arange(6))
    # a chain 1-2-3-4 with one weak border (a link's value is the larger end: 0.9 makes both of label 3's borders strong);
    # counts below cap drop labels
    L = np.array([[[1, 2, 3, 4]]])
    V = np.array([[[0.1, 0.1, 0.9, 0.1]]], F)
    merged, n, maps, _ = ref.merge(L, V, 0.5)
    assert merged.tolist() == [[[1, 1, 2, 3]]] and n[0] == 3 and maps[0].tolist() == [0, 1, 1, 2, 3]
    merged, n, maps, _ = ref.merge(L, V, 0.5, counts=[3])
    assert merged.tolist() == [[[1, 1, 2, 0]]] and n[0] == 2 and maps[0].tolist() == [0, 1, 1, 2, 0]
    # numbering by smallest member: {1, 3} comes before {2}
    merged, n, maps, _ = ref.merge(np.array([[[2, 1, 3]]]), np.array([[[0.9, 0.1, 0.1]]], F), 0.5)
    assert merged.tolist() == [[[2, 1, 1]]] and n[0] == 2 and maps[0].tolist() == [0, 1, 2, 1]


# ---- the C ABI (fails without the feature)
@pytest.fixture(scope="module")
def lib():
    from particle_col_image_segmentation_amd import build
    build.build()
    from particle_col_image_segmentation_amd import _lib
    return _lib.load()


def test_border_workspace_query_and_argument_checks(lib):
    """Argument and workspace checks come before the first device call: nothing here touches a device."""
    B, H, W, cap, pair_cap = 2, 96, 80, 100, 400
    need = lib.pcseg_label_borders_workspace_bytes(B, pair_cap, cap)
    assert need > 0 and need % 256 == 0
    assert need >= B * pair_cap * 24 + B * (cap + 1) * 4  # key, links, saddle, 64-bit sum per slot; the merge's parents
    for bad in ((0, pair_cap, cap), (B, 0, cap), (B, pair_cap, 0), (65536, pair_cap, cap)):
        assert lib.pcseg_label_borders_workspace_bytes(*bad) == 0
    p = ctypes.c_void_p(4096)
    fill = lambda **kw: lib.pcseg_label_borders(kw.get("labels", p), p, kw.get("stride", H * W), cap, kw.get("conn", 8), pair_cap, p, p, p,
                                                B, H, W, p, kw.get("nbytes", need), None)
    assert fill(nbytes=need - 1) == -3 and b"workspace too small" in lib.pcseg_last_error()
    assert fill(labels=None) == -1 and b"bad arguments" in lib.pcseg_last_error()
    assert fill(stride=H * W - 1) == -1
    assert fill(conn=6) == -1 and b"conn" in lib.pcseg_last_error()
    assert lib.pcseg_label_borders_write(pair_cap, cap, p, p, p, p, p, p, B, p, need - 1, None) == -3
    assert lib.pcseg_label_borders_write(pair_cap, cap, None, p, p, p, p, p, B, p, need, None) == -1
    merge = lambda below=0.5, by=0, nbytes=need, flags=p: lib.pcseg_border_merge(pair_cap, cap, None, below, by, flags, p, p, B, p, nbytes, None)
    assert merge(nbytes=need - 1) == -3 and b"workspace too small" in lib.pcseg_last_error()
    assert merge(flags=None) == -1
    assert merge(below=1.5) == -1 and b"threshold" in lib.pcseg_last_error()
    assert merge(below=float("nan")) == -1 and merge(below=-0.1) == -1
    assert merge(by=2) == -1
    assert lib.pcseg_relabel_map(None, p, cap, p, B, H, W, None) == -1 and lib.pcseg_relabel_map(p, p, 0, p, B, H, W, None) == -1
    assert lib.pcseg_relabel_map(p, p, cap, p, B, 0, W, None) == -1


def test_border_block_is_the_sibling_walks():
    from particle_col_image_segmentation_amd import ops
    R, C, lds = ops.border_block()
    assert (R, C) == (32, 256) and lds >= 1024
