"""The nearest-label transform, territories and adjacency restated in numpy by brute force (no GPU), checked against
scipy / scikit-image through tests/golden/territory.npz, and the host-only reach thresholds against ``np.sqrt``.

The restatement is what tests/test_gpu_territory.py compares the device with, by equality.  Definitions (include/pcseg.h): a
site is a pixel whose label lies in 1 .. cap and is selected; D2(p) the smallest squared distance to a site, N(p) the
smallest label among the sites at that distance, Q(p) the smallest raster index among the sites of label N(p) at that
distance; a pixel belongs to N(p) iff 0 <= D2(p) <= R2 (R2 < 0: unbounded)."""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "territory.npz")
TIE_SHARE_CAP = 0.01  # of the pixels of a seeded layout


# ---------------------------------------------------------------- restatement
def site_mask(lab, sel=None, cap=None):
    lab = np.asarray(lab).astype(np.int64)
    cap = int(lab.max()) if cap is None else int(cap)
    ok = (lab >= 1) & (lab <= cap)
    if sel is not None:
        sel = np.asarray(sel).astype(bool)
        keep = np.zeros(cap + 1, bool)
        keep[1:] = sel[:cap]
        ok &= keep[np.where(ok, lab, 0)]
    return ok


def nearest_label(lab, sel=None, cap=None, chunk=1 << 21):
    """(D2, N, Q) of one (H, W) label image, int64: every pixel against every site, the lexicographic minimum of (d2, label,
    raster index)."""
    lab = np.asarray(lab).astype(np.int64)
    H, W = lab.shape
    sites = site_mask(lab, sel, cap)
    qr, qc = np.nonzero(sites)
    if qr.size == 0:
        return np.full((H, W), -1, np.int64), np.zeros((H, W), np.int64), np.full((H, W), -1, np.int64)
    ql, qi = lab[qr, qc], qr * W + qc
    npx = H * W
    sub = ql * npx + qi  # (label, index) as one number; d2 * scale + sub orders (d2, label, index)
    scale = (int(ql.max()) + 1) * npx
    assert (H * H + W * W) * scale < 2 ** 62
    d2, near, site = (np.empty(npx, np.int64) for _ in range(3))
    pr, pc = np.divmod(np.arange(npx), W)
    step = max(1, chunk // qr.size)
    for lo in range(0, npx, step):
        hi = min(npx, lo + step)
        d = (pr[lo:hi, None] - qr[None]) ** 2 + (pc[lo:hi, None] - qc[None]) ** 2
        best = np.argmin(d * scale + sub[None], axis=1)
        d2[lo:hi], near[lo:hi], site[lo:hi] = d[np.arange(hi - lo), best], ql[best], qi[best]
    return d2.reshape(H, W), near.reshape(H, W), site.reshape(H, W)


def tie_mask(lab):
    """pixels whose two nearest DISTINCT labels are equally far"""
    lab = np.asarray(lab).astype(np.int64)
    d2, near, _ = nearest_label(lab)
    tie = np.zeros(lab.shape, bool)
    if (d2 < 0).all():
        return tie
    for l in np.unique(lab[lab > 0]):
        dl, _, _ = nearest_label(np.where(lab == l, l, 0))
        tie |= (dl == d2) & (near != l)
    return tie


def owned(near, d2, r2):
    near, d2 = np.asarray(near).astype(np.int64), np.asarray(d2).astype(np.int64)
    ok = (near >= 1) & (d2 >= 0)
    if r2 >= 0:
        ok &= d2 <= r2
    return np.where(ok, near, 0)


def territory_table(near, d2, r2, cap, mask=None):
    """int64 (cap, 4): territory_px, territory_on_px, reach2_max, clipped per label 1 .. cap"""
    own = owned(near, d2, r2)
    H, W = own.shape
    edge = np.zeros((H, W), bool)
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
    on = np.zeros((H, W), bool) if mask is None else np.asarray(mask) != 0
    out = np.zeros((cap, 4), np.int64)
    for l in np.unique(own[(own >= 1) & (own <= cap)]):
        m = own == l
        out[l - 1] = [m.sum(), (m & on).sum(), np.asarray(d2)[m].max(), int((m & edge).any())]
    return out


def adjacency_pairs(near, d2, r2):
    """int64 (n, 4): a, b (a < b), border_px, contact_px, sorted by (a, b)"""
    own = owned(near, d2, r2)
    zero = np.asarray(d2) == 0
    acc = {}
    for a, b, za, zb in ((own[:, :-1], own[:, 1:], zero[:, :-1], zero[:, 1:]), (own[:-1], own[1:], zero[:-1], zero[1:])):
        link = (a > 0) & (b > 0) & (a != b)
        lo, hi = np.minimum(a, b)[link], np.maximum(a, b)[link]
        for x, y, ct in zip(lo.tolist(), hi.tolist(), (za & zb)[link].tolist()):
            e = acc.setdefault((x, y), [0, 0])
            e[0] += 1
            e[1] += int(ct)
    return np.array([[a, b, v[0], v[1]] for (a, b), v in sorted(acc.items())], np.int64).reshape(-1, 4)


def degrees(pairs, slot_of, n_types):
    """int64 (cap, 2 K): distinct partners per type slot, then those with contact (``slot_of`` (cap,), >= K: no type)"""
    K = int(n_types)
    out = np.zeros((len(slot_of), 2 * K), np.int64)
    for a, b, _, ct in np.asarray(pairs).tolist():
        for x, y in ((a, b), (b, a)):
            s = int(slot_of[y - 1])
            if s < K:
                out[x - 1, s] += 1
                out[x - 1, K + s] += int(ct > 0)
    return out


def reach_r2(distance, n_max):
    """the largest n <= n_max with np.sqrt(float64(n)) <= distance, straight from the definition; None: none"""
    ok = np.sqrt(np.arange(n_max + 1, dtype=np.float64)) <= distance
    return int(np.nonzero(ok)[0].max()) if ok.any() else None


def expand_labels(lab, distance):
    d2, near, _ = nearest_label(lab)
    r2 = reach_r2(distance, int(max(d2.max(), 0)))
    return np.zeros_like(near) if r2 is None else owned(near, d2, r2)


# ---------------------------------------------------------------- the fixture
@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _cases(golden):
    return [str(n) for n in golden["names"]]


def test_fixture_holds_the_cases_it_should(golden):
    names = _cases(golden)
    seeded = [n for n in names if n.startswith("discs_")]
    assert len(seeded) >= 4 and sum(n.startswith("ties_") for n in names) == 2
    shapes = [golden["lab_" + n].shape for n in seeded]
    assert (64, 64) in shapes and (256, 256) in shapes
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_restatement_equals_scipy_off_the_ties(golden):
    for name in _cases(golden):
        lab = golden["lab_" + name].astype(np.int64)
        d2, near, site = nearest_label(lab)
        ties = tie_mask(lab)
        if name.startswith("ties_"):  # compared against the brute-force rule only: the rule's own properties
            assert ties.mean() > 0.05
        else:
            share = ties.mean()
            print(name, "tie share %.4f" % share)
            assert share <= TIE_SHARE_CAP
            assert np.array_equal(ties, golden["tie_" + name])
            assert np.array_equal(d2, golden["d2_" + name])  # D2 everywhere
            for k, dist in enumerate(golden["distances"]):
                want = golden["exp_%s_%d" % (name, k)]
                got = expand_labels(lab, float(dist))
                assert np.array_equal(got[~ties], want[~ties]), (name, dist)
        # the rule itself: a site is its own, N carries a site's label, Q is a site of label N at distance D2
        s = lab > 0
        assert np.array_equal(near[s], lab[s]) and (d2[s] == 0).all()
        H, W = lab.shape
        qr, qc = np.divmod(site, W)
        pr, pc = np.mgrid[:H, :W]
        assert np.array_equal(lab[qr, qc], near) and np.array_equal((pr - qr) ** 2 + (pc - qc) ** 2, d2)


def test_selection_and_cap_remove_sites():
    lab = np.zeros((9, 11), np.int64)
    lab[1, 1], lab[4, 5], lab[7, 9], lab[0, 10] = 1, 2, 3, 7
    lab[8, 0] = -4
    d2, near, _ = nearest_label(lab, sel=[1, 0, 1], cap=3)
    assert set(np.unique(near)) == {1, 3} and d2[4, 5] > 0 and d2[0, 10] > 0 and d2[8, 0] > 0
    d2e, neare, sitee = nearest_label(lab, sel=[0, 0, 0], cap=3)
    assert (d2e == -1).all() and (neare == 0).all() and (sitee == -1).all()


def test_tables_on_a_hand_made_frame():
    lab = np.zeros((6, 8), np.int64)
    lab[1:3, 1:3] = 1
    lab[1:3, 3:5] = 2   # abuts 1 four-wise over two rows
    lab[3, 5] = 3       # abuts 2 only diagonally
    d2, near, _ = nearest_label(lab)
    pairs = adjacency_pairs(near, d2, 0)
    assert pairs.tolist() == [[1, 2, 2, 2]]  # reach 0: the label image itself; the diagonal pair has no link
    full = adjacency_pairs(near, d2, -1)
    assert {(a, b): ct for a, b, _, ct in full.tolist()} == {(1, 2): 2, (1, 3): 0, (2, 3): 0}
    t = territory_table(near, d2, -1, 3, mask=lab == 2)
    assert t[:, 0].sum() == lab.size and t[1, 1] == 4 and t[:, 3].tolist() == [1, 1, 1]
    t0 = territory_table(near, d2, 0, 3)
    assert t0[:, 0].tolist() == [4, 4, 1] and (t0[:, 2] == 0).all() and t0[:, 3].tolist() == [0, 0, 0]
    deg = degrees(full, np.array([0, 1, 9]), 2)
    assert deg.tolist() == [[0, 1, 0, 1], [1, 0, 1, 0], [1, 1, 0, 0]]


def test_reach_thresholds_against_sqrt():
    from particle_col_image_segmentation_amd import ops
    n_max = 2 * 1024 ** 2
    roots = np.sqrt(np.arange(n_max + 1, dtype=np.float64))
    rng = np.random.default_rng(5)
    picks = rng.integers(0, n_max + 1, 40)
    dists = [0.0, 0.5, 1.0, 1.5, np.sqrt(2.0), 2.0, 1447.9, float(roots[-1])]
    dists += [float(v) for n in picks for v in (roots[n], np.nextafter(roots[n], 0.0), np.nextafter(roots[n], np.inf))]
    n_sampled = len(dists)
    # every n of a dense range, at its root and at the floats either side of it
    dists += [float(v) for n in range(4097) for v in (roots[n], np.nextafter(roots[n], -1.0), np.nextafter(roots[n], np.inf))]
    for k, dist in enumerate(dists):
        want = int(np.searchsorted(roots, dist, side="right")) - 1  # the largest n with sqrt(n) <= dist, over ALL n <= n_max
        got = ops.reach_r2(dist)
        assert (got is None and want == -1) or got == want, (dist, got, want)
        if k < n_sampled:  # (the restatement recomputes every root per call)
            assert reach_r2(dist, n_max) == want
    assert ops.reach_r2(-1.0) is None and ops.reach_r2(float("nan")) is None and ops.reach_r2(float("inf")) == -1
    # the reach of the tables, in um: d2 <= R2 iff sqrt(d2) / scale < reach, for every d2 <= n_max
    for scale in (512.0 / 19.0, 9.95, 1.0):
        for reach in (0.05, 1.0, 3.3, 20.0, float(roots[777] / scale)):
            r2 = ops.reach_um_r2(reach, scale)
            within = roots / scale < reach
            if within.all():
                assert r2 == -1 or r2 >= n_max
            else:
                assert r2 == int(np.nonzero(within)[0].max())
    assert ops.reach_um_r2(None, 2.0) == -1
    with pytest.raises(ValueError):
        ops.reach_um_r2(0.0, 2.0)


def test_table_schema_with_territories():
    from particle_col_image_segmentation_amd.pipeline import OPTIONAL_TABLES, FramePipeline, TableSwitches
    pipe = FramePipeline()
    names = pipe.tables_.slot_names
    plain = pipe.table_columns(5)
    cols = pipe.table_columns(5, territory=True, territory_reach=2.0, refined=True)
    for k in ("territories", "adjacency", "refined_territories", "refined_adjacency"):
        assert k in cols and k not in plain and k in {t.name for t in OPTIONAL_TABLES}
    assert "refined_territories" not in pipe.table_columns(5, territory=True)
    assert cols["territories"] == (["frame", "label", "slot", "territory_px", "territory_on_px", "reach2_max", "clipped"]
                                   + ["n_adj_%s" % n for n in names] + ["n_contact_%s" % n for n in names]
                                   + ["territory_um2", "territory_on_um2"])
    assert cols["adjacency"] == ["frame", "label_a", "label_b", "slot_a", "slot_b", "border_px", "contact_px"]
    assert cols["refined_territories"] == cols["territories"] and cols["refined_adjacency"] == cols["adjacency"]
    assert TableSwitches().territory is False and TableSwitches().territory_reach is None
    kw = FramePipeline.table_kwargs("empty_device_tables", {"territory": True, "territory_reach": 1.0, "raster": 19.0})
    assert kw == {"territory": True, "territory_reach": 1.0}
    empty = pipe.empty_device_tables(5, device="cpu", territory=True, refined=True)
    assert {k: v.shape[1] for k, v in empty.items() if "territor" in k or "adjacency" in k} == {
        k: len(cols[k]) for k in ("territories", "adjacency", "refined_territories", "refined_adjacency")}
