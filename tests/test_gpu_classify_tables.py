"""Region classification (csrc/reduce.hip: classify_regions_kernel, group_reduce_kernel), the host split of the merges
(FramePipeline._merge_all) and the table assembly (csrc/tables.hip) on the crafted class maps of class_map_patterns.py:
regions at every threshold, clusters that are exact multiples of the mean cell area, every order of first appearance,
a type with clusters and no cell, more than 2048 listed regions, four type slots.

The reference is the oracle on the same map (class_map_patterns.expectation); tests/test_classify_tables_cpu.py shows
that the maps are what they are meant to be.  Everything is compared exactly but the floating-point centroids of the
merged groups (parity._compare_groups, rtol 1e-12: the oracle averages in floating point) and the cell distances
(rtol 1e-12, the suite's figure for them: the kernel's sum of squares is contracted to a fused multiply-add)."""
import types
import zlib

import numpy as np
import pytest

import class_map_patterns as cmp_
from oracle import oracle as orc
from oracle import parity

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

C = 5
# ratios of tb_ratios: two of the pipeline's, three and four denominator planes, and a numerator / a denominator plane
# that the C planes do not have (NaN)
RATIOS = (("C13act", 1, (1, 0)), ("N15act", 3, (2, 3)), ("three", 4, (4, 2, 0)), ("no_numerator", 6, (1, 0)),
          ("no_denominator", 1, (1, 7)), ("four", 0, (3, 2, 1, 0)))
BIG_ID = 2 ** 40 + 3


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")
    from particle_col_image_segmentation_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def ta():
    from particle_col_image_segmentation_amd import tiff_analysis
    return tiff_analysis


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def class_tables(ops, ta, ct):
    """ops.ClassTables of the three reference types, or with the fourth one of class_map_patterns.FOURTH"""
    names, mc, mk = list(ta.CELL_TYPES), dict(ta.MIN_CELL_AREA), dict(ta.MIN_CLUSTER_AREA)
    if ct is cmp_.CT4:
        name, a, b = cmp_.FOURTH
        names.append(name)
        mc[name], mk[name] = a, b
    return ops.ClassTables(ct, names, mc, mk)


def classify(ops, cms, tb, cap=None):
    """label_equal8 -> region_reduce(cls=cm) -> classify_regions on a batch of class maps: a FramePipeline result's
    entries of that stage"""
    cmd = dev(np.stack(cms))
    labels, counts = ops.label_equal8(cmd)
    stats, cls_out, _, overflow = ops.region_reduce(labels, counts, cls=cmd, cap=cap)
    res = dict(denoised=cmd, labels=labels, counts=counts, stats=stats, cls_out=cls_out, overflow=overflow, groups={})
    res.update(ops.classify_regions(stats, cls_out, counts, tb))
    return res


def merge_all(ops, ta, res, tb):
    """the pipeline's merges (FramePipeline._merge_all: dilated_runs_multi + merge_groups_fused_multi on the lists in
    place, at most four masks a call) into res["groups"]"""
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    pipe = FramePipeline(cmp_.CT3)
    pipe.tables_ = tb
    B, H, W = res["denoised"].shape
    res["groups"] = {}
    pipe._merge_all(types.SimpleNamespace(shape=(B, 1, H, W)), res)
    return res


def check_classification(verdict, counts, b, e, what):
    """kind, slot_of, cells, particle_area, nan_flag, type_stats, n_list and the five lists of frame ``b`` against the
    expectation ``e`` (of a NaN frame: ``cells`` where it does not depend on the missing mean)"""
    n = e["n"]
    assert int(counts[b]) == n, what
    for key in ("kind", "slot_of"):
        np.testing.assert_array_equal(host(verdict[key][b, :n]), e["classes"][key], err_msg="%s: %s" % (what, key))
    free = e.get("mean_free", np.ones(n, bool))
    np.testing.assert_array_equal(host(verdict["cells"][b, :n])[free], e["classes"]["cells"][free], err_msg="%s: cells" % what)
    assert int(verdict["particle_area"][b]) == e["particle_area"], what
    assert int(verdict["nan_flag"][b]) == int(e["nan"]), what
    np.testing.assert_array_equal(host(verdict["type_stats"][b]), e["type_stats"], err_msg="%s: type_stats" % what)
    np.testing.assert_array_equal(host(verdict["n_list"][b]), [len(l) for l in e["lists"]], err_msg="%s: n_list" % what)
    for s, lst in enumerate(e["lists"]):
        np.testing.assert_array_equal(host(verdict["region_list"][b, s, :len(lst)]), lst, err_msg="%s: list %d" % (what, s))


def check_groups(ops, res, b, e, what):
    """merged groups of frame ``b`` against the oracle (parity._compare_groups); group_reduce on the same group_of gives
    the fused call's rows"""
    parity._compare_groups(res, b, e["groups"])
    H, W = res["denoised"].shape[1:]
    for s, g in res["groups"].items():
        gs = ops.group_reduce(res["stats"], res["region_list"][:, s].contiguous(), res["n_list"][:, s].contiguous(),
                              g["group_of"], g["n_groups"], H, W)
        ng = int(g["n_groups"][b])
        assert torch.equal(gs[b, :ng], g["group_stats"][b, :ng]), "%s: group_reduce, slot %d" % (what, s)


@pytest.fixture(scope="module")
def nan_case():
    frame = cmp_.frame_nan()
    return frame, cmp_.expectation_nan(frame, cmp_.frame_nan(sibling=True))


@pytest.fixture(scope="module")
def batch3(ops, ta):
    """the three-type frames in one batch (frames 0 and 2 without a cell row), classified and merged"""
    tb = class_tables(ops, ta, cmp_.CT3)
    res = classify(ops, [f.cm for f in cmp_.frames3().values()], tb)
    return merge_all(ops, ta, res, tb), tb


@pytest.fixture(scope="module")
def batch4(ops, ta):
    tb = class_tables(ops, ta, cmp_.CT4)
    return classify(ops, [f.cm for f in cmp_.frames4().values()], tb), tb


# ------------------------------------------------------------------------------------------------------ classification
ALONE = list(cmp_.frames3()) + list(cmp_.frames4()) + ["d_nan"]


@pytest.mark.parametrize("name", ALONE)
def test_classification_alone(ops, ta, nan_case, name):
    if name == "d_nan":
        frame, e = nan_case
    elif name in cmp_.frames3():
        frame, e = cmp_.frames3()[name], cmp_.expectations3()[name]
    else:
        frame, e = cmp_.frames4()[name], cmp_.expectations4()[name]
    res = classify(ops, [frame.cm], class_tables(ops, ta, frame.cell_types))
    assert res["stats"].shape[1] == e["n"]
    check_classification(res, res["counts"], 0, e, name)
    np.testing.assert_array_equal(host(res["stats"][0, :e["n"]]), e["tab"])
    np.testing.assert_array_equal(host(res["cls_out"][0, :e["n"]]), e["cls"])


def test_classification_batch(batch3, batch4):
    (res3, _), (res4, _) = batch3, batch4
    n = [e["n"] for e in cmp_.expectations3().values()]
    assert len(set(n)) >= 6 and n[0] < n[1] > n[2]  # the frames differ in region count
    assert not cmp_.expectations3()["no_cells_particles"]["classes"]["kind"].any() and list(cmp_.frames3())[2] == "no_cells_background"
    for res, exps in ((res3, cmp_.expectations3()), (res4, cmp_.expectations4())):
        assert not host(res["overflow"]).any()
        for b, (name, e) in enumerate(exps.items()):
            check_classification(res, res["counts"], b, e, "%s in its batch" % name)
            np.testing.assert_array_equal(host(res["labels"][b]), e["label_im"], err_msg=name)


def test_rows_beyond_the_counts_are_not_read(ops, batch3):
    """The same region tables at capacity cap + 37, every row at and beyond counts[b] a cell-class region of 10^6 pixels:
    no count, list or sum changes.  (In the first run cap == max(counts), and the rows beyond the shorter frames' counts
    are whatever the allocation held.)"""
    res, tb = batch3
    B, cap = res["stats"].shape[:2]
    counts = host(res["counts"])
    assert cap == counts.max()
    stats = np.zeros((B, cap + 37, 8), np.int64)
    stats[:] = [10 ** 6, 3 * 10 ** 6, 4 * 10 ** 6, 0, 0, 7, 9, 0]
    cls_out = np.full((B, cap + 37), 1, np.uint8)
    assert tb.slot[1] == 0
    s0, c0 = host(res["stats"]), host(res["cls_out"])
    for b in range(B):
        stats[b, :counts[b]] = s0[b, :counts[b]]
        cls_out[b, :counts[b]] = c0[b, :counts[b]]
    verdict = ops.classify_regions(dev(stats), dev(cls_out), res["counts"], tb)
    for b, (name, e) in enumerate(cmp_.expectations3().items()):
        check_classification(verdict, res["counts"], b, e, "%s, poisoned rows" % name)


# -------------------------------------------------------------------------------------------------------------- merges
def test_merges_three_types(ops, batch3):
    res, _ = batch3
    assert sorted(res["groups"]) == [0, 1, 2, 4]
    for b, (name, e) in enumerate(cmp_.expectations3().items()):
        check_groups(ops, res, b, e, name)


def test_merges_four_types(ops, ta, batch4, monkeypatch):
    """Five masks: one call of four and one of one, the fifth ("combined") over the first class value of every type."""
    res, tb = batch4
    assert tb.slot_names == ["3D05", "6B07", "C3M10", cmp_.FOURTH[0]] and tb.slot_value == [1, 2, 4, 6]
    assert tb.slot[7] == 1 and tb.particle[3] and tb.particle[8]
    calls = []
    fused = ops.merge_groups_fused_multi
    monkeypatch.setattr(ops, "merge_groups_fused_multi", lambda *a: (calls.append(list(a[5])), fused(*a))[1])
    merge_all(ops, ta, res, tb)
    assert calls == [[0, 1, 2, 3], [4]]
    assert sorted(res["groups"]) == [0, 1, 2, 3, 4]
    for b, (name, e) in enumerate(cmp_.expectations4().items()):
        check_groups(ops, res, b, e, name)


# -------------------------------------------------------------------------------------------------------------- tables
def frame_inputs(name, m=None):
    """What the table assembly takes beside the classification, made up per frame (seeded by its name, so a frame brings
    the same values into every batch): plane sums of the class components and of the refined ROIs with zero
    denominators, 0 / 0, -0.0, 1e300 and subnormals among them; a refined label image of ``m`` markers of which three
    in ten have no pixel; tie flag and overlap area."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    H, W = cmp_.SHAPE

    def sums(rows=4096):
        s = rng.standard_normal((rows, C)) * 10.0 ** rng.integers(-3, 7, (rows, 1))
        p = rng.integers(0, 16, rows)
        s[p == 1, 0], s[p == 1, 1] = 0.0, 0.0            # 0 / 0
        s[p == 2, 0] = -s[p == 2, 1]                     # x / 0
        s[p == 3, 2], s[p == 3, 3] = -0.0, 0.0           # 0 / (0 + -0 + 0)
        s[p == 4, 0], s[p == 4, 1] = 1e300, 1e300
        s[p == 5, 2], s[p == 5, 3] = 0.0, 5e-324         # subnormal / itself
        s[p == 6, 1], s[p == 6, 0] = -0.0, 3.0           # -0 / 3 = -0
        s[p == 7, 3], s[p == 7, 2] = 1.5e-323, 2.0       # a quotient that is rounded among the subnormals
        return s

    cc, ws = sums(), sums()
    if m is None:
        m = 0 if name == "no_cells_background" else int(rng.integers(300, 900))
    present = rng.random(m) < 0.7
    cell = rng.permutation((H // 4) * (W // 4))[:m]
    lab = np.zeros((H, W), np.int32)
    for l in np.nonzero(present)[0]:
        r, c = divmod(int(cell[l]), W // 4)
        lab[4 * r:4 * r + 2 + l % 2, 4 * c:4 * c + 3] = l + 1
    return dict(cc=cc, ws=ws, ws_labels=lab, m=m, tie=int(rng.integers(0, 3)), overlap=int(rng.integers(0, 10 ** 7)))


def assemble(ops, res, names, frame_ids, m=None):
    """the FramePipeline result entries that build_tables reads, on top of a classified (and merged) batch"""
    B, cap = res["stats"].shape[:2]
    inp = [frame_inputs(n, m) for n in names]
    assert max(i["m"] for i in inp) <= cap <= 4096
    n_markers = dev(np.array([i["m"] for i in inp], np.int32))
    ws_labels = dev(np.stack([i["ws_labels"] for i in inp]))
    ws_stats, _, _, ws_overflow = ops.region_reduce(ws_labels, n_markers, cap=cap, zero_sums=C)
    res = dict(res)
    res.update(cc_sums=dev(np.stack([i["cc"][:cap] for i in inp])), ws_sums=dev(np.stack([i["ws"][:cap] for i in inp])),
               n_markers=n_markers, ws_labels=ws_labels, ws_stats=ws_stats, ws_overflow=ws_overflow,
               tie_flags=dev(np.array([i["tie"] for i in inp], np.int32)),
               overlap_area=dev(np.array([i["overlap"] for i in inp], np.int64)))
    return res, inp, dev(np.array(frame_ids, np.int64))


def ratio_columns(s):
    """the denominators added in order starting from 0.0, then one division; NaN where a plane does not exist"""
    out = np.full((s.shape[0], len(RATIOS)), np.nan)
    with np.errstate(all="ignore"):
        for k, (_, num, den) in enumerate(RATIOS):
            if num >= C or any(p >= C for p in den):
                continue
            d = np.zeros(s.shape[0])
            for p in den:
                d = d + s[:, p]
            out[:, k] = s[:, num] / d
    return out


def expected_tables(res, inp, frame_ids, exps):
    """rois / cells / groups / frames as documented at the head of csrc/tables.hip, in plain numpy: from the host copies
    of the inputs, and the ``frames`` record from the oracle (``exps[b]`` None: a frame to leave out)"""
    h = {k: host(res[k]) for k in ("counts", "stats", "cls_out", "kind", "cells", "region_list", "n_list", "cc_sums", "ws_sums")}
    groups = {s: {k: host(v) for k, v in g.items()} for s, g in res["groups"].items()}
    cap = h["stats"].shape[1]
    rois, cells, grp, frames = [], [], [], []
    for b, fid in enumerate(frame_ids):
        n, i = min(int(h["counts"][b]), cap), inp[b]
        # rois: the refined labels with a pixel, ascending
        rr, cc_ = np.nonzero(i["ws_labels"])
        l = i["ws_labels"][rr, cc_]
        area = np.bincount(l, minlength=i["m"] + 1)[1:]
        sr = np.bincount(l, weights=rr, minlength=i["m"] + 1)[1:].astype(np.int64)
        sc = np.bincount(l, weights=cc_, minlength=i["m"] + 1)[1:].astype(np.int64)
        keep = np.nonzero(area)[0]
        assert i["m"] < 100 or 0 < len(keep) < i["m"]  # (labels without a pixel: the compaction skips rows)
        a = area[keep].astype(np.float64)
        s = h["ws_sums"][b, keep]
        rois.append(np.column_stack([np.full(len(keep), float(fid)), keep + 1.0, a, sr[keep] / a, sc[keep] / a, s, ratio_columns(s)]))
        # cells: the regions of kind >= 1, ascending; group columns scattered from the lists
        own, comb = np.zeros(cap, np.int64), np.zeros(cap, np.int64)
        for sl, g in groups.items():
            k = int(h["n_list"][b, sl])
            (comb if sl == 4 else own)[h["region_list"][b, sl, :k]] = g["group_of"][b, :k]
        keep = np.nonzero(h["kind"][b, :n])[0]
        st = h["stats"][b, keep]
        a = st[:, 0].astype(np.float64)
        s = h["cc_sums"][b, keep]
        cells.append(np.column_stack([np.full(len(keep), float(fid)), keep + 1.0, h["cls_out"][b, keep], h["kind"][b, keep], a,
                                      st[:, 1] / a, st[:, 2] / a, st[:, 3:7], h["cells"][b, keep], own[keep], comb[keep], s,
                                      ratio_columns(s)]))
        for sl in sorted(groups):
            ng = int(groups[sl]["n_groups"][b])
            t = groups[sl]["group_stats"][b, :ng]
            a = t[:, 0].astype(np.float64)
            grp.append(np.column_stack([np.full(ng, float(fid)), np.full(ng, float(sl)), np.arange(ng) + 1.0, a, t[:, 1] / a,
                                        t[:, 2] / a, t[:, 3:8]]))
        e = exps[b]
        if e is not None:
            rec = [n, i["m"], e["particle_area"], e["particle_area"] + i["overlap"], i["tie"]]
            for sl in range(4):
                name = e["names"][sl] if sl < len(e["names"]) else None
                rec += [1, e["counts"][0][name], e["area_px"][name]] if name in e["order"] else [0, 0, 0]
            frames.append(rec)
    return np.concatenate(rois), np.concatenate(cells), np.concatenate(grp), np.array(frames, np.int64)


def assert_same(got, exp, what):
    """equal, NaN at the same places, zeros of the same sign"""
    got, exp = np.asarray(got), np.asarray(exp)
    np.testing.assert_array_equal(got, exp, err_msg=what)
    np.testing.assert_array_equal(np.signbit(got[~np.isnan(exp)]), np.signbit(exp[~np.isnan(exp)]), err_msg=what + " (signs)")


def rows_of(tabs, fids):
    """the rows of ``fids`` in every table of a build_tables result, as numpy"""
    fids = [float(f) for f in fids]
    out = {k: host(tabs[k]) for k in ("rois", "cells", "groups")}
    out = {k: v[np.isin(v[:, 0], fids)] for k, v in out.items()}
    return out


@pytest.fixture(scope="module")
def tables3(ops, batch3):
    res, tb = batch3
    names = list(cmp_.frames3())
    frame_ids = [3 + 17 * b * b for b in range(len(names))]
    frame_ids[1] = BIG_ID
    res, inp, fid = assemble(ops, res, names, frame_ids)
    tabs = ops.build_tables(res, res["groups"], fid, C, RATIOS, check=True, distance_slots=tb.slot)
    return res, inp, frame_ids, tabs, tb


def test_tables_bit_for_bit(tables3):
    res, inp, frame_ids, tabs, _ = tables3
    exps = list(cmp_.expectations3().values())
    rois, cells, grp, frames = expected_tables(res, inp, frame_ids, exps)
    assert not host(res["ws_overflow"]).any()
    # the special values made it into rows that are written
    assert np.isnan(cells[:, 14 + C]).any() and np.isinf(cells[:, 14 + C]).any() and np.isnan(rois[:, 5 + C]).any()
    assert np.isnan(cells[:, 14 + C + 3:14 + C + 5]).all() and (cells[:, 14 + C + 1] == 1e-323).any()
    assert np.signbit(cells[cells[:, 14 + C] == 0, 14 + C]).any()
    assert len(rois) > 256 * 8 and len(cells) > 256 * 8
    assert_same(host(tabs["rois"]), rois, "rois")
    assert_same(host(tabs["cells"]), cells, "cells")
    assert_same(host(tabs["groups"]), grp, "groups")
    np.testing.assert_array_equal(host(tabs["frames"]), frames, err_msg="frames")
    # a type present only through regions below the minimum cell area: present, 0, 0
    b = list(cmp_.frames3()).index("a_absent")
    assert frames[b, 5 + 3:5 + 6].tolist() == [1, 0, 0] and frames[b, 5 + 6:5 + 9].tolist() == [0, 0, 0]
    # frames 0 and 2 have no cell row and the frames after them start where they should
    assert not np.isin(cells[:, 0], [frame_ids[0], frame_ids[2]]).any()


def test_tables_groups_against_the_oracle(tables3):
    res, inp, frame_ids, tabs, _ = tables3
    refs = [{"groups": e["groups"]} for e in cmp_.expectations3().values()]
    assert parity.compare_tables({"groups": host(tabs["groups"]), "cells": host(tabs["cells"])}, frame_ids, refs) == len(refs)


def test_cell_distances(tables3):
    """.m:260-268 between the rows of type slot 0 and of slot 1; NaN for the rows of other types and for every row of a
    frame without one of the two"""
    res, inp, frame_ids, tabs, tb = tables3
    cells, dist = host(tabs["cells"]), host(tabs["cell_dist"])
    assert dist.shape == (len(cells),)
    with_both = []
    for name, fid in zip(cmp_.frames3(), frame_ids):
        sel = np.nonzero(cells[:, 0] == fid)[0]
        slot = tb.slot[cells[sel, 2].astype(np.int64)]
        a, b = sel[slot == 0], sel[slot == 1]
        exp = np.full(len(sel), np.nan)
        if len(a) and len(b):
            with_both.append(name)
            xy = lambda rows: np.stack([cells[rows, 6] + 1.0, cells[rows, 5] + 1.0], 1)
            near = orc.nearest_distances(xy(a), xy(b))
            exp[np.searchsorted(sel, a)] = near[:len(a)]
            exp[np.searchsorted(sel, b)] = near[len(a):]
        np.testing.assert_array_equal(np.isnan(dist[sel]), np.isnan(exp), err_msg=name)
        np.testing.assert_allclose(dist[sel], exp, rtol=1e-12, atol=0, err_msg=name)
        if name in ("a_thresholds", "e_many"):
            assert (slot > 1).any() and np.isnan(exp).any() and not np.isnan(exp).all()
    assert "a_thresholds" in with_both and "e_many" in with_both and "a_absent" not in with_both
    assert (cells[:, 0] == frame_ids[list(cmp_.frames3()).index("a_absent")]).any()


def small_batch(ops, ta, names, frames, frame_ids, cap=None, m=10):
    tb = class_tables(ops, ta, cmp_.CT3)
    res = merge_all(ops, ta, classify(ops, [frames[n].cm for n in names], tb, cap=cap), tb)
    return assemble(ops, res, names, frame_ids, m=m)


def test_nan_frame_in_a_batch(ops, ta, nan_case):
    """a type with clusters and no cell between two good frames: its flag alone is set, check=True raises what the
    reference raises, and with check=False the good frames' rows are those of the batch without it"""
    frame, e = nan_case
    frames = dict(cmp_.frames3(), d_nan=frame)
    res, inp, fid = small_batch(ops, ta, ["a_thresholds", "d_nan", "c_order_124"], frames, [5, 9, BIG_ID])
    assert host(res["nan_flag"]).tolist() == [0, 1, 0]
    check_classification(res, res["counts"], 1, e, "d_nan in a batch")
    for b, name in ((0, "a_thresholds"), (2, "c_order_124")):
        check_classification(res, res["counts"], b, cmp_.expectations3()[name], name)
    with pytest.raises(ValueError, match="cannot convert float NaN to integer"):
        ops.build_tables(res, res["groups"], fid, C, RATIOS, check=True)
    tabs = ops.build_tables(res, res["groups"], fid, C, RATIOS, check=False)
    res2, inp2, fid2 = small_batch(ops, ta, ["a_thresholds", "c_order_124"], frames, [5, BIG_ID])
    tabs2 = ops.build_tables(res2, res2["groups"], fid2, C, RATIOS, check=True)
    got, want = rows_of(tabs, [5, BIG_ID]), rows_of(tabs2, [5, BIG_ID])
    for k in want:
        assert len(want[k]) > 0
        assert_same(got[k], want[k], k)
    np.testing.assert_array_equal(host(tabs["frames"])[[0, 2]], host(tabs2["frames"]))
    # the NaN frame's own rows are written like any other (`cells` of its clusters without a mean: what the kernel left)
    exps = [cmp_.expectations3()["a_thresholds"], None, cmp_.expectations3()["c_order_124"]]
    rois, cells, grp, _ = expected_tables(res, inp, [5, 9, BIG_ID], exps)
    assert (cells[:, 0] == 9).sum() == np.count_nonzero(e["classes"]["kind"]) > 0
    assert_same(host(tabs["cells"]), cells, "cells with the NaN frame")
    assert_same(host(tabs["rois"]), rois, "rois with the NaN frame")
    assert_same(host(tabs["groups"]), grp, "groups with the NaN frame")


def test_overflow(ops, ta):
    """one frame with more regions than the table holds: its flag alone is set, check=True raises the capacity error,
    with check=False the other frames' rows are those of a batch whose table holds everything"""
    names, ids = ["a_thresholds", "e_many", "a_absent"], [4, 6, BIG_ID]
    res, inp, fid = small_batch(ops, ta, names, cmp_.frames3(), ids, cap=100)
    assert host(res["overflow"]).tolist() == [0, 1, 0] and int(res["counts"][1]) > 100
    with pytest.raises(RuntimeError, match="capacity"):
        ops.build_tables(res, res["groups"], fid, C, RATIOS, check=True)
    tabs = ops.build_tables(res, res["groups"], fid, C, RATIOS, check=False)
    res2, inp2, fid2 = small_batch(ops, ta, names, cmp_.frames3(), ids)
    tabs2 = ops.build_tables(res2, res2["groups"], fid2, C, RATIOS, check=True)
    got, want = rows_of(tabs, [4, BIG_ID]), rows_of(tabs2, [4, BIG_ID])
    for k in want:
        assert len(want[k]) > 0
        assert_same(got[k], want[k], k)
    np.testing.assert_array_equal(host(tabs["frames"])[[0, 2]], host(tabs2["frames"])[[0, 2]])
    assert host(tabs["frames"])[1, 0] == 100  # (the overflowed frame's record counts the rows the table holds)


# ------------------------------------------------------------------------------------------------------------- drop-in
DROP_IN = [n for n in cmp_.frames3() if n[:2] in ("a_", "b_", "c_")]


@pytest.mark.parametrize("name", DROP_IN)
def test_drop_in(ta, name):
    frame, e = cmp_.frames3()[name], cmp_.expectations3()[name]
    cell_pos, cell_clusters, particle_area, merged = ta.get_cell_positions_and_areas(frame.cm, frame.cell_types, merged=True)
    assert list(cell_pos) == e["order"] and list(cell_clusters) == e["order"]
    assert particle_area == e["particle_area"]
    for t in e["order"]:
        for got, exp in ((cell_pos[t], e["cell_pos"][t]), (cell_clusters[t], e["cell_clusters"][t])):
            assert [r.label for r in got] == [r.label for r in exp]
            assert [r.area for r in got] == [r.area for r in exp]
            assert [getattr(r, "cells", None) for r in got] == [getattr(r, "cells", None) for r in exp]
    assert list(merged) == list(e["merged"]) == e["order"] + ["combined"]
    for t, groups in e["merged"].items():
        assert [[r.label for r in g["regions"]] for g in merged[t]] == [[r.label for r in g["regions"]] for g in groups], t
        assert [g["area"] for g in merged[t]] == [g["area"] for g in groups]
        assert [tuple(g["bbox"]) for g in merged[t]] == [tuple(g["bbox"]) for g in groups]
        if groups:
            np.testing.assert_allclose([g["centroid"] for g in merged[t]], [g["centroid"] for g in groups], rtol=1e-12, atol=0)
    got = ta.get_cell_counts_and_densities(cell_pos, cell_clusters, particle_area)
    for g, x in zip(got, e["counts"]):
        assert list(g) == list(x) and g == x


def test_drop_in_nan(ta, nan_case):
    frame, _ = nan_case
    with pytest.raises(ValueError, match="cannot convert float NaN to integer"):
        ta.get_cell_positions_and_areas(frame.cm, frame.cell_types, merged=True)
    with pytest.raises(ValueError, match="cannot convert float NaN to integer"):
        ta.get_cell_positions_and_areas(frame.cm, frame.cell_types)
