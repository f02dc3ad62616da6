"""What an OUTPUT buffer held before a call must never reach the call's result, and nothing outside an output is written: the
prior states an output is put into, and the cases that drive every compute entry of ``_lib.SIGNATURES`` (no tests in here;
``test_output_cases_cpu.py`` checks this module, ``test_gpu_output_state.py`` runs it).

The cases are those of tests/workspace_cases.py -- with the entries they drive that take no workspace declared on top -- and
per-op cases for the entries no workspace case reaches.  A case is what workspace_cases.py says it is; in addition ``run`` may
return, under the key ``_raw``, a dict name -> ``(tensor, defined)``: an output as the library left it and a bool tensor over
its leading dimensions, True where the call defines the element.  include/pcseg.h promises that the rest is NOT WRITTEN: it
must still hold the fill it was handed out with."""
import numpy as np

import workspace_cases as wc

OUTPUT_STATES = ("zeros", "ones", "unit")  # in the order they are run
UNIT_DTYPES = (np.uint8, np.uint16, np.int32, np.int64, np.float32, np.float64)


# ------------------------------------------------------------------ states of an output
def fill_pattern(state, dtype):
    """The bytes of one element of ``dtype`` in ``state``: uint8 (itemsize,).  zeros: what fresh device memory tends to hold;
    ones: every byte 0xFF (NaN in float64, -1 in int32, 255 in uint8); unit: the value 1 of the dtype itself -- a flag never
    cleared reads "set", a mask pixel never written "inside", a count never stored 1."""
    dt = np.dtype(dtype)
    if state == "zeros":
        return np.zeros(dt.itemsize, np.uint8)
    if state == "ones":
        return np.full(dt.itemsize, 0xFF, np.uint8)
    if state == "unit":
        return np.ones(1, dt).view(np.uint8).copy()
    raise ValueError(state)


def zone_pattern(state, dtype):
    """... and of the red zones around it: they continue the fill, except under zeros, where they are 0xFF (a stray zero
    write shows too)."""
    return fill_pattern("ones" if state == "zeros" else state, dtype)


def output_fill(state, dtype, nbytes):
    """The whole buffer of an output of ``nbytes``: uint8 ``[RED_ZONE front][body][RED_ZONE back]``.  RED_ZONE is a multiple
    of 256 and of every itemsize: the body starts as well aligned as the buffer, and the element pattern runs through."""
    item = np.dtype(dtype).itemsize
    assert nbytes % item == 0 and wc.RED_ZONE % 256 == 0 and wc.RED_ZONE % item == 0
    zone = np.tile(zone_pattern(state, dtype), wc.RED_ZONE // item)
    return np.concatenate([zone, np.tile(fill_pattern(state, dtype), nbytes // item), zone])


# ------------------------------------------------------------------ helpers of the runners
def _below(n, cap):
    """bool (B, cap): the rows of every frame below its count"""
    import torch
    return torch.arange(cap, device=n.device)[None, :] < n.to(torch.int64)[:, None]


def _run_tops(bits, H):
    """bool (..., H, W) from the 32-row column words (..., ceil(H / 32), W): the top pixel of every vertical run of set bits
    within its word -- the only entries of ``run_parent`` that are written (include/pcseg.h)"""
    import torch
    words = bits.to(torch.int64) & 0xFFFFFFFF
    shifts = torch.arange(32, device=bits.device).reshape(32, 1)
    m = ((words[..., :, None, :] >> shifts) & 1).bool()                     # (..., words, 32, W)
    above = torch.zeros_like(m)
    above[..., 1:, :] = m[..., :-1, :]                                      # (bit 0 of a word has no pixel above it in the word)
    top = m & ~above
    return top.reshape(top.shape[:-3] + (-1, top.shape[-1]))[..., :H, :]


def _oracle():
    return wc._oracle()


_eq = wc._eq


def _bits_eq(got, want, what):
    """float64 tables by their bits: NaN rows and infinities included"""
    _eq(np.ascontiguousarray(got, np.float64).view(np.uint64), np.ascontiguousarray(want, np.float64).view(np.uint64), what)


# ------------------------------------------------------------------ front-end operators on their own
def build_frontend(shape, seed):
    return {"stack": wc.build_classmap(5)(shape, seed)["stack"], "img": wc.build_edt_lt(shape, seed)["img"]}


def run_frontend(ops, x):
    cm = ops.argmax_planes(x["stack"])
    mask = ops.threshold_lt(x["img"], 0.5)
    return {"class_map": cm, "denoised": ops.median5(cm), "mask": mask, "eroded": ops.morph3x3(mask, True),
            "dilated": ops.morph3x3(mask, False)}


def check_frontend(x, out):
    orc = _oracle()
    for b, st in enumerate(x["stack"]):
        cm = (np.argmax(st, axis=0) + 1).astype(np.uint8)
        _eq(out["class_map"][b], cm, "class map, frame %d" % b)
        _eq(out["denoised"][b], orc.median_filter(cm), "denoised, frame %d" % b)
        mask = x["img"][b] < np.float32(0.5)
        _eq(out["mask"][b].astype(bool), mask, "mask, frame %d" % b)
        _eq(out["eroded"][b].astype(bool), orc.morph3x3(mask, 1), "eroded, frame %d" % b)
        _eq(out["dilated"][b].astype(bool), orc.morph3x3(mask, 0), "dilated, frame %d" % b)
    assert out["mask"][-1].all() and not out["mask"][0].all()


def build_otsu(shape, seed):
    img = wc._rng(shape, seed, 40).random(shape).astype(np.float32)
    img[0] *= np.float32(37.0)  # every frame keeps its own [min, max]
    img[-1] = 0.25              # a constant frame
    return {"img": img}


def run_otsu(ops, x):
    thr, hist, lohi = ops.threshold_otsu(x["img"], return_hist=True)
    hist_alone, lohi_alone = ops.otsu_hist(x["img"])
    return {"thr": thr, "hist": hist, "lohi": lohi, "hist_alone": hist_alone, "lohi_alone": lohi_alone}


def check_otsu(x, out):
    orc = _oracle()
    for b, img in enumerate(x["img"]):
        t, h = orc.threshold_otsu(img)
        assert float(out["thr"][b]) == t, b
        _eq(out["hist"][b], h, "histogram, frame %d" % b)
        _eq(out["lohi"][b], [img.min(), img.max()], "range, frame %d" % b)
    _eq(out["hist_alone"], out["hist"], "the histogram on its own")
    _eq(out["lohi_alone"], out["lohi"], "the range on its own")


# ------------------------------------------------------------------ region tables and plane sums
SUM_CLASSES = (1 << 1) | (1 << 2)
SUMS_C = 3
CAP_LOW = 40     # below the label count of every frame but the last: their overflow flag is raised, the last frame's is not
CAP_SPARE = 8    # ... and a table that many rows higher than the largest count: rows no frame fills


def _planes(shape, seed, salt):
    """float32 (B, SUMS_C, H, W) of multiples of 1 / 64 below 1: a float64 sum of fewer than 2^40 of them is exact in any
    order, so the sums tables are compared bit for bit (workspace_cases.PIPELINE_UNORDERED)"""
    B, H, W = shape
    return (wc._rng(shape, seed, salt).integers(0, 64, (B, SUMS_C, H, W)) / 64.0).astype(np.float32)


def build_plane_sums(shape, seed):
    orc = _oracle()
    cm = wc._class_map(shape, seed, 41)
    labs = np.stack([orc.label(c) for c in cm]).astype(np.int32)
    counts = np.array([int(l.max()) for l in labs], np.int32)
    assert counts[:-1].min() > CAP_LOW > counts[-1] > 0, counts
    return {"cm": cm, "labels": labs, "counts": counts, "planes": _planes(shape, seed, 42)}


def run_plane_sums(ops, x):
    torch = ops.torch  # (inside a pass of the output hooks: the padded allocations)
    cm, labels, counts, planes = x["cm"], x["labels"], x["counts"], x["planes"]
    B, H, W = labels.shape
    dev = labels.device
    out, raw = {}, {}

    def tables(cap):
        return (torch.empty((B, cap, 8), dtype=torch.int64, device=dev), torch.empty((B, cap), dtype=torch.uint8, device=dev),
                torch.empty((B, cap, SUMS_C), dtype=torch.float64, device=dev), torch.empty((B,), dtype=torch.int32, device=dev))

    def keep(tag, res, n, cap):
        defined = _below(n, cap)
        for name, t in zip(("stats", "cls_out", "sums"), res[:3]):
            if t is not None:
                out["%s_%s" % (name, tag)] = wc._rows_upto(t, n)
                raw["%s_%s" % (name, tag)] = (t, defined)
        out["overflow_" + tag] = res[3]

    for tag, cap in (("low", CAP_LOW), ("high", int(counts.max().item()) + CAP_SPARE)):
        # pcseg_region_reduce_sel through the wrapper: every pixel, then the classes 1 and 2 only
        keep("sel_all_" + tag, ops.region_reduce(labels, counts, cls=cm, planes=planes, cap=cap), counts, cap)
        keep("sel_" + tag, ops.region_reduce(labels, counts, cls=cm, planes=planes, cap=cap, sum_classes=SUM_CLASSES), counts, cap)
        res = tables(cap)
        ops._call("region_reduce_n", labels, counts, cm, planes, SUMS_C, B, H, W, cap, *res)
        keep("n_" + tag, res, counts, cap)
        res = tables(cap)  # without counts every row is initialised: the whole table is defined
        ops._call("region_reduce", labels, cm, planes, SUMS_C, B, H, W, cap, *res)
        out.update(("%s_every_%s" % (name, tag), t) for name, t in zip(("stats", "cls_out", "sums", "overflow"), res))
        stats, sums, overflow = ops.region_init(counts, cap, SUMS_C, (B, H, W), dev)
        keep("init_" + tag, (stats, None, sums, overflow), counts, cap)
    out["_raw"] = raw
    return out


def _expected_tables(orc, lab, cm, planes, bits=0):
    """(region table, class at the first pixel, plane sums under the classes in ``bits``) of one frame, every label"""
    tab = orc.region_table(lab)
    sel = lab if not bits else np.where(np.isin(cm, [v for v in range(64) if (bits >> v) & 1]), lab, 0)
    return tab, cm.ravel()[tab[:, 7]], orc.channel_sums(sel, planes, n=len(tab))


def check_plane_sums(x, out):
    orc = _oracle()
    counts = x["counts"]
    for b, lab in enumerate(x["labels"]):
        tab, first, sums = _expected_tables(orc, lab, x["cm"][b], x["planes"][b])
        _, _, sums_sel = _expected_tables(orc, lab, x["cm"][b], x["planes"][b], SUM_CLASSES)
        assert b or (sums_sel.any() and (sums_sel != sums).any()), "the class selection selects everything or nothing"
        for tag, cap in (("low", CAP_LOW), ("high", int(counts.max()) + CAP_SPARE)):
            k = min(int(counts[b]), cap)
            for route, want in (("sel_all", sums), ("sel", sums_sel), ("n", sums), ("every", sums)):
                name = "%s_%s" % (route, tag)
                _eq(out["stats_" + name][b, :k], tab[:k], "stats %s, frame %d" % (name, b))
                _eq(out["cls_out_" + name][b, :k], first[:k], "cls_out %s, frame %d" % (name, b))
                _eq(out["sums_" + name][b, :k], want[:k], "sums %s, frame %d" % (name, b))
                assert int(out["overflow_" + name][b]) == int(counts[b] > cap), (name, b)
            assert not out["stats_every_" + tag][b, k:, 0].any() and not out["sums_every_" + tag][b, k:].any(), (tag, b)
            # the neutral rows: no area, no centroid sums, an empty bounding box -- and a cleared flag
            neutral = out["stats_init_" + tag][b, :k]
            assert not neutral[:, :3].any() and (neutral[:, 3] >= neutral[:, 5]).all() and (neutral[:, 4] >= neutral[:, 6]).all(), (tag, b)
            assert not out["sums_init_" + tag][b, :k].any() and not out["overflow_init_" + tag][b], (tag, b)


SUMS2_SHAPES = (wc.SECOND, (2, 70, 132))  # the fused pass takes W % 4 == 0 only: full tiles, and ragged ones


def build_plane_sums2(shape, seed):
    orc = _oracle()
    x = build_plane_sums(shape, seed)
    other = wc._rng(shape, seed, 43).random(shape) < 0.3  # (below the percolation threshold: hundreds of small components)
    other[-1] = False  # image B has no label in the last frame
    lb = np.stack([orc.label(m) for m in other]).astype(np.int32)
    x.update(labels_b=lb, counts_b=np.array([int(l.max()) for l in lb], np.int32))
    assert x["counts_b"][:-1].min() > CAP_LOW and shape[2] % 4 == 0
    return x


def run_plane_sums2(ops, x):
    la, lb, ca, cb, cm = x["labels"], x["labels_b"], x["counts"], x["counts_b"], x["cm"]
    cap_a = int(ca.max().item()) + CAP_SPARE
    stats_a, _, sums_a, overflow_a = ops.region_reduce(la, ca, cls=cm, cap=cap_a, zero_sums=SUMS_C)
    stats_b, sums_b, overflow_b = ops.region_init(cb, CAP_LOW, SUMS_C, tuple(lb.shape), lb.device)
    ops.region_sums2(la, cm, SUM_CLASSES, sums_a, lb, sums_b, x["planes"], stats_b=stats_b, overflow_b=overflow_b)
    da, db = _below(ca, cap_a), _below(cb, CAP_LOW)
    return {"stats_a": wc._rows_upto(stats_a, ca), "sums_a": wc._rows_upto(sums_a, ca), "overflow_a": overflow_a,
            "stats_b": wc._rows_upto(stats_b, cb), "sums_b": wc._rows_upto(sums_b, cb), "overflow_b": overflow_b,
            "_raw": {"stats_a": (stats_a, da), "sums_a": (sums_a, da), "stats_b": (stats_b, db), "sums_b": (sums_b, db)}}


def check_plane_sums2(x, out):
    orc = _oracle()
    for b in range(x["labels"].shape[0]):
        tab, _, sums = _expected_tables(orc, x["labels"][b], x["cm"][b], x["planes"][b], SUM_CLASSES)
        k = int(x["counts"][b])
        _eq(out["stats_a"][b, :k], tab, "stats of image A, frame %d" % b)
        _eq(out["sums_a"][b, :k], sums, "sums of image A, frame %d" % b)
        tab, _, sums = _expected_tables(orc, x["labels_b"][b], x["cm"][b], x["planes"][b])
        k = min(int(x["counts_b"][b]), CAP_LOW)
        _eq(out["stats_b"][b, :k], tab[:k], "stats of image B, frame %d" % b)
        _eq(out["sums_b"][b, :k], sums[:k], "sums of image B, frame %d" % b)
        assert int(out["overflow_b"][b]) == int(x["counts_b"][b] > CAP_LOW) and not out["overflow_a"][b], b


# ------------------------------------------------------------------ the per-ROI tables and their derived columns
def build_roi_tables(shape, seed):
    labels = wc._labels(shape, seed, 44, 9, 40, zero=0.35)
    return {"labels": labels, "counts": labels.reshape(shape[0], -1).max(axis=1).astype(np.int32)}


def run_roi_tables(ops, x):
    labels, counts = x["labels"], x["counts"]
    cap = max(int(counts.max().item()), 1)
    stats, _, _, _ = ops.region_reduce(labels, counts, cap=cap)
    shape, shape_overflow = ops.region_shape(labels, counts, cap=cap)
    hull, hull_overflow = ops.region_hull(labels, counts, stats, cap=cap)
    peel, iters = ops.thin_labels(labels)
    skeleton = ops.region_skeleton(labels, peel, counts, cap=cap)
    tables = {"stats": stats, "shape": shape, "shape_props": ops.shape_properties(stats, shape, counts), "hull": hull,
              "hull_props": ops.hull_properties(stats, hull, counts), "skeleton": skeleton,
              "skeleton_props": ops.skeleton_properties(stats, skeleton, counts)}
    out = {k: wc._rows_upto(v, counts) for k, v in tables.items()}  # rows of the labels 1 .. min(counts[b], cap)
    out.update(shape_overflow=shape_overflow, hull_overflow=hull_overflow, peel=peel, iters=iters)
    out["_raw"] = {k: (v, _below(counts, cap)) for k, v in tables.items()}
    return out


def check_roi_tables(x, out):
    import test_hull_cpu as hc
    import test_shape_cpu as sc
    import test_skeleton_cpu as kc
    for b, lab in enumerate(x["labels"]):
        n = int(x["counts"][b])
        stats, shape = sc.region_table(lab, n), sc.shape_table(lab, n)
        live = stats[:, 0] > 0
        _eq(out["stats"][b, :n][live], stats[live], "stats, frame %d" % b)
        _eq(out["shape"][b, :n], shape, "shape, frame %d" % b)
        props = out["shape_props"][b, :n]
        assert np.isnan(props[~live]).all(), b
        dev = sc.deviation(props[live], sc.exact_properties(stats[live], shape[live]))
        assert (dev <= 1.0).all(), ("shape properties, frame %d" % b, dev.max(axis=0))
        hull = hc.hull_table(lab, n)
        _eq(out["hull"][b, :n], hull, "hull, frame %d" % b)
        _bits_eq(out["hull_props"][b, :n], hc.hull_properties(hc.areas(lab, n), hull), "hull properties, frame %d" % b)
        peel, iters = kc.peel_image(lab)
        _eq(out["peel"][b], peel, "peel, frame %d" % b)
        assert int(out["iters"][b]) == int(iters), b
        skeleton = kc.skeleton_table(lab, peel, n)
        _eq(out["skeleton"][b, :n], skeleton, "skeleton, frame %d" % b)
        _bits_eq(out["skeleton_props"][b, :n], kc.skeleton_properties(kc.areas(lab, n), skeleton), "skeleton properties, frame %d" % b)
    assert not out["shape_overflow"].any() and not out["hull_overflow"].any()


# ------------------------------------------------------------------ territories
TERRITORY_R2 = 20


def build_territory(shape, seed):
    x = wc.build_nearest(shape, seed)
    x["mask"] = (wc._rng(shape, seed, 45).random(shape) < 0.5).astype(np.uint8)
    return x


def run_territory(ops, x):
    d2, near, _ = ops.nearest_label(x["labels"], x["sel"], wc.NEAREST_CAP)
    return {"owned": ops.territory_labels(near, d2, TERRITORY_R2), "owned_unbounded": ops.territory_labels(near, d2),
            "rows": ops.territory_reduce(near, d2, x["mask"], TERRITORY_R2, wc.NEAREST_CAP),
            "rows_unbounded": ops.territory_reduce(near, d2, None, -1, wc.NEAREST_CAP),
            "expanded": ops.expand_labels(x["labels"], 2.5)}


def check_territory(x, out):
    import test_territory_cpu as tc
    for b, lab in enumerate(x["labels"]):
        d2, near, _ = tc.nearest_label(lab, x["sel"][b], wc.NEAREST_CAP)
        _eq(out["owned"][b], tc.owned(near, d2, TERRITORY_R2), "owned, frame %d" % b)
        _eq(out["owned_unbounded"][b], tc.owned(near, d2, -1), "owned (unbounded), frame %d" % b)
        _eq(out["rows"][b], tc.territory_table(near, d2, TERRITORY_R2, wc.NEAREST_CAP, x["mask"][b]), "rows, frame %d" % b)
        _eq(out["rows_unbounded"][b], tc.territory_table(near, d2, -1, wc.NEAREST_CAP), "rows (unbounded), frame %d" % b)
        _eq(out["expanded"][b], tc.expand_labels(lab, 2.5), "expanded, frame %d" % b)
    assert not out["rows"][-1].any() and out["rows"][0].any()


# ------------------------------------------------------------------ h-extrema
HMAX_H_INT, HMAX_H_FLOAT, HMAX_H_EDT = 2, 0.5, 1.0


def build_hmax(shape, seed):
    orc = _oracle()
    rng = wc._rng(shape, seed, 46)
    img = wc._blocks(rng, shape, 3, 9, 0.2).astype(np.int32)
    img[-1] = 4  # a constant frame: its range is below h, it has no extremum
    fimg = img.astype(np.float64) / 4.0 + rng.integers(0, 2, shape) * 0.125
    fimg[-1] = 1.25
    inside = wc._blocks(rng, shape, 12, 1, 0.4) > 0
    inside[-1] = False  # ... and a distance map that is zero everywhere
    d2 = np.stack([orc.edt_sq(m) if m.any() else np.zeros(m.shape, np.int64) for m in inside]).astype(np.int32)
    return {"img": img, "fimg": fimg, "d2": d2}


def run_hmax(ops, x):
    is_max, markers, counts, flags = ops.edt_maxima(x["d2"], HMAX_H_EDT)
    return {"i32_maxima": ops.h_maxima(x["img"], HMAX_H_INT), "i32_minima": ops.h_minima(x["img"], HMAX_H_INT),
            "f64_maxima": ops.h_maxima(x["fimg"], HMAX_H_FLOAT), "f64_minima": ops.h_minima(x["fimg"], HMAX_H_FLOAT),
            "edt_maxima": is_max, "edt_markers": markers, "edt_counts": counts, "edt_flags": flags}


def check_hmax(x, out):
    from test_reconstruct_cpu import h_extrema_np
    orc = _oracle()
    for b in range(x["img"].shape[0]):
        for name, img, h in (("i32", x["img"][b], HMAX_H_INT), ("f64", x["fimg"][b], HMAX_H_FLOAT)):
            _eq(out[name + "_maxima"][b], h_extrema_np(img, h), "%s maxima, frame %d" % (name, b))
            _eq(out[name + "_minima"][b], h_extrema_np(img, h, minima=True), "%s minima, frame %d" % (name, b))
        want = h_extrema_np(np.sqrt(x["d2"][b].astype(np.float64)), HMAX_H_EDT)
        _eq(out["edt_maxima"][b], want, "maxima of the distance, frame %d" % b)
        lab, n = orc.label(want.astype(bool), return_num=True)
        _eq(out["edt_markers"][b], lab, "markers, frame %d" % b)
        assert int(out["edt_counts"][b]) == n, b
    assert not out["edt_flags"].any() and out["edt_maxima"][0].any() and out["i32_maxima"][0].any() and out["f64_minima"][0].any()
    assert not out["edt_maxima"][-1].any() and not out["i32_maxima"][-1].any() and not out["f64_maxima"][-1].any()


# ------------------------------------------------------------------ nearest distance between two point sets
def build_nearest_dist(shape, seed):
    """two point sets on a half-pixel lattice below 2^7: the squared differences, their sum and the correctly rounded square
    root are the same float64 on the host and on the device -- the brute-force reference is compared bit for bit"""
    rng = wc._rng(shape, seed, 47)
    na, nb = 3 * shape[1] + 1, shape[2] + 3  # more than one block of 256 queries, sizes that are no multiple of anything
    return {"a": rng.integers(0, 256, (na, 2)) / 2.0, "b": rng.integers(0, 256, (nb, 2)) / 2.0}


def run_nearest_dist(ops, x):
    return {"a_to_b": ops.nearest_dist(x["a"], x["b"]), "b_to_a": ops.nearest_dist(x["b"], x["a"])}


def check_nearest_dist(x, out):
    d = np.sqrt(((x["a"][:, None, :] - x["b"][None, :, :]) ** 2).sum(axis=2))
    _bits_eq(out["a_to_b"], d.min(axis=1), "a to b")
    _bits_eq(out["b_to_a"], d.min(axis=0), "b to a")


# ------------------------------------------------------------------ what the groupings leave untouched
def run_groups_raw(ops, x):
    """the groupings of workspace_cases.run_groups with outputs that hold the state's fill (``ops.merge_groups`` and
    ``merge_groups_runs`` zero theirs: those two entries are called directly), and ``pcseg_group_reduce`` on their result"""
    torch = ops.torch  # (inside a pass of the output hooks: the padded allocations)
    cm, labels, counts = x["cm"], x["labels"], x["counts"]
    B, H, W = cm.shape
    cap = x["lists"].shape[2]
    stats, _, _, _ = ops.region_reduce(labels, counts, cls=cm, cap=cap)
    rl, n_list = x["lists"][:, 1].contiguous(), x["n_lists"][:, 1].contiguous()
    listed = _below(n_list, cap)
    out, raw = {}, {}

    def keep(tag, group_of, n_groups, group_stats=None, lengths=n_list):
        flat = lambda t, *tail: t.reshape((-1, cap) + tail)
        out["group_of_" + tag], out["n_groups_" + tag] = wc._rows_upto(flat(group_of), lengths), n_groups
        raw["group_of_" + tag] = (flat(group_of), _below(lengths, cap))
        if group_stats is not None:
            out["group_stats_" + tag] = wc._rows_upto(flat(group_stats, 8), n_groups.reshape(-1))
            raw["group_stats_" + tag] = (flat(group_stats, 8), _below(n_groups.reshape(-1), cap))

    def grouping(tag, entry, *keys):
        group_of = torch.empty((B, cap), dtype=torch.int32, device=cm.device)
        n_groups = torch.empty((B,), dtype=torch.int32, device=cm.device)
        ops._call(entry, *keys, stats, rl, n_list, group_of, n_groups, B, H, W, cap, cap, ws=(B, cap))
        keep(tag, group_of, n_groups)
        return group_of, n_groups

    labelled, _ = ops.label_bool8(ops.dilate_disk(cm, wc.GROUP_BITS, 2))
    grouping("labels", "merge_groups", labelled, 0)
    grouping("roots", "merge_groups", ops.dilated_roots(cm, wc.GROUP_BITS, 2), 1)
    bits, run_parent = ops.dilated_runs(cm, wc.GROUP_BITS, 2)
    raw["run_parent"] = (run_parent, _run_tops(bits, H))
    group_of, n_groups = grouping("runs", "merge_groups_runs", bits, run_parent)
    reduced = ops.group_reduce(stats, rl, n_list, group_of, n_groups, H, W)  # (entries beyond the list: the fill, never read)
    out["group_stats_reduce"] = wc._rows_upto(reduced, n_groups)
    reduced = torch.empty((B, cap, 8), dtype=torch.int64, device=cm.device)  # (the wrapper zeroes its table: the entry itself)
    ops._call("group_reduce", stats, rl, n_list, group_of, n_groups, reduced, B, H, W, cap, cap)
    out["group_stats_reduce_raw"] = wc._rows_upto(reduced, n_groups)
    keep("fused", *ops.merge_groups_fused(bits, run_parent, stats, x["lists"], x["n_lists"], 1))
    mbits, mpar = ops.dilated_runs_multi(cm, wc.MULTI_BITS, 2)
    raw["run_parent_multi"] = (mpar, _run_tops(mbits, H))
    lists3 = x["lists"][:, [1, 1, 1]].contiguous()  # every mask groups the same list
    keep("multi", *ops.merge_groups_fused_multi(mbits, mpar, stats, lists3, x["n_lists"][:, [1, 1, 1]].contiguous(), (0, 1, 2)),
         lengths=n_list.repeat(3))
    out["_raw"] = raw
    assert bool(listed.any()) and not bool(listed.all()), "every list is full or empty: nothing is left untouched"
    return out


def check_groups_raw(x, out):
    orc = _oracle()
    cm = x["cm"]
    B = cm.shape[0]
    for b in range(B):
        k = int(x["n_lists"][b, 1])
        entries = x["lists"][b, 1, :k]
        members = np.isin(cm[b], [v for v in range(8) if (wc.GROUP_BITS >> v) & 1])
        exp, ng = wc._expected_groups(orc, members, x["labels"][b], entries)
        for route in ("labels", "roots", "runs", "fused"):
            _eq(out["group_of_" + route][b, :k], exp, "%s, frame %d" % (route, b))
            assert int(out["n_groups_" + route][b]) == ng, (route, b)
        _eq(out["group_of_multi"][2 * B + b, :k], exp, "multi (all classes), frame %d" % b)
        assert int(out["n_groups_multi"][2, b]) == ng
        tab = orc.region_table(x["labels"][b])
        want = np.zeros((ng, 8), np.int64)
        for g in range(ng):
            rows = tab[entries[exp == g + 1]]
            want[g] = (rows[:, 0].sum(), rows[:, 1].sum(), rows[:, 2].sum(), rows[:, 3].min(), rows[:, 4].min(), rows[:, 5].max(),
                       rows[:, 6].max(), len(rows))
        for name, got in (("fused", out["group_stats_fused"][b]), ("multi", out["group_stats_multi"][2 * B + b]),
                          ("reduce", out["group_stats_reduce"][b]), ("reduce, its own table", out["group_stats_reduce_raw"][b])):
            _eq(got[:ng], want, "group rows (%s), frame %d" % (name, b))


# ------------------------------------------------------------------ outputs that a wrapper zeroes although the library writes them
def run_unzeroed(ops, x):
    """``ops.watershed`` zeroes its tie flags and ``ops.otsu_hist`` its histogram and range before the call, so the wrappers
    never show whether the library itself defines them: the two entries called directly, on outputs that hold the state's fill"""
    torch = ops.torch  # (inside a pass of the output hooks: the padded allocations)
    img, markers, mask = x["img"], x["markers"], x["mask"]
    B, H, W = img.shape
    out = {}
    for mode in (0, 1, 2):
        labels = torch.empty((B, H, W), dtype=torch.int32, device=img.device)
        flags = torch.empty((B,), dtype=torch.int32, device=img.device)
        ops._call("watershed4_f32", img, H * W, markers, mask, labels, flags, B, H, W, mode, ws=(B, H, W))
        if mode == 2:  # no exact fallback: a flagged frame's labels are no result (include/pcseg.h)
            labels = labels * (flags == 0).to(labels.dtype)[:, None, None]
        out["labels_m%d" % mode], out["flags_m%d" % mode] = labels, flags
    hist = torch.empty((B, 256), dtype=torch.int64, device=img.device)
    lohi = torch.empty((B, 2), dtype=torch.float32, device=img.device)
    ops._call("otsu_hist_f32", img, hist, lohi, B, H, W)
    out.update(hist=hist, lohi=lohi)
    return out


def check_unzeroed(x, out):
    orc = _oracle()
    wc.check_watershed(x, out)
    for b, img in enumerate(x["img"]):
        _eq(out["hist"][b], orc.threshold_otsu(img)[1], "histogram, frame %d" % b)
        _eq(out["lohi"][b], [img.min(), img.max()], "range, frame %d" % b)


# ------------------------------------------------------------------ surface points beyond points_cap
def run_surface_cap(ops, x):
    """pcseg_surface_points with a points_cap of half the surface: the first half is written, the rest is not"""
    torch = ops.torch  # (inside a pass of the output hooks: the padded allocations)
    mask = x["mask"]
    B, H, W = mask.shape
    full = ops.surface_points(mask, 2)
    n = full["points"].shape[0]
    cap = n // 2
    sf = {"bits": torch.empty_like(full["bits"]), "counts": torch.empty_like(full["counts"]),
          "offsets": torch.empty_like(full["offsets"]), "area": torch.empty_like(full["area"])}
    points = torch.empty((n, 2), dtype=torch.int32, device=mask.device)
    ops._call("surface_points", mask, 2, sf["bits"], sf["counts"], sf["offsets"], sf["area"], points, cap, B, H, W, ws=(B, H, W))
    written = torch.arange(n, device=mask.device) < cap
    out = dict(sf, points_head=points[:cap], points_all=full["points"], n_points=np.array([n, cap]))
    out["_raw"] = {"points": (points, written)}
    return out


def check_surface_cap(x, out):
    from test_gpu_surface import surface_ref
    S = surface_ref(x["mask"].astype(bool))
    pts = np.concatenate([np.argwhere(s) for s in S])
    n, cap = (int(v) for v in out["n_points"])
    assert n == len(pts) and 0 < cap < n
    _eq(out["points_all"], pts, "points")
    _eq(out["points_head"], pts[:cap], "points below the cap")
    _eq(out["counts"], S.reshape(S.shape[0], -1).sum(axis=1), "counts")
    _eq(out["offsets"], np.concatenate([[0], np.cumsum(S.reshape(S.shape[0], -1).sum(axis=1))]), "offsets")
    _eq(out["area"], x["mask"].reshape(S.shape[0], -1).sum(axis=1), "area")


# ------------------------------------------------------------------ the cases
# entries without a workspace that the workspace cases drive as they stand (test_workspace_cases_cpu.py holds their own lists to
# the entries WITH one): what FramePipeline.run / tables / agreement reach with every table switched on, and the second calls
# of two wrappers
_PIPELINE_ALSO = ("region_reduce_sel", "region_sums2", "classify_regions", "shape_properties", "hull_properties",
                  "skeleton_properties", "territory_reduce", "surface_pack_refined", "agreement_match")
ALSO_DRIVEN = {"pipeline": _PIPELINE_ALSO, "pipeline_ties": _PIPELINE_ALSO, "borders": ("relabel_map",), "contingency": ("agreement_match",)}

NEW_CASES = (
    wc._case("frontend_ops", ("argmax_planes_f32", "median5_u8", "threshold_lt_f32", "morph3x3"), build_frontend, run_frontend,
             check_frontend),
    wc._case("otsu", ("otsu_f32", "otsu_hist_f32"), build_otsu, run_otsu, check_otsu),
    wc._case("plane_sums", ("region_reduce", "region_reduce_n", "region_reduce_sel", "region_init"), build_plane_sums, run_plane_sums,
             check_plane_sums, note="W % 4 == 0 takes the fused column kernel, the ragged width the row sums kernel; a cap below the "
                                    "label count raises the overflow flag of every frame but the last"),
    wc._case("plane_sums2", ("region_sums2", "region_init", "region_reduce_sel"), build_plane_sums2, run_plane_sums2, check_plane_sums2,
             shapes=SUMS2_SHAPES),
    wc._case("roi_tables", ("region_reduce_sel", "region_shape", "shape_properties", "region_hull", "hull_properties", "thin_labels",
                            "region_skeleton", "skeleton_properties"), build_roi_tables, run_roi_tables, check_roi_tables),
    wc._case("territory", ("nearest_label_i32", "territory_labels", "territory_reduce"), build_territory, run_territory, check_territory),
    wc._case("h_extrema", ("hmax_range_i32", "hmax_range_f64", "hmax_shift_i32", "hmax_shift_f64", "hmax_shift_edt", "hmax_mark_i32",
                           "hmax_mark_f64", "reconstruct_i32", "reconstruct_f64", "ccl8_bool"), build_hmax, run_hmax, check_hmax),
    wc._case("nearest_dist", ("nearest_dist_f64",), build_nearest_dist, run_nearest_dist, check_nearest_dist),
    wc._case("groups_raw", ("merge_groups", "merge_groups_runs", "merge_groups_fused", "merge_groups_fused_multi", "group_reduce",
                            "dilate_ccl_runs_u8", "dilate_ccl_runs_multi_u8", "dilate_ccl_roots_u8"), wc.build_groups, run_groups_raw,
             check_groups_raw),
    wc._case("unzeroed", ("watershed4_f32", "otsu_hist_f32"), wc.build_watershed, run_unzeroed, check_unzeroed),
    wc._case("surface_cap", ("surface_points",), wc.build_shells, run_surface_cap, check_surface_cap),
)

CASES = tuple(c._replace(entries=c.entries + tuple("pcseg_" + e for e in ALSO_DRIVEN.get(c.name, ()))) for c in wc.CASES) + NEW_CASES

# the "not written" promises of include/pcseg.h, by the case and the ``_raw`` outputs that hold them: rows at or beyond counts[b]
# (pcseg_region_reduce_n / _sel) and min(counts[b], cap) (pcseg_region_init, also under pcseg_region_sums2), group_of beyond the
# list and group rows beyond n_groups[b] (the four groupings), run_parent off the run heads, points beyond points_cap
PROMISES = {
    "plane_sums": ("stats_sel_high", "cls_out_sel_high", "sums_sel_high", "stats_sel_low", "stats_n_high", "cls_out_n_high", "sums_n_high",
                   "stats_n_low", "stats_init_high", "sums_init_high", "stats_init_low"),
    "plane_sums2": ("stats_b", "sums_b"),
    "groups_raw": ("group_of_labels", "group_of_roots", "group_of_runs", "group_of_fused", "group_of_multi", "group_stats_fused",
                   "group_stats_multi", "run_parent", "run_parent_multi"),
    "surface_cap": ("points",),
}

# the entries of _lib.SIGNATURES that enqueue no device work, each with its reason; every other entry is declared by a case
EXEMPT = {
    "pcseg_version": "a constant", "pcseg_last_error": "the calling thread's message", "pcseg_device_count": "a query of the runtime",
    "pcseg_timing_enable": "a measurement switch", "pcseg_timing_report": "writes a host string",
    "pcseg_watershed_counters": "a measurement aid that writes host memory", "pcseg_mixing_tile": "a constant",
    "pcseg_surface_thresholds": "host only: numpy in, numpy out", "pcseg_border_block": "host only: three constants",
}


def exempt(name):
    """the reason ``name`` needs no case, or None"""
    if name.endswith("_workspace_bytes"):
        return "a size query: host arithmetic"
    return EXEMPT.get(name)
