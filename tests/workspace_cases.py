"""What a workspace held before a call must never reach the call's result: the prior states a workspace is put into, and
the cases that drive every entry of ``_lib.WORKSPACE`` / ``_lib.WORKSPACE_HANDED_ON`` through the public ``ops`` wrappers and
``FramePipeline`` (no tests in here; ``test_workspace_cases_cpu.py`` checks this module, ``test_gpu_workspace_state.py`` runs it).

A case is a name, the entries it is expected to drive, ``build(shape, seed)`` -> a dict of numpy inputs (deterministic),
``run(ops, x)`` -> a dict of the DEFINED outputs only (``x``: the inputs as CUDA tensors) and ``check(x, out)`` that holds the
outputs (numpy) against the CPU reference the entry's own test file uses (None: no callable reference at a small shape --
``note`` says so, and the case rests on the equality across states).  ``unordered`` names the outputs that are float64 sums of
atomics in no fixed order (a finding recorded here, not a looser comparison in general): they are compared within
``sum_rtol(shape)`` instead of bit for bit."""
import collections

import numpy as np

RED_ZONE = 4096
STATES = ("zeros", "leftover-same", "leftover-other", "ones")  # in the order they are run
PRIMARY, SECOND = (2, 70, 130), (3, 96, 64)    # ragged words / tiles and W % 4 != 0; full tiles and W % 4 == 0
PIPELINE, PIPELINE_DONOR = (2, 96, 80), (2, 70, 130)


# ------------------------------------------------------------------ states of a workspace
def align256(n):
    return (int(n) + 255) & ~255


def body_bytes(nbytes):
    """Bytes in front of the red zone: the size the size query named, rounded up to the library's 256-byte carve unit (at
    least one unit, as ``ops._ws`` allocates)."""
    return max(align256(nbytes), 256)


def padded_bytes(nbytes):
    return body_bytes(nbytes) + RED_ZONE


def stretch(snapshot, n):
    """``snapshot`` (uint8) repeated or truncated to ``n`` bytes; zeros where there is nothing to repeat."""
    snapshot = np.asarray(snapshot, np.uint8).reshape(-1)
    if snapshot.size == 0:
        return np.zeros(n, np.uint8)
    return np.resize(snapshot, n)


def state_fill(state, nbytes, snapshot=None):
    """The whole buffer (body + red zone) of a workspace of ``nbytes`` in ``state``: uint8 (padded_bytes(nbytes),)."""
    n = padded_bytes(nbytes)
    if state == "zeros":
        return np.zeros(n, np.uint8)
    if state == "ones":
        return np.full(n, 0xFF, np.uint8)
    if state in ("leftover-same", "leftover-other"):
        return stretch(snapshot if snapshot is not None else np.zeros(0, np.uint8), n)
    raise ValueError(state)


def red_zone(buffer, nbytes):
    """The red-zone bytes of a whole buffer."""
    return buffer[body_bytes(nbytes):body_bytes(nbytes) + RED_ZONE]


def first_changed(got, want):
    """Offset of the first byte of ``got`` that differs from ``want``, or -1."""
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    return int(bad[0]) if bad.size else -1


def donor(snapshots, key):
    """The snapshot that fills the workspace ``key`` = (entry, ordinal): that call's, else the entry's first, else any
    (the calls of two shapes need not pair up), else None."""
    if key in snapshots:
        return snapshots[key]
    if (key[0], 0) in snapshots:
        return snapshots[(key[0], 0)]
    for k in sorted(snapshots):
        return snapshots[k]
    return None


def sum_rtol(shape):
    """Two float64 sums of the same n <= H W non-negative float32 terms, added in different orders, differ by at most
    2 (n - 1) u sum with u = 2^-53 (Higham, Accuracy and Stability, eq. 4.4 on each): relative H W 2^-52."""
    return shape[-2] * shape[-1] * 2.0 ** -52


# ------------------------------------------------------------------ inputs
def _rng(shape, seed, salt):
    return np.random.default_rng([int(seed), int(salt)] + [int(v) for v in shape])


def _blocks(rng, shape, cell, hi, zero):
    """(B, H, W) int64: a grid of ``cell`` x ``cell`` blocks of values 1 .. hi (0 with probability ``zero``), at a random offset"""
    B, H, W = shape
    out = np.zeros(shape, np.int64)
    gh, gw = -(-H // cell) + 1, -(-W // cell) + 1
    for b in range(B):
        g = rng.integers(1, hi + 1, (gh, gw))
        g[rng.random((gh, gw)) < zero] = 0
        oy, ox = rng.integers(0, cell, 2)
        out[b] = np.kron(g, np.ones((cell, cell), np.int64))[oy:oy + H, ox:ox + W]
    return out


def _class_map(shape, seed, salt=0):
    """uint8 class map: blocks of the classes 1, 2 (cells), 3 (particle), 5 (background), salted with single pixels; the
    last frame has no particle pixel and no cell: the per-frame flags of the frames differ"""
    rng = _rng(shape, seed, salt)
    cm = _blocks(rng, shape, 5, 3, 0.45)
    cm[cm == 0] = 5
    salt_px = rng.random(shape) < 0.02
    cm[salt_px] = rng.integers(1, 6, int(salt_px.sum()))
    cm[-1] = 5
    cm[-1, 0, :2] = 4
    return cm.astype(np.uint8)


def _labels(shape, seed, salt, cell, hi, zero=0.3, empty_last=True):
    lab = _blocks(_rng(shape, seed, salt), shape, cell, hi, zero).astype(np.int32)
    if empty_last:
        lab[-1] = 0
    return lab


def _points(B, seed, sizes, K, extent):
    """frame-contiguous points: xy (n, 2) float64 on a half-pixel lattice (distance ties), slot (n,) int32 with some untyped,
    ids, frame offsets; the last frame is empty"""
    rng = np.random.default_rng([int(seed), 77, B])
    sizes = list(sizes[:B - 1]) + [0]
    n = sum(sizes)
    xy = rng.integers(0, 2 * extent, (n, 2)).astype(np.float64) / 2.0
    slot = rng.integers(-1, K, n).astype(np.int32)
    ids = (np.arange(n) % 97 + 1).astype(np.int32)
    foff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return xy, slot, ids, foff


def _oracle():
    from oracle import oracle as orc
    return orc


def _eq(got, want, what):
    np.testing.assert_array_equal(np.asarray(got), np.asarray(want), err_msg=what)


# ------------------------------------------------------------------ per-op cases
def build_ccl(shape, seed):
    rng = _rng(shape, seed, 1)
    a = (rng.integers(1, 4, shape) * (rng.random(shape) < 0.55)).astype(np.uint8)
    a[-1] = 0
    return {"a": a}


def run_ccl(ops, x):
    a = x["a"]
    out = {}
    for name, fn in (("eq8", ops.label_equal8), ("bool8", ops.label_bool8), ("bool4", ops.label_bool4)):
        out[name + "_labels"], out[name + "_counts"] = fn(a)
    # the parent image of the radius-0 "dilation" of value 1, numbered: label_bool8(a == 1)
    out["compact_labels"], out["compact_counts"] = ops.compact_labels(ops.dilated_roots(a, 1 << 1, 0) + 1)
    return out


def check_ccl(x, out):
    orc = _oracle()
    a = x["a"]
    for b in range(a.shape[0]):
        for name, img, conn in (("eq8", a[b], None), ("bool8", a[b] > 0, None), ("bool4", a[b] > 0, 1), ("compact", a[b] == 1, None)):
            exp, n = orc.label(img, connectivity=conn, return_num=True) if conn else orc.label(img, return_num=True)
            _eq(out[name + "_labels"][b], exp, "%s labels, frame %d" % (name, b))
            assert int(out[name + "_counts"][b]) == n, (name, b)


def build_classmap(C):
    def build(shape, seed):
        B, H, W = shape
        rng = _rng(shape, seed, 2 + C)
        coarse = rng.random((B, C, -(-H // 4) + 1, -(-W // 4) + 1)).astype(np.float32)
        st = np.kron(coarse, np.ones((4, 4), np.float32))[:, :, 1:H + 1, 2:W + 2] + 0.6 * rng.random((B, C, H, W)).astype(np.float32)
        st[-1] = 0.25  # a constant frame: class 1 everywhere, one component
        return {"stack": np.ascontiguousarray(st, np.float32)}
    return build


def run_classmap(ops, x):
    z, labels, counts = ops.classmap_label(x["stack"])
    return {"denoised": z, "labels": labels, "counts": counts}


def check_classmap(x, out):
    orc = _oracle()
    st = x["stack"]
    for b in range(st.shape[0]):
        den = orc.median_filter((np.argmax(st[b], axis=0) + 1).astype(np.uint8))
        exp, n = orc.label(den, return_num=True)
        _eq(out["denoised"][b], den, "denoised, frame %d" % b)
        _eq(out["labels"][b], exp, "labels, frame %d" % b)
        assert int(out["counts"][b]) == n, b


EDT_CAP = 50


def build_edt(shape, seed):
    m = (_rng(shape, seed, 10).random(shape) < 0.97).astype(np.uint8)
    m[-1] = 1  # no zero pixel at all
    return {"mask": m}


def run_edt(ops, x):
    return {"d2": ops.edt_sq(x["mask"]), "d2_capped": ops.edt_sq(x["mask"], cap=EDT_CAP)}


def check_edt(x, out):
    orc = _oracle()
    for b, m in enumerate(x["mask"]):
        exp = orc.edt_sq(m.astype(bool))
        _eq(out["d2"][b], exp, "d2, frame %d" % b)
        _eq(out["d2_capped"][b], np.minimum(exp, EDT_CAP + 1), "capped d2, frame %d" % b)


def build_edt_lt(shape, seed):
    img = _rng(shape, seed, 11).random(shape).astype(np.float32) * 0.53
    img[0, 5, 5] = 0.5
    img[-1] = 0.25  # every pixel below the threshold
    return {"img": img}


def run_edt_lt(ops, x):
    d2, mask = ops.edt_sq_lt(x["img"], 0.5)
    return {"d2": d2, "mask": mask}


def check_edt_lt(x, out):
    orc = _oracle()
    for b, img in enumerate(x["img"]):
        _eq(out["mask"][b].astype(bool), img < 0.5, "mask, frame %d" % b)
        _eq(out["d2"][b], orc.edt_sq(img < 0.5), "d2, frame %d" % b)


DILATE_RADII = (2, 31, 32)  # the bit path, its last radius, the first radius of the row-block path


def build_dilate(shape, seed):
    z = (_rng(shape, seed, 12).random(shape) < 0.004).astype(np.uint8) * 3
    z[0, 0, 0] = z[0, -1, -1] = 3
    z[-1] = 1  # no pixel of the set
    return {"z": z}


def run_dilate(ops, x):
    return {"r%d" % r: ops.dilate_disk(x["z"], 1 << 3, r) for r in DILATE_RADII}


def check_dilate(x, out):
    orc = _oracle()
    for r in DILATE_RADII:
        for b, z in enumerate(x["z"]):
            _eq(out["r%d" % r][b].astype(bool), orc.binary_dilation_disk(z == 3, r), "radius %d, frame %d" % (r, b))


OVERLAP_PRESET = 1000  # overlap_area is accumulated in place (include/pcseg.h): it starts at a non-zero value


def build_fill_particle(shape, seed):
    return {"cm": _class_map(shape, seed, 13), "preset": OVERLAP_PRESET + np.arange(shape[0], dtype=np.int64)}


def run_fill_particle(ops, x):
    out, area = ops.fill_particle(x["cm"], 3, 1, 3, 20, 2, overlap_area=x["preset"].clone())
    return {"out": out, "overlap_area": area}


def check_fill_particle(x, out):
    orc = _oracle()
    for b, cm in enumerate(x["cm"]):
        exp, ov = orc.fill_particle_area(cm, 3, 1, 3)
        _eq(out["out"][b], exp, "frame %d" % b)
        assert int(out["overlap_area"][b]) == int(x["preset"][b]) + ov, b


def build_fill_holes(shape, seed):
    m = (_rng(shape, seed, 14).random(shape) < 0.58).astype(np.uint8)
    m[-1] = 0
    return {"mask": m}


def run_fill_holes(ops, x):
    return {"filled": ops.fill_holes(x["mask"])}


def check_fill_holes(x, out):
    orc = _oracle()
    for b, m in enumerate(x["mask"]):
        _eq(out["filled"][b].astype(bool), orc.binary_fill_holes(m.astype(bool)), "frame %d" % b)


def build_local_maxima(shape, seed):
    a = _rng(shape, seed, 15).integers(0, 3, shape).astype(np.int32)
    a[-1] = 7  # a constant frame has no maximum
    return {"img": a}


def run_local_maxima(ops, x):
    is_max, markers, counts = ops.local_maxima(x["img"])
    return {"is_max": is_max, "markers": markers, "counts": counts}


def check_local_maxima(x, out):
    orc = _oracle()
    for b, a in enumerate(x["img"]):
        lm = orc.local_maxima(a)
        exp, n = orc.label(lm, return_num=True)
        _eq(out["is_max"][b].astype(bool), lm, "is_max, frame %d" % b)
        _eq(out["markers"][b], exp, "markers, frame %d" % b)
        assert int(out["counts"][b]) == n, b


def build_watershed(shape, seed):
    """tie-heavy: three grey levels in frame 0 (lakes and plateaus: the second level and the exact flood), twelve smoothed
    levels in the others; the last frame has no marker"""
    B, H, W = shape
    rng = _rng(shape, seed, 16)
    img = rng.random(shape).astype(np.float32)
    img[0] = np.floor(img[0] * 3) / 3
    for b in range(1, B):
        q = np.floor(img[b] * 12) / 12
        img[b] = (q + np.roll(q, 1, 0) + np.roll(q, 1, 1)) / 3
    img = img.astype(np.float32)
    mask = (rng.random(shape) < 0.9).astype(np.uint8)
    mk = np.zeros(shape, np.int32)
    for b in range(B - 1):
        sel = rng.random((H, W)) < 0.02
        mk[b][sel] = rng.permutation(int(sel.sum())).astype(np.int32) + 1
    mk[0, 1:3, 1:4] = 500
    return {"img": img, "markers": mk, "mask": mask}


def run_watershed(ops, x):
    out = {}
    for mode in (0, 1, 2):
        labels, flags = ops.watershed(x["img"], x["markers"], x["mask"], mode=mode)
        if mode == 2:  # no exact fallback: a flagged frame's labels are no result (include/pcseg.h)
            labels = labels * (flags == 0).to(labels.dtype)[:, None, None]
        out["labels_m%d" % mode], out["flags_m%d" % mode] = labels, flags
    return out


def check_watershed(x, out):
    orc = _oracle()
    flags = out["flags_m2"]
    assert flags[:-1].any(), "no frame took the second level and the exact flood: the case has lost its ties"
    assert not flags[-1], "a frame without marker has nothing to prove"
    for b in range(x["img"].shape[0]):
        exp = orc.watershed(x["img"][b], x["markers"][b], x["mask"][b].astype(bool))
        _eq(out["labels_m0"][b], exp, "mode 0, frame %d" % b)
        _eq(out["labels_m1"][b], exp, "mode 1, frame %d" % b)
        if not flags[b]:
            _eq(out["labels_m2"][b], exp, "mode 2 (proven), frame %d" % b)
    _eq(out["flags_m0"], flags, "mode 0 reports the frames the parallel flood could not prove")


def build_reconstruct(shape, seed):
    rng = _rng(shape, seed, 17)
    mask = _blocks(rng, shape, 3, 9, 0.2).astype(np.int32)
    keep = rng.random(shape) < 0.02
    lo = np.where(keep, mask, 0).astype(np.int32)
    hi = np.where(keep, mask, 12).astype(np.int32)
    lo[-1], hi[-1] = mask[-1], mask[-1]  # seed == mask: nothing to do
    fmask = mask.astype(np.float64) / 4.0 + rng.integers(0, 2, shape) * 0.125
    flo, fhi = np.where(keep, fmask, -1.0), np.where(keep, fmask, 9.0)
    flo[-1], fhi[-1] = fmask[-1], fmask[-1]
    return {"mask": mask, "seed_lo": lo, "seed_hi": hi, "fmask": fmask, "fseed_lo": flo, "fseed_hi": fhi}


_REC = (("i32_dilation", "seed_lo", "mask", "dilation"), ("i32_erosion", "seed_hi", "mask", "erosion"),
        ("f64_dilation", "fseed_lo", "fmask", "dilation"), ("f64_erosion", "fseed_hi", "fmask", "erosion"))


def run_reconstruct(ops, x):
    out = {}
    for name, s, m, method in _REC:
        out[name], out[name + "_flags"] = ops.reconstruct(x[s], x[m], method=method, conn=8)
    return out


def check_reconstruct(x, out):
    from test_reconstruct_cpu import reconstruct_np
    for name, s, m, method in _REC:
        for b in range(x[m].shape[0]):
            _eq(out[name][b], reconstruct_np(x[s][b], x[m][b], method, 8), "%s, frame %d" % (name, b))
        assert not out[name + "_flags"].any(), name


def build_thin(shape, seed):
    return {"labels": _labels(shape, seed, 18, 9, 40, zero=0.35)}


def run_thin(ops, x):
    peel, iters = ops.thin_labels(x["labels"])
    return {"peel": peel, "iters": iters}


def check_thin(x, out):
    from test_skeleton_cpu import peel_image
    for b, lab in enumerate(x["labels"]):
        peel, iters = peel_image(lab)
        _eq(out["peel"][b], peel, "peel, frame %d" % b)
        assert int(out["iters"][b]) == int(iters), b


GROUP_BITS = (1 << 1) | (1 << 2)
MULTI_BITS = (1 << 1, 1 << 2, GROUP_BITS)


def build_groups(shape, seed):
    """a class map and one region list per frame: the regions of the classes 1 and 2, in label order (the labels are the
    oracle's: the list is an input, not a result)"""
    orc = _oracle()
    cm = _class_map(shape, seed, 19)
    labs = np.stack([orc.label(c) for c in cm]).astype(np.int32)
    counts = np.array([int(l.max()) for l in labs], np.int32)
    cap = int(max(counts.max(), 1))
    lists = np.full((shape[0], 3, cap), -7, np.int32)  # slot 1 of 3 holds the list, the others garbage
    n_lists = np.tile(np.array([5, 0, 9], np.int32), (shape[0], 1))
    for b in range(shape[0]):
        first = orc.region_table(labs[b])[:, 7]
        sel = np.nonzero(np.isin(cm[b].ravel()[first], (1, 2)))[0]
        lists[b, 1, :len(sel)] = sel
        n_lists[b, 1] = len(sel)
    return {"cm": cm, "labels": labs, "counts": counts, "lists": lists, "n_lists": n_lists}


def _rows_upto(t, n):
    """rows of every frame beyond its count set to zero: what is left is the defined part"""
    import torch
    keep = torch.arange(t.shape[1], device=t.device)[None, :] < n.to(torch.int64)[:, None]
    return torch.where(keep.reshape(keep.shape + (1,) * (t.dim() - 2)), t, torch.zeros_like(t))  # (not a product: NaN garbage)


def run_groups(ops, x):
    cm, labels, counts = x["cm"], x["labels"], x["counts"]
    stats, _, _, _ = ops.region_reduce(labels, counts, cls=cm, cap=x["lists"].shape[2])
    rl, n_list = x["lists"][:, 1].contiguous(), x["n_lists"][:, 1].contiguous()
    out = {}
    roots = ops.dilated_roots(cm, GROUP_BITS, 2)
    # a parent image is defined up to its partition (which pixel of a tree points where depends on the order of the unions):
    # its background and its numbering
    out["roots_set"] = roots >= 0
    out["roots_labels"], out["roots_counts"] = ops.compact_labels(roots + 1)
    dl, _ = ops.label_bool8(ops.dilate_disk(cm, GROUP_BITS, 2))
    out["group_of_labels"], out["n_groups_labels"] = ops.merge_groups(dl, stats, rl, n_list)
    out["group_of_roots"], out["n_groups_roots"] = ops.merge_groups(roots, stats, rl, n_list, roots=True)
    # run_parent: only the run heads are written, and they too are a parent image -- compared through the groupings
    bits, run_parent = ops.dilated_runs(cm, GROUP_BITS, 2)
    out["bits"] = bits
    out["group_of_runs"], out["n_groups_runs"] = ops.merge_groups_runs(bits, run_parent, stats, rl, n_list)
    gof, ng, gst = ops.merge_groups_fused(bits, run_parent, stats, x["lists"], x["n_lists"], 1)
    out["group_of_fused"], out["n_groups_fused"], out["group_stats_fused"] = _rows_upto(gof, n_list), ng, _rows_upto(gst, ng)
    mbits, mpar = ops.dilated_runs_multi(cm, MULTI_BITS, 2)
    out["bits_multi"] = mbits
    lists3 = x["lists"][:, [1, 1, 1]].contiguous()  # every mask groups the same list
    gof, ng, gst = ops.merge_groups_fused_multi(mbits, mpar, stats, lists3, x["n_lists"][:, [1, 1, 1]].contiguous(), (0, 1, 2))
    B, cap = rl.shape
    n3 = n_list.repeat(3)
    out["group_of_multi"] = _rows_upto(gof.reshape(3 * B, cap), n3)
    out["n_groups_multi"] = ng
    out["group_stats_multi"] = _rows_upto(gst.reshape(3 * B, cap, 8), ng.reshape(-1))
    return out


def _unpack(words, H):
    w = np.ascontiguousarray(words).view(np.uint32)
    return (((w[:, None, :] >> np.arange(32, dtype=np.uint32)[None, :, None]) & 1).reshape(-1, w.shape[1])[:H]).astype(bool)


def _expected_groups(orc, mask, label_im, entries):
    regs = {r.label - 1: r for r in orc.regionprops(label_im)}
    valid = [(k, regs[e]) for k, e in enumerate(entries) if e in regs]
    groups, _ = orc.get_merged_regions(mask, [r for _, r in valid])
    pos = {r.label: k for k, r in valid}
    exp = np.zeros(len(entries), np.int32)
    for gi, g in enumerate(groups):
        for r in g["regions"]:
            exp[pos[r.label]] = gi + 1
    return exp, len(groups)


def check_groups(x, out):
    orc = _oracle()
    cm = x["cm"]
    B, H, W = cm.shape
    for b in range(B):
        sets = [np.isin(cm[b], [v for v in range(8) if (bits >> v) & 1]) for bits in MULTI_BITS]
        dil = [orc.binary_dilation_disk(s, 2) for s in sets]
        _eq(out["roots_set"][b], dil[2], "roots, frame %d" % b)
        exp_lab, n_lab = orc.label(dil[2], return_num=True)
        _eq(out["roots_labels"][b], exp_lab, "numbered roots, frame %d" % b)
        assert int(out["roots_counts"][b]) == n_lab
        _eq(_unpack(out["bits"][b], H), dil[2], "bits, frame %d" % b)
        for m in range(3):
            _eq(_unpack(out["bits_multi"][m, b], H), dil[m], "bits of mask %d, frame %d" % (m, b))
        k = int(x["n_lists"][b, 1])
        entries = x["lists"][b, 1, :k]
        exp, ng = _expected_groups(orc, sets[2], x["labels"][b], entries)
        for route in ("labels", "roots", "runs", "fused"):
            _eq(out["group_of_" + route][b, :k], exp, "%s, frame %d" % (route, b))
            assert int(out["n_groups_" + route][b]) == ng, (route, b)
        _eq(out["group_of_multi"][2 * B + b, :k], exp, "multi (all classes), frame %d" % b)
        assert int(out["n_groups_multi"][2, b]) == ng
        tab = orc.region_table(x["labels"][b])
        for g in range(ng):
            members = entries[exp == g + 1]
            assert int(out["group_stats_fused"][b, g, 0]) == int(tab[members, 0].sum()), (b, g)
            assert int(out["group_stats_fused"][b, g, 7]) == len(members), (b, g)
        _eq(out["group_stats_multi"][2 * B + b], out["group_stats_fused"][b], "group rows, frame %d" % b)


MG_LDS = 4096                                  # csrc/reduce.hip: longer lists keep their grouping tables in the workspace
LONG_LISTS = ((2, 398, 396), (2, 394, 398))    # room for 66 x 66 and 65 x 65 single pixels at gaps of 5 or 6


def build_long_lists(shape, seed):
    """single pixels of class 1 on a grid whose gaps are 5 or 6 -- at 5 two disk(2) dilations touch, at 6 they do not --: frame
    0 lists more than MG_LDS regions (the only lists whose grouping touches its workspace), frame 1 fewer (tables in LDS)"""
    orc = _oracle()
    B, H, W = shape
    N = 66 if shape == LONG_LISTS[0] else 65
    rng = _rng(shape, seed, 31)
    rows = 2 + np.concatenate([[0], np.cumsum(rng.integers(5, 7, N - 1))])
    cols = 2 + np.concatenate([[0], np.cumsum(rng.integers(5, 7, N - 1))])
    assert rows[-1] < H and cols[-1] < W and N * N > MG_LDS > 40 * N
    cm = np.zeros(shape, np.uint8)
    cm[0][np.ix_(rows, cols)] = 1
    cm[1][np.ix_(rows[:40], cols)] = 1
    labs = np.stack([orc.label(c) for c in cm]).astype(np.int32)
    counts = np.array([int(l.max()) for l in labs], np.int32)
    lists = np.full((B, int(counts.max())), -1, np.int32)
    for b in range(B):
        lists[b, :counts[b]] = np.arange(counts[b])
    return {"cm": cm, "labels": labs, "counts": counts, "lists": lists}


def run_long_lists(ops, x):
    cm, counts, rl = x["cm"], x["counts"], x["lists"]
    cap = rl.shape[1]
    stats, _, _, _ = ops.region_reduce(x["labels"], counts, cls=cm, cap=cap)
    out = {}
    dl, _ = ops.label_bool8(ops.dilate_disk(cm, 1 << 1, 2))
    out["group_of_labels"], out["n_groups_labels"] = ops.merge_groups(dl, stats, rl, counts)
    out["group_of_roots"], out["n_groups_roots"] = ops.merge_groups(ops.dilated_roots(cm, 1 << 1, 2), stats, rl, counts, roots=True)
    bits, run_parent = ops.dilated_runs(cm, 1 << 1, 2)
    out["group_of_runs"], out["n_groups_runs"] = ops.merge_groups_runs(bits, run_parent, stats, rl, counts)
    gof, ng, gst = ops.merge_groups_fused(bits, run_parent, stats, rl[:, None, :].contiguous(), counts[:, None].contiguous(), 0)
    out["group_of_fused"], out["n_groups_fused"], out["group_stats_fused"] = _rows_upto(gof, counts), ng, _rows_upto(gst, ng)
    mbits, mpar = ops.dilated_runs_multi(cm, (1 << 1, 1 << 1), 2)
    gof, ng, gst = ops.merge_groups_fused_multi(mbits, mpar, stats, rl[:, None, :].contiguous(), counts[:, None].contiguous(), (0, 0))
    B = cm.shape[0]
    out["group_of_multi"], out["n_groups_multi"] = _rows_upto(gof.reshape(2 * B, cap), counts.repeat(2)), ng
    out["group_stats_multi"] = _rows_upto(gst.reshape(2 * B, cap, 8), ng.reshape(-1))
    return out


def check_long_lists(x, out):
    orc = _oracle()
    B = x["cm"].shape[0]
    assert x["counts"][0] > MG_LDS > x["counts"][1]
    for b in range(B):
        k = int(x["counts"][b])
        exp, ng = _expected_groups(orc, x["cm"][b] == 1, x["labels"][b], x["lists"][b, :k])
        for route in ("labels", "roots", "runs", "fused"):
            _eq(out["group_of_" + route][b, :k], exp, "%s, frame %d" % (route, b))
            assert int(out["n_groups_" + route][b]) == ng, (route, b)
        members = np.bincount(exp, minlength=ng + 1)[1:]
        _eq(out["group_stats_fused"][b, :ng, 7], members, "members, frame %d" % b)
        _eq(out["group_stats_fused"][b, :ng, 0], members, "area (single pixels), frame %d" % b)
        for m in range(2):
            _eq(out["group_of_multi"][m * B + b, :k], exp, "multi, mask %d, frame %d" % (m, b))
            _eq(out["group_stats_multi"][m * B + b], out["group_stats_fused"][b], "group rows, mask %d, frame %d" % (m, b))
            assert int(out["n_groups_multi"][m, b]) == ng


def build_overlap(shape, seed):
    rng = _rng(shape, seed, 20)
    dapi = (_blocks(rng, shape, 4, 1, 0.5) > 0).astype(np.uint8)
    other = (_blocks(rng, shape, 6, 1, 0.85) > 0).astype(np.uint8)  # some components overlap it by more than a tenth, some less
    dapi[-1] = 0
    return {"dapi": dapi, "other": other}


def run_overlap(ops, x):
    return {"out": ops.remove_overlapping(x["dapi"], x["other"], _oracle().DAPI_RFP_OVERLAP_THRESHOLD)}


def check_overlap(x, out):
    orc = _oracle()
    for b in range(x["dapi"].shape[0]):
        _eq(out["out"][b], orc.combine_cell_positions_and_clusters(x["dapi"][b], x["other"][b]), "frame %d" % b)


NEAREST_CAP = 24


def build_nearest(shape, seed):
    lab = _labels(shape, seed, 21, 11, 30, zero=0.8)  # labels above the cap are no sites; the last frame has none
    sel = (_rng(shape, seed, 22).random((shape[0], NEAREST_CAP)) < 0.8).astype(np.uint8)
    return {"labels": lab, "sel": sel}


def run_nearest(ops, x):
    d2, near, site = ops.nearest_label(x["labels"], x["sel"], NEAREST_CAP, want_site=True)
    return {"d2": d2, "near": near, "site": site}


def check_nearest(x, out):
    from test_territory_cpu import nearest_label
    for b, lab in enumerate(x["labels"]):
        d2, near, site = nearest_label(lab, x["sel"][b], NEAREST_CAP)
        _eq(out["d2"][b], d2, "d2, frame %d" % b)
        _eq(out["near"][b], near, "near, frame %d" % b)
        _eq(out["site"][b], site, "site, frame %d" % b)


PARENT_CAP = 64


def build_parent(shape, seed):
    A = _labels(shape, seed, 23, 7, PARENT_CAP, zero=0.2, empty_last=False)
    R = _labels(shape, seed, 24, 5, PARENT_CAP, zero=0.2, empty_last=False)
    R[0, :40, :40] = 3  # a ROI over more than sixteen components: the spill pass
    counts = np.array([PARENT_CAP] * (shape[0] - 1) + [0], np.int32)
    cls_a = _rng(shape, seed, 25).integers(1, 6, (shape[0], PARENT_CAP)).astype(np.uint8)
    return {"A": A, "R": R, "counts": counts, "cls_a": cls_a}


def run_parent(ops, x):
    stats, _, _, _ = ops.region_reduce(x["R"], x["counts"], cap=PARENT_CAP)
    out = ops.label_parent(x["A"], x["R"], x["counts"], cls_a=x["cls_a"], cap=PARENT_CAP, stats_r=stats, return_spilled=True)
    names = ("parent", "parent_px", "n_overlap", "cls_r")
    res = {k: _rows_upto(v, x["counts"]) for k, v in zip(names, out[:4])}  # rows r = 1 .. min(counts_r[b], cap)
    res.update(overflow=out[4], n_spilled=out[5])
    return res


def check_parent(x, out):
    from test_gpu_refined_cells import np_label_parent
    exp = np_label_parent(x["A"], x["R"], x["counts"], PARENT_CAP, x["cls_a"])
    for name, e in zip(("parent", "parent_px", "n_overlap", "cls_r", "overflow"), exp):
        _eq(out[name].astype(np.int64), e, name)
    assert int(out["n_spilled"][0]) >= 1, "no ROI took the spill pass"


CONT_CAP = 40


def build_contingency(shape, seed):
    return {"T": _labels(shape, seed, 26, 8, CONT_CAP, zero=0.3), "S": _labels(shape, seed, 27, 6, CONT_CAP + 3, zero=0.3, empty_last=False)}


def run_contingency(ops, x):
    r = ops.label_contingency(x["T"], x["S"], cap_t=CONT_CAP, cap_s=CONT_CAP)
    return {k: r[k] for k in ("frame", "t", "s", "n", "area_t", "area_s", "overflow")}


def check_contingency(x, out):
    from test_agreement_cpu import pair_rows
    rows = [pair_rows(x["T"][b], x["S"][b], CONT_CAP, CONT_CAP) for b in range(x["T"].shape[0])]
    _eq(out["frame"], np.concatenate([np.full(len(r[0]), b) for b, r in enumerate(rows)]), "frame")
    for k, name in enumerate(("t", "s", "n")):
        _eq(out[name], np.concatenate([r[k] for r in rows]), name)
    _eq(out["overflow"], [r[3] for r in rows], "overflow")
    for b, (t, s, n, _) in enumerate(rows):
        _eq(out["area_t"][b], np.bincount(t, weights=n, minlength=CONT_CAP + 1)[1:], "area_t, frame %d" % b)
        _eq(out["area_s"][b], np.bincount(s, weights=n, minlength=CONT_CAP + 1)[1:], "area_s, frame %d" % b)


BORDER_CAP, BORDER_BELOW, BORDER_PAIRS = 48, 0.45, 2048  # (blocks of random labels are no planar map: far more than 4 cap pairs)


def build_borders(shape, seed):
    L = _labels(shape, seed, 28, 6, BORDER_CAP, zero=0.1)
    V = _rng(shape, seed, 29).random(shape).astype(np.float32)
    V[0, ::7, ::5] = np.float32(0.5)
    counts = np.array([BORDER_CAP] * shape[0], np.int32)
    return {"L": L, "V": V, "counts": counts}


_BORDER_ROWS = ("frame", "a", "b", "links", "sum", "saddle", "mean", "overflow")


def run_borders(ops, x):
    r = ops.label_borders(x["L"], x["V"], conn=8, cap=BORDER_CAP, pair_cap=BORDER_PAIRS)
    out = {k: r[k] for k in _BORDER_ROWS}
    for by in ("mean", "saddle"):
        names = ("merged", "n_merged", "map", "flags")
        out.update(zip(("%s_%s" % (by, k) for k in names),
                       ops.merge_by_border(x["L"], x["V"], BORDER_BELOW, by=by, conn=8, counts=x["counts"], cap=BORDER_CAP,
                                           pair_cap=BORDER_PAIRS)))
    return out


def check_borders(x, out):
    import borders_reference as ref
    want = ref.borders(x["L"], x["V"], 8, BORDER_CAP)
    for k in _BORDER_ROWS:
        _eq(out[k].view(np.uint32) if k == "saddle" else out[k], ref.float_bits(want[k]) if k == "saddle" else want[k], k)
    for by in ("mean", "saddle"):
        for k, e in zip(("merged", "n_merged", "map", "flags"), ref.merge(x["L"], x["V"], BORDER_BELOW, by, 8, x["counts"], BORDER_CAP)):
            _eq(out["%s_%s" % (by, k)], e, "%s %s" % (by, k))


SHELL_SCALE = 2.0
SHELL_EDGES = (0.0, 0.5, 1.0, 2.0, 3.5, 6.0)


def build_shells(shape, seed):
    m = (_blocks(_rng(shape, seed, 30), shape, 12, 1, 0.6) > 0).astype(np.uint8)
    m[-1] = 0  # a frame without surface: every pixel is `over`
    return {"mask": m}


def run_shells(ops, x):
    sf = ops.surface_points(x["mask"], 2)
    out = {k: sf[k] for k in ("bits", "counts", "offsets", "area", "points")}
    out["shells"] = ops.surface_shells(sf, x["mask"], SHELL_EDGES, SHELL_SCALE)
    return out


def check_shells(x, out):
    from test_gpu_surface import shells_ref, surface_ref
    m = x["mask"].astype(bool)
    S = surface_ref(m)
    _eq(out["counts"], S.reshape(S.shape[0], -1).sum(axis=1), "counts")
    _eq(out["area"], m.reshape(m.shape[0], -1).sum(axis=1), "area")
    _eq(out["points"], np.concatenate([np.argwhere(s) for s in S]), "points")
    for b in range(m.shape[0]):
        _eq(out["shells"][b], shells_ref(m[b], SHELL_SCALE, np.asarray(SHELL_EDGES)), "shells, frame %d" % b)


MIX_K, MIX_P, MIX_SEED, MIX_SCALE = 2, 21, 7, 1.5
MIX_EDGES = (0.0, 1.0, 2.0, 4.0, 8.0, 16.0)


def build_mixing(shape, seed):
    xy, slot, _, foff = _points(shape[0], seed, (150, 90, 40), MIX_K, 40)
    return {"xy": xy, "slot": slot, "foff": foff, "keys": np.arange(shape[0], dtype=np.int64) * 3 + 11}


def run_mixing(ops, x):
    out = {}
    for tag, counts in (("", False), ("c_", True)):
        r = ops.pair_label_mixing(x["xy"], x["slot"], x["foff"], MIX_K, MIX_SCALE, MIX_EDGES, MIX_P, MIX_SEED, frame_keys=x["keys"],
                                  counts=counts)
        out.update((tag + k, v) for k, v in r.items())
    return out


def check_mixing(x, out):
    import mixing_reference as mr
    counts = mr.mixing(x["xy"], x["slot"], x["foff"], MIX_K, MIX_SCALE, np.asarray(MIX_EDGES), MIX_P, MIX_SEED, x["keys"])
    _eq(out["c_counts"], counts, "counts")
    for k, v in mr.envelope(counts).items():
        _eq(out[k], v, k)
        _eq(out["c_" + k], v, k + " (with counts)")


# ------------------------------------------------------------------ the pipeline case
PAIR_EDGES = (0.0, 0.25, 0.5, 1.0, 2.0, 4.0)      # um, at 512 / 19 pixels per um
SURFACE_EDGES = (0.0, 0.1, 0.25, 0.5, 1.0, 2.0)
TABLE_SWITCHES = dict(neighbours=True, pair_edges=PAIR_EDGES, mixing=19, mixing_seed=5, refined=True, surface=True,
                      surface_edges=SURFACE_EDGES, territory=True, territory_reach=0.6, skeleton=True, convex=True, shape=True)
# float64 sums whose terms are added by atomics in no fixed order (csrc/reduce.hip: region_sums2_col_kernel and the row
# sums kernel; DESIGN.md, "plane sums to the float64 atomics' reordering"): the two sums tables and the columns made of them.
# (Measured on the MI355X at these shapes: 57 runs, no bit ever differed -- but nothing fixes the order, so the unquantised
# case states the bound.  The quantised case needs none: its planes are float32(k / 100), multiples of 2^-30 below 1, and a
# sum of fewer than 2^13 of them is exact in float64 whatever the order -- there every sum is compared bit for bit.)
PIPELINE_UNORDERED = {"cc_sums": 0, "ws_sums": 0, "table_cells": 14, "table_rois": 5}  # name -> first unordered column


def _cell_types():
    from particle_col_image_segmentation_amd import synth
    return dict(synth.CELL_TYPES_5)


def build_pipeline(ties):
    def build(shape, seed):
        """``shape[0]`` frames the reference segments without raising (tiff_analysis.py:776-781 does on some), from ``seed`` on"""
        from particle_col_image_segmentation_amd import synth
        orc = _oracle()
        B, H, W = shape
        ct = _cell_types()
        seeds, s = [], 300 + 1000 * int(seed)
        while len(seeds) < B:
            try:
                orc.segment_frame(synth.gen_frame(s, H, W, ties=ties), ct, merged=False)
                seeds.append(s)
            except ValueError:
                pass
            s += 1
        stack = np.stack([synth.gen_frame(s, H, W, ties=ties) for s in seeds])
        # a truth image for agreement(): the reference's refined labels, shifted by a row
        truth = np.stack([np.roll(orc.refine_boundaries(st[synth.BOUNDARY_PLANE])["labels"], 1, 0) for st in stack]).astype(np.int32)
        return {"stack": stack, "truth": truth, "frame_ids": np.array(seeds, np.int64)}
    return build


_RES_WHOLE = ("denoised", "labels", "counts", "recreated", "overlap_area", "particle_area", "mask", "markers", "n_markers", "ws_labels",
              "tie_flags", "nan_flag", "overflow", "ws_overflow", "n_list", "type_stats")
_RES_ROWS = (("stats", "counts"), ("cls_out", "counts"), ("kind", "counts"), ("slot_of", "counts"), ("cells", "counts"),
             ("cc_sums", "counts"), ("ws_stats", "n_markers"), ("ws_sums", "n_markers"))


def run_pipeline(ops, x):
    from particle_col_image_segmentation_amd.pipeline import FramePipeline
    pipe = FramePipeline(_cell_types(), graph=False)
    res = pipe.run(x["stack"])
    res.check()
    ids = [int(v) for v in x["frame_ids"].cpu()]
    out = {k: res[k] for k in _RES_WHOLE}
    out.update((k, _rows_upto(res[k], res[n])) for k, n in _RES_ROWS)  # rows at or beyond a frame's count are not written
    for s, g in res["groups"].items():
        k = res["n_list"][:, s]
        out["group_of_%d" % s], out["n_groups_%d" % s] = _rows_upto(g["group_of"], k), g["n_groups"]
        out["group_stats_%d" % s] = _rows_upto(g["group_stats"], g["n_groups"])
    tabs = pipe.tables(res, frame_ids=ids, distances=True, **FramePipeline.table_kwargs("tables_device", TABLE_SWITCHES))
    out.update(("table_" + k, v) for k, v in tabs.items() if isinstance(v, np.ndarray))
    for part in (pipe.agreement(res, x["truth"], frame_ids=ids), pipe.borders(res, frame_ids=ids)):
        out.update(("table_" + k, v) for k, v in part.items() if isinstance(v, np.ndarray))
    pipe.synchronize()
    out["_reference"] = (res, tabs)  # for check(): what oracle.parity compares
    return out


def check_pipeline(x, out):
    from oracle import parity
    orc = _oracle()
    ct = _cell_types()
    res, tabs = out["_reference"]
    refs = [parity.describe(orc.segment_frame(st, ct), ct) for st in x["stack"]]
    n = len(refs)
    assert parity.compare(res, range(n), refs, sums_rtol=1e-9) == n
    assert parity.compare_tables(tabs, [int(v) for v in x["frame_ids"]], refs) == n
    for name in ("neighbours", "mixing", "refined", "surface", "surface_shells", "territories", "adjacency", "skeletons", "convexity",
                 "shapes", "refined_shapes", "distances", "agreement_pairs", "borders"):
        assert out["table_" + name].shape[0] > 0, "the %s table is empty: the case does not exercise its entry" % name


_PIPELINE_ENTRIES = (
    "classmap_label_f32", "edt_sq_lt_f32", "local_maxima_i32", "watershed4_f32", "fill_particle", "dilate_ccl_runs_multi_u8",
    "merge_groups_fused_multi", "table_layout", "table_write", "cell_distances", "neighbours_pack_cells", "surface_pack_cells",
    "point_neighbours", "pair_label_mixing", "label_parent", "refined_layout", "refined_table_write", "fill_holes", "surface_points",
    "surface_distances", "surface_shells", "nearest_label_i32", "territory_pairs", "territory_pairs_write", "thin_labels",
    "region_skeleton", "region_hull", "region_shape", "label_contingency", "contingency_write", "label_borders", "label_borders_write")
_PIPELINE_NOTE = ("images, region tables, classification, groups and the dense tables are held against oracle.segment_frame through "
                  "oracle.parity; the optional tables (neighbours, mixing, refined, surface, territory, skeleton, convexity, shape), "
                  "agreement and borders have no single callable reference for a whole pipeline batch -- their entries' own test "
                  "files restate them table by table -- and rest on the equality across states here.  Both frames are regular ones: "
                  "the reference raises on a frame without cells, so the degenerate frame is left to the per-op cases")

Case = collections.namedtuple("Case", "name entries shapes donor_shape build run check unordered note")


def _case(name, entries, build, run, check, shapes=(PRIMARY, SECOND), donor_shape=None, unordered=None, note=""):
    return Case(name, tuple("pcseg_" + e for e in entries), tuple(shapes), donor_shape, build, run, check, dict(unordered or {}), note)


CASES = (
    _case("pipeline", _PIPELINE_ENTRIES, build_pipeline(False), run_pipeline, check_pipeline, shapes=(PIPELINE,),
          donor_shape=PIPELINE_DONOR, unordered=PIPELINE_UNORDERED, note=_PIPELINE_NOTE),
    _case("pipeline_ties", _PIPELINE_ENTRIES, build_pipeline(True), run_pipeline, check_pipeline, shapes=(PIPELINE,),
          donor_shape=PIPELINE_DONOR, note=_PIPELINE_NOTE),
    _case("ccl", ("ccl8_equal_u8", "ccl8_bool", "ccl4_bool", "compact_labels", "dilate_ccl_roots_u8"), build_ccl, run_ccl, check_ccl),
    _case("classmap_c5", ("classmap_label_f32",), build_classmap(5), run_classmap, check_classmap),
    _case("classmap_c7", ("classmap_label_f32",), build_classmap(7), run_classmap, check_classmap,
          note="seven planes: the unfused route, which hands the head of its workspace to pcseg_ccl8_equal_u8 inside the library"),
    _case("edt", ("edt_sq_u8",), build_edt, run_edt, check_edt),
    _case("edt_lt", ("edt_sq_lt_f32",), build_edt_lt, run_edt_lt, check_edt_lt),
    _case("dilate_disk", ("dilate_disk_u8",), build_dilate, run_dilate, check_dilate),
    _case("fill_particle", ("fill_particle",), build_fill_particle, run_fill_particle, check_fill_particle),
    _case("fill_holes", ("fill_holes",), build_fill_holes, run_fill_holes, check_fill_holes),
    _case("local_maxima", ("local_maxima_i32",), build_local_maxima, run_local_maxima, check_local_maxima),
    _case("watershed", ("watershed4_f32",), build_watershed, run_watershed, check_watershed,
          note="mode 2 has no exact fallback: the labels of a frame it flags are no result and are left out"),
    _case("reconstruct", ("reconstruct_i32", "reconstruct_f64"), build_reconstruct, run_reconstruct, check_reconstruct),
    _case("thin_labels", ("thin_labels",), build_thin, run_thin, check_thin),
    _case("groups", ("dilate_ccl_roots_u8", "dilate_ccl_runs_u8", "dilate_ccl_runs_multi_u8", "merge_groups", "merge_groups_runs",
                     "merge_groups_fused", "merge_groups_fused_multi", "compact_labels", "dilate_disk_u8", "ccl8_bool"),
          build_groups, run_groups, check_groups,
          note="the parent images (roots, run_parent) are defined up to their partition: compared as numbered labels and through "
               "the groupings that read them; entries of group_of beyond a list and group rows beyond the group count are not "
               "written.  Lists here are shorter than 4096 regions: the groupings keep their tables in LDS and never touch the "
               "workspace they are handed (the case long_lists does)"),
    _case("long_lists", ("merge_groups", "merge_groups_runs", "merge_groups_fused", "merge_groups_fused_multi", "dilate_ccl_roots_u8",
                         "dilate_ccl_runs_u8", "dilate_ccl_runs_multi_u8", "dilate_disk_u8", "ccl8_bool"),
          build_long_lists, run_long_lists, check_long_lists, shapes=LONG_LISTS,
          note="the one case above the small shapes: only a list of more than 4096 regions makes a grouping use its workspace"),
    _case("remove_overlapping", ("remove_overlapping",), build_overlap, run_overlap, check_overlap),
    _case("nearest_label", ("nearest_label_i32",), build_nearest, run_nearest, check_nearest),
    _case("label_parent", ("label_parent",), build_parent, run_parent, check_parent),
    _case("contingency", ("label_contingency", "contingency_write"), build_contingency, run_contingency, check_contingency),
    _case("borders", ("label_borders", "label_borders_write", "border_merge"), build_borders, run_borders, check_borders),
    _case("surface_shells", ("surface_points", "surface_shells"), build_shells, run_shells, check_shells),
    _case("mixing", ("pair_label_mixing",), build_mixing, run_mixing, check_mixing),
)


def other_shape(case, shape):
    """The shape whose leftovers fill the workspaces of ``case`` at ``shape`` in the state leftover-other."""
    if case.donor_shape is not None:
        return case.donor_shape
    return [s for s in case.shapes if s != shape][0]
