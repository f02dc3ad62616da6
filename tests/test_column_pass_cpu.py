"""Frames for the column pass that the distance transform and the nearest-label transform share (csrc/column_pass.h), and
their expectations, without a device.

The two transforms measure to the same targets when the distance transform's mask is "1 except on a site": the frames below
are label images, built where the shared pass can go wrong -- the carry kernel takes a column's words eight at a time, the
staging of a row block takes 1024 columns at a time, the last word of a column may hold a single row.  The expectations are
checked against each other here, before tests/test_gpu_column_pass.py compares the device with them by equality."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from test_territory_cpu import nearest_label

# (257, 5): nine words, the ninth holds one row -- the carry's second batch holds one word.  (549, 3): eighteen words, the
# last holds five rows, three carry batches.  (290, 70): ten words, more than a wave of columns.  (33, 1030): the staging's
# second batch holds six columns.  (65, 8): not a case of the shared pass itself -- a width that is a multiple of four, so
# that the distance transform's four-column bit kernel writes the words, the last of which holds one row
SHAPES = [(257, 5), (549, 3), (290, 70), (33, 1030), (65, 8)]
CAP = 7     # labels of the sites: 1 .. 7
EDT_CAP = 50
RADII = (31, 32)  # the largest reach of the bit-word dilation, the smallest of the row-block pass


def frames(H, W):
    """[(name, (H, W) int32 label image)]: seven frames with sites, then one without"""
    rng = np.random.default_rng(1000 * H + W)
    lab = (1 + (np.arange(H)[:, None] * 3 + np.arange(W)[None] * 5) % CAP).astype(np.int32)  # the label a site would have
    last = 32 * ((H - 1) // 32)  # first row of the last word
    out = []

    def add(name, sites):
        out.append((name, np.where(sites, lab, 0).astype(np.int32)))

    s = np.zeros((H, W), bool); s[0, 0] = True
    add("site at (0, 0)", s)
    s = np.zeros((H, W), bool); s[H - 1, W - 1] = True
    add("site at (H-1, W-1)", s)
    s = rng.random((H, W)) < 0.02  # sites only in the first and in the last word
    s[32:last] = False
    s[5, 0] = s[H - 1, W - 1] = True
    add("first and last word", s)
    s = np.zeros((H, W), bool)  # the first and last row of every word, every third column
    rows = np.arange(H)
    s[(rows % 32 == 0) | (rows % 32 == 31) | (rows == H - 1), ::3] = True
    add("word ends", s)
    s = np.zeros((H, W), bool); s[:, W // 2] = True
    add("one full column", s)
    s = np.zeros((H, W), bool); s[0, :] = True; s[0, W // 2] = False
    add("one empty column", s)
    add("sparse", rng.random((H, W)) < 0.02)
    add("empty", np.zeros((H, W), bool))
    return out


def capped(d2, cap):
    """include/pcseg.h: a squared distance above cap is reported as cap + 1"""
    return np.where(d2 > cap, cap + 1, d2)


@functools.lru_cache(maxsize=None)
def reference(shape):
    """the frames of a shape and what both transforms must give, computed once: labels (8, H, W) int32, mask (1 except on a
    site) uint8, the brute-force (d2, near, site) of the nearest-label transform, the oracle's squared distances, and the
    oracle's disk dilations of the sites at RADII"""
    H, W = shape
    labs = np.stack([f for _, f in frames(H, W)])
    mask = (labs == 0).astype(np.uint8)
    vor = [np.stack(x) for x in zip(*(nearest_label(l, None, CAP) for l in labs))]
    ref = {"names": [n for n, _ in frames(H, W)], "labels": labs, "mask": mask, "d2": vor[0], "near": vor[1], "site": vor[2],
           "edt": np.stack([orc.edt_sq(m) for m in mask]),
           "dilate": {r: np.stack([orc.binary_dilation_disk(m == 0, r) for m in mask]) for r in RADII}}
    for v in (labs, mask, *vor, ref["edt"], *ref["dilate"].values()):
        v.setflags(write=False)
    return ref


@pytest.mark.parametrize("shape", SHAPES)
def test_frames_are_what_they_claim(shape):
    H, W = shape
    ref = reference(shape)
    sites = ref["labels"] > 0
    assert ref["names"][-1] == "empty" and len(ref["names"]) == 8
    assert sites[:7].any(axis=(1, 2)).all() and not sites[7].any()
    assert sites[0].sum() == 1 and sites[0, 0, 0] and sites[1].sum() == 1 and sites[1, H - 1, W - 1]
    last = 32 * ((H - 1) // 32)
    assert sites[2, :32].any() and sites[2, last:].any() and not sites[2, 32:last].any()
    assert sites[3, 0, 0] and sites[3, 31, 0] and sites[3, H - 1, 0] and sites[3, last, 0]
    assert sites[4].all(axis=0).sum() == 1 and sites[4].sum() == H
    assert (~sites[5].any(axis=0)).sum() == 1 and sites[5].sum() == W - 1
    assert 0.01 < sites[6].mean() < 0.03
    assert ref["labels"].max() == CAP


@pytest.mark.parametrize("shape", SHAPES)
def test_references_agree(shape):
    H, W = shape
    ref = reference(shape)
    d2, edt = ref["d2"], ref["edt"]
    # the nearest-label transform's D2 is the squared distance transform of "1 except on a site"
    np.testing.assert_array_equal(d2[:7], edt[:7])
    # the disk dilation of the sites is a threshold of it
    for r in RADII:
        np.testing.assert_array_equal(ref["dilate"][r][:7], d2[:7] <= r * r)
        assert not ref["dilate"][r][7].any()  # the empty set dilates to the empty set
    # cap = 50: min(D2, 51), and the frames hold distances on both sides of it
    np.testing.assert_array_equal(capped(edt, EDT_CAP), np.minimum(edt, EDT_CAP + 1))
    assert (edt[:7] <= EDT_CAP).any() and (edt[:7] > EDT_CAP).any()
    # the two empty-frame rules: -1, 0, -1 for the nearest-label transform, scipy's virtual pixel at (-1, 0) for the other
    assert (d2[7] == -1).all() and (ref["near"][7] == 0).all() and (ref["site"][7] == -1).all()
    r, c = np.mgrid[:H, :W]
    np.testing.assert_array_equal(edt[7], (r + 1) ** 2 + c ** 2)
