#!/usr/bin/env python3
"""Generate tests/golden/agreement.npz: scikit-image's contingency table, adapted Rand error and variation of information
on small pairs of label images.

Run under the oracle interpreter of make_golden.py (numpy 1.26.4 / scipy 1.7.1 / scikit-image 0.18.3), from a directory
outside the repository, as the other make_golden_*.py scripts.

Only scikit-image computes anything that is stored.  ``names``: the cases.  Per case ``t_<name>`` / ``s_<name>`` the truth
and the test labels (uint8, at most 96 x 80), ``ct_<name>`` int64 (max t + 1, max s + 1) =
skimage.metrics.contingency_table(t, s, ignore_labels=[], normalize=False) as a dense array, ``are_<name>`` float64 (3) =
adapted_rand_error(t, s) (error, precision, recall) and ``vi_<name>`` float64 (2) = variation_of_information(t, s)."""
import os

import numpy as np
from skimage.metrics import adapted_rand_error, contingency_table, variation_of_information

HERE = os.path.dirname(os.path.abspath(__file__))


def discs(seed, H, W, n, rmin, rmax):
    rng = np.random.default_rng(seed)
    lab = np.zeros((H, W), np.uint8)
    rr, cc = np.mgrid[:H, :W]
    for l in range(1, n + 1):
        r, c, rad = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(rmin, rmax)
        m = (rr - r) ** 2 + (cc - c) ** 2 <= rad * rad
        lab[m & (lab == 0)] = l
    return lab


def blocks(H, W, bh, bw):
    rr, cc = np.mgrid[:H, :W]
    return (1 + (rr // bh) * ((W + bw - 1) // bw) + cc // bw).astype(np.uint8)


def main():
    rng = np.random.default_rng(2024)
    a = discs(21, 96, 80, 14, 3.0, 9.0)
    b = discs(22, 64, 64, 9, 2.0, 8.0)
    left = a.copy()
    left[a > 7] = 0
    right = a.copy()
    right[a <= 7] = 0
    over = a.copy()  # every disc cut in two along a row
    rr = np.mgrid[:96, :80][0]
    over[(a > 0) & (rr % 16 < 8)] += 14
    under = ((a + 1) // 2).astype(np.uint8)  # discs merged pairwise
    shift = np.zeros_like(a)
    shift[:, 1:] = a[:, :-1]
    dense = blocks(70, 51, 10, 7)  # no background at all
    cases = [
        ("identical", a, a.copy()),
        ("disjoint", left, right),
        ("empty_test", b, np.zeros_like(b)),
        ("empty_truth", np.zeros_like(b), b),
        ("over", a, over),
        ("under", a, under),
        ("shift", a, shift),
        ("dense_blocks", dense, blocks(70, 51, 7, 10)),
        ("random", rng.integers(0, 6, (33, 70)).astype(np.uint8), rng.integers(0, 9, (33, 70)).astype(np.uint8)),
        ("random_sparse", (rng.integers(0, 40, (83, 37)) * (rng.random((83, 37)) < 0.3)).astype(np.uint8),
         (rng.integers(0, 25, (83, 37)) * (rng.random((83, 37)) < 0.4)).astype(np.uint8)),
        ("discs_vs_discs", discs(23, 64, 64, 12, 2.0, 7.0), discs(24, 64, 64, 10, 2.0, 8.0)),
        ("one_pixel", np.array([[3]], np.uint8), np.array([[2]], np.uint8)),
    ]
    out = {"names": np.array([n for n, _, _ in cases])}
    for name, t, s in cases:
        out["t_" + name] = t
        out["s_" + name] = s
        ct = contingency_table(t, s, ignore_labels=[], normalize=False)
        out["ct_" + name] = np.asarray(ct.todense()).astype(np.int64)
        with np.errstate(all="ignore"):
            out["are_" + name] = np.array(adapted_rand_error(t, s), np.float64)
            out["vi_" + name] = np.array(variation_of_information(t, s), np.float64)
        print(name, t.shape, out["ct_" + name].shape, out["are_" + name], out["vi_" + name])
    path = os.path.join(HERE, "agreement.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
