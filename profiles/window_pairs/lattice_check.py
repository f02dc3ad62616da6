"""CPU Monte Carlo behind the lattice caveat of DESIGN.md section 22: continuous uniform points in a window against the exact
lattice expectation npairs * G / A^2.  numpy only; no GPU, no part of the tests.

    python profiles/window_pairs/lattice_check.py [--trials 400] [--points 300]
"""
import argparse

import numpy as np


def window(n=256):
    yy, xx = np.mgrid[:n, :n].astype(np.float64)
    c = (n - 1) / 2.0
    return ((((yy - c) / (0.42 * n)) ** 2 + ((xx - c) / (0.35 * n)) ** 2) <= 1.0) & (((yy - 0.8 * c) ** 2 + (xx - 1.1 * c) ** 2) > (0.09 * n) ** 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=400)
    ap.add_argument("--points", type=int, default=300)
    a = ap.parse_args()
    scale, m = 9.95, 10
    M = window()
    H, W = M.shape
    A = int(M.sum())
    f = np.fft.rfft2(M.astype(np.float64), s=(2 * H, 2 * W))
    ac = np.rint(np.fft.irfft2(f * np.conj(f), s=(2 * H, 2 * W)))
    d = np.fft.fftfreq(2 * H, 1.0 / (2 * H))
    dist = np.sqrt(d[:, None] ** 2 + d[None, :] ** 2) / scale
    G = np.histogram(dist, bins=np.arange(m + 1.0), weights=ac)[0]
    n = a.points
    expected = n * (n - 1) / 2.0 * G / (float(A) * A)
    rng = np.random.default_rng(1)
    ys, xs = np.nonzero(M)
    total = np.zeros(m)
    for _ in range(a.trials):
        pick = rng.integers(0, A, n)
        p = np.stack([ys[pick] + rng.uniform(-0.5, 0.5, n), xs[pick] + rng.uniform(-0.5, 0.5, n)], axis=1)
        dd = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2))[np.triu_indices(n, 1)] / scale
        total += np.histogram(dd, bins=np.arange(m + 1.0))[0]
    print("window px", A)
    for k in range(m):
        print("bin %d: mean observed / lattice expectation = %.4f" % (k, total[k] / a.trials / expected[k]))


if __name__ == "__main__":
    main()
