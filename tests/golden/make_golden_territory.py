#!/opt/conda/bin/python3.9
"""Generate tests/golden/territory.npz: scipy's distance transform and scikit-image's expand_labels on small label images.

Run under the oracle interpreter of make_golden.py (numpy 1.26.4 / scipy 1.7.1 / scikit-image 0.18.3):

    cd /tmp && /opt/conda/bin/python3.9 -B <repo>/tests/golden/make_golden_territory.py

Only scipy / scikit-image compute anything that is stored.  ``names``: the cases; seeded disc layouts ``discs_*`` from 64 x 64
to 256 x 256 and two hand-made tie-heavy images ``ties_*``.  Per case: ``lab_<name>`` the labels (uint8); for the seeded
layouts also ``d2_<name>`` int32 = round(distance_transform_edt(lab == 0) ** 2), ``exp_<name>_<k>`` uint8 =
expand_labels(lab, distances[k]) and ``tie_<name>`` bool: the pixels whose two nearest DISTINCT labels are equally far
(per-label distance transforms, squared and rounded) -- where scikit-image calls the result undefined and the project takes
the smallest label.  The tie share of every seeded layout is printed; tests/test_territory_cpu.py holds it to 1 %."""
import os

import numpy as np
from scipy import ndimage as ndi
from skimage.segmentation import expand_labels

HERE = os.path.dirname(os.path.abspath(__file__))
DISTANCES = np.array([1.0, 2.5, 7.0, 1000.0])


def discs(seed, H, W, n, rmin, rmax):
    rng = np.random.default_rng(seed)
    lab = np.zeros((H, W), np.uint8)
    rr, cc = np.mgrid[:H, :W]
    for l in range(1, n + 1):
        r, c, rad = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(rmin, rmax)
        m = (rr - r) ** 2 + (cc - c) ** 2 <= rad * rad
        lab[m & (lab == 0)] = l
    return lab


def ties(lab):
    d = np.stack([np.rint(ndi.distance_transform_edt(lab != l) ** 2).astype(np.int64) for l in np.unique(lab[lab > 0])])
    return (d == d.min(axis=0)).sum(axis=0) >= 2


def main():
    cases = [("discs_64", discs(11, 64, 64, 5, 1.5, 5.0)), ("discs_96x80", discs(12, 96, 80, 14, 1.0, 6.0)),
             ("discs_70x131", discs(13, 70, 131, 12, 1.0, 4.0)), ("discs_128", discs(14, 128, 128, 20, 1.0, 6.0)),
             ("discs_256", discs(15, 256, 256, 24, 1.0, 5.0))]
    a = np.zeros((33, 35), np.uint8)  # single-pixel labels on a lattice of spacing 2: nearly every other pixel is tied
    k = 0
    for r in range(0, 33, 2):
        for c in range(0, 35, 2):
            k += 1
            a[r, c] = 1 + (k * 7) % 200
    b = np.zeros((40, 40), np.uint8)  # bars across the frame, the larger label above: whole rows midway between two of them
    for k, r in enumerate(range(4, 40, 8)):
        b[r, 3:38] = 5 - k
    b[20, 20] = 0  # (a gap: its pixel has the bar's two ends beside it and a bar above and below equally far)
    cases += [("ties_lattice", a), ("ties_mirror", b)]
    out = {"names": np.array([n for n, _ in cases]), "distances": DISTANCES}
    for name, lab in cases:
        out["lab_" + name] = lab
        if name.startswith("ties_"):
            continue
        out["d2_" + name] = np.rint(ndi.distance_transform_edt(lab == 0) ** 2).astype(np.int32)
        out["tie_" + name] = ties(lab)
        print(name, lab.shape, "labels", int(lab.max()), "tie share %.4f" % out["tie_" + name].mean())
        for k, dist in enumerate(DISTANCES):
            out["exp_%s_%d" % (name, k)] = expand_labels(lab, dist).astype(np.uint8)
    path = os.path.join(HERE, "territory.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
