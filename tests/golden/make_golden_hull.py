#!/opt/conda/bin/python3.9
"""Generate tests/golden/hull.npz: per region, scikit-image's own convex_area, solidity, feret_diameter_max, euler_number.

Run under the oracle interpreter of make_golden.py (numpy 1.26.4 / scipy 1.7.1 / scikit-image 0.18.3), after
make_golden_shape.py:

    cd /tmp && /opt/conda/bin/python3.9 -B <repo>/tests/golden/make_golden_hull.py

Only scikit-image computes anything that is stored.  The inputs are every label image of shape.npz (read from it, not
stored again) and hand-made cases, which this file does store.  Per image i (``names[i]``): ``lab_%02d`` the labels
(uint16; hand-made cases only), ``lbl_%02d`` int32 (n,) the labels of the recorded regions in label order, ``val_%02d``
float64 (n, 4) = convex_area, solidity, feret_diameter_max, euler_number.  A region on which scikit-image raises is left
out and printed.  The restatement of tests/test_hull_cpu.py is imported to REPORT how many regions it reproduces exactly;
the data do not depend on it."""
import importlib.util
import os
import warnings

import numpy as np

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))

from skimage import measure  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


restate = _load("hull_restatement", os.path.join(REPO, "tests", "test_hull_cpu.py"))


def hand_made():
    z = lambda h=12, w=14: np.zeros((h, w), np.int32)
    out = []
    a = z(); a[2:10, 3:5] = 1; a[8:10, 3:11] = 1
    out.append(("hull_L", a))
    a = z(); a[2:10, 2:4] = 1; a[2:10, 9:11] = 1; a[8:10, 2:11] = 1
    out.append(("hull_U", a))
    a = z(21, 23)  # a thin spiral: the hull is much larger than the area
    r, c, dr, dc, run = 10, 11, 0, 1, 2
    while 0 < r < 20 and 0 < c < 22:
        for _ in range(run):
            if not (0 < r < 20 and 0 < c < 22):
                break
            a[r, c] = 1
            r, c = r + dr, c + dc
        dr, dc = dc, -dr
        run += 2
    out.append(("hull_spiral", a))
    a = z(12, 16); a[2:10, 2:14] = 1; a[4:8, 4:7] = 0; a[4:8, 9:12] = 0
    out.append(("hull_ring_two_holes", a))
    a = z(); a[2:5, 2:5] = 1; a[5:8, 5:8] = 1; a[3, 3] = 0; a[6, 6] = 0  # two rings that touch only diagonally
    out.append(("hull_eight_diagonal", a))
    a = z(9, 11); a[3, 3] = 1; a[4, 4] = 1; a[5, 3] = 1; a[2, 7] = 2; a[3, 8] = 2
    out.append(("hull_diagonal_pixels", a))
    a = z(12, 15)  # two combs pushed into each other: each hull covers the other's teeth
    a[1, 1:14] = 1; a[10, 1:14] = 2
    for c in range(1, 14, 4):
        a[1:9, c] = 1
    for c in range(3, 14, 4):
        a[3:11, c] = 2
    out.append(("hull_interleaved", a))
    a = z(9, 11); a[0:3, 3:9] = 1; a[1, 4:8] = 0; a[5:9, 10] = 2; a[8, 2:6] = 3; a[3:7, 0] = 4; a[4, 0] = 0
    out.append(("hull_on_edges", a))
    a = z(9, 11); a[0:2, 0:3] = 1; a[1, 1] = 0; a[7:9, 9:11] = 2; a[0, 10] = 3; a[6:9, 0] = 4; a[8, 0:3] = 4
    out.append(("hull_in_corners", a))
    a = z(5, 7); a[2, 3] = 1
    out.append(("hull_single_pixel", a))
    a = z(6, 7); a[2:4, 3:5] = 1
    out.append(("hull_block_2x2", a))
    a = z(12, 13); a[2:10, 2:11] = 1; a[4:8, 5:8] = 0; a[5, 6] = 2
    out.append(("hull_ring", a))
    out.append(("hull_full_frame", np.ones((7, 10), np.int32)))
    a = np.zeros((300, 5), np.int32)  # one ROI over all 300 rows, wandering between the columns
    a[np.arange(300), (np.arange(300) // 37) % 5] = 1; a[np.arange(300), 2] = 1
    out.append(("hull_tall_300x5", a))
    a = np.zeros((67, 130), np.int32)  # a concave ROI across row 64 and column 64
    a[2:66, 60:70] = 1; a[60:66, 3:128] = 1; a[20:60, 66:70] = 0; a[63:66, 40:50] = 0; a[0:3, 120:130] = 2
    out.append(("hull_cross_67x130", a))
    rng = np.random.default_rng(20)
    a = (rng.random((40, 45)) < 0.55).astype(np.int32)
    out.append(("hull_noise_labels", measure.label(a, connectivity=2).astype(np.int32)))
    return out


def properties(name, lab):
    lbl, val = [], []
    for r in measure.regionprops(lab):
        try:
            row = [float(r.convex_area), float(r.solidity), float(r.feret_diameter_max), float(r.euler_number)]
        except Exception as e:  # noqa: BLE001
            print("   EXCLUDED %s label %d: %s" % (name, r.label, type(e).__name__))
            continue
        lbl.append(r.label)
        val.append(row)
    return np.array(lbl, np.int32), np.array(val, np.float64).reshape(-1, 4)


def main():
    s = np.load(os.path.join(HERE, "shape.npz"), allow_pickle=False)
    images = [(str(name), s["lab_%02d" % i].astype(np.int32), False) for i, name in enumerate(s["names"])]
    images += [(name, lab, True) for name, lab in hand_made()]
    out = {"names": np.array([n for n, _, _ in images])}
    for i, (name, lab, store) in enumerate(images):
        assert 0 <= lab.min() and lab.max() < 65536
        lbl, val = properties(name, lab)
        n_regions = int(len(np.unique(lab[lab > 0])))
        assert store or len(lbl) == n_regions, name  # nothing excluded on the shape.npz images
        if store:
            out["lab_%02d" % i] = lab.astype(np.uint16)
        out["lbl_%02d" % i], out["val_%02d" % i] = lbl, val
        table = restate.hull_table(lab)
        props = restate.hull_properties(restate.areas(lab), table)[lbl - 1]
        same = [(props[:, k] == val[:, k]).sum() for k in range(4)]
        print("%-28s %5d regions (%d excluded)  equal: convex_area %d solidity %d feret %d euler %d" % (
            name, len(lbl), n_regions - len(lbl), *same))
    path = os.path.join(HERE, "hull.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
