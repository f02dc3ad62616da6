#!/opt/conda/bin/python3.9
"""Generate tests/golden/skeleton.npz: per label image, scikit-image's own thinning of every label.

Run under the oracle interpreter of make_golden.py (numpy 1.26.4 / scipy 1.7.1 / scikit-image 0.18.3), after
make_golden_shape.py:

    cd /tmp && /opt/conda/bin/python3.9 -B <repo>/tests/golden/make_golden_skeleton.py

Only scikit-image computes anything that is stored.  The inputs are every label image of shape.npz (read from it, not
stored again) and hand-made cases, which this file does store.  Per image i (``names[i]``): ``lab_%02d`` the labels
(uint16; hand-made cases only), ``skel_%02d`` the union over the labels l of ``thin(lab == l)`` (packed bits, row-major),
``full_%02d`` uint8 (H, W): the k of the first ``thin(lab == l, max_iter=k)`` that no longer holds the pixel, 0 where
nothing was deleted, and ``iters[i]``: the largest such k of the image.  Once: ``lut_first`` / ``lut_second``,
scikit-image's two look-up tables as 256 booleans each.  A label is thinned inside its bounding box with one pixel of
background around it -- what ``mode='constant'`` makes of the frame's edge.  The restatement of tests/test_skeleton_cpu.py is
imported to REPORT whether it reproduces every image; the data do not depend on it."""
import importlib.util
import os
import warnings

import numpy as np

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))

from skimage.morphology import _skeletonize, thin  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


restate = _load("skeleton_restatement", os.path.join(REPO, "tests", "test_skeleton_cpu.py"))


def hand_made():
    z = lambda h=12, w=16: np.zeros((h, w), np.int32)
    out = []
    a = z(); a[5, 2:14] = 1; a[1:4, 3] = 2
    out.append(("thin_bar_w1", a))
    a = z(); a[4:6, 2:14] = 1; a[7:11, 4:6] = 2
    out.append(("thin_bar_w2", a))
    a = z(); a[2:5, 2:14] = 1; a[6:11, 7:10] = 2
    out.append(("thin_bar_w3", a))
    a = z(); a[1:11, 2:5] = 1; a[8:11, 2:14] = 1
    out.append(("thin_L", a))
    a = z(); a[1:4, 1:15] = 1; a[1:11, 6:9] = 1
    out.append(("thin_T", a))
    a = z(14, 16); a[1:13, 2:14] = 1; a[5:9, 6:10] = 0
    out.append(("thin_ring", a))
    a = z(6, 7); a[2:4, 3:5] = 1
    out.append(("thin_block_2x2", a))
    a = z(15, 15); a[6:9, 1:14] = 1; a[1:14, 6:9] = 1
    out.append(("thin_plus", a))
    a = z(16, 20); a[2:14, 2:18] = 1  # two labels that touch along a bent line
    for r in range(2, 14):
        a[r, (10 if r < 6 else 10 + (r - 6) if r < 10 else 14):18] = 2
    out.append(("thin_touching_bent", a))
    a = z(11, 13); a[0:4, 0:5] = 1; a[0:3, 8:13] = 2; a[4:9, 10:13] = 3; a[7:11, 0:4] = 4; a[8:11, 5:9] = 5; a[5, 0] = 6
    out.append(("thin_on_edge_and_corner", a))
    out.append(("thin_full_9x13", np.ones((9, 13), np.int32)))
    a = z(48, 48); a[3:44, 4:45] = 1
    out.append(("thin_square_41_in_48", a))
    a = z(48, 48)
    rr, cc = np.mgrid[0:48, 0:48]
    a[(rr - 24) ** 2 + (cc - 23) ** 2 <= 20 * 20] = 1
    out.append(("thin_disk_20_in_48", a))
    return out


def thin_every_label(lab):
    """(skeleton bool, full-iteration image, iters) of one label image, from scikit-image's thin alone"""
    H, W = lab.shape
    skel = np.zeros((H, W), bool)
    full = np.zeros((H, W), np.int64)
    for l in np.unique(lab[lab > 0]):
        rows, cols = np.nonzero(lab == l)
        r0, r1, c0, c1 = rows.min(), rows.max() + 1, cols.min(), cols.max() + 1
        mask = np.zeros((r1 - r0 + 2, c1 - c0 + 2), bool)
        mask[1:-1, 1:-1] = lab[r0:r1, c0:c1] == l
        prev, k = mask, 0
        while True:
            k += 1
            now = thin(mask, max_iter=k)
            gone = prev & ~now
            if not gone.any():
                break
            full[r0:r1, c0:c1][gone[1:-1, 1:-1]] = k
            prev = now
        assert (prev == thin(mask)).all()
        skel[r0:r1, c0:c1] |= prev[1:-1, 1:-1]
    return skel, full, int(full.max())


def main():
    s = np.load(os.path.join(HERE, "shape.npz"), allow_pickle=False)
    images = [(str(name), s["lab_%02d" % i].astype(np.int32), False) for i, name in enumerate(s["names"])]
    images += [(name, lab, True) for name, lab in hand_made()]
    out = {"names": np.array([n for n, _, _ in images]),
           "lut_first": np.asarray(_skeletonize.G123_LUT, bool), "lut_second": np.asarray(_skeletonize.G123P_LUT, bool)}
    assert out["lut_first"].shape == out["lut_second"].shape == (256,)
    iters = []
    for i, (name, lab, store) in enumerate(images):
        assert 0 <= lab.min() and lab.max() < 65536
        skel, full, it = thin_every_label(lab)
        assert it < 256
        if lab.max() == 1:  # a 0/1 image: the union is thin(image) itself
            assert (skel == thin(lab > 0)).all(), name
        if store:
            out["lab_%02d" % i] = lab.astype(np.uint16)
        out["skel_%02d" % i], out["full_%02d" % i] = np.packbits(skel), full.astype(np.uint8)
        iters.append(it)
        peel, pit = restate.peel_image(lab)
        same = ((peel == restate.SKELETON) == skel).all() and pit == it
        gone = (lab > 0) & ~skel
        same_full = (((peel.astype(np.int64) + 1) // 2)[gone] == full[gone]).all()
        print("%-28s %4d labels  skeleton %5d px  iters %3d  restatement: skeleton %s, iterations %s" % (
            name, len(np.unique(lab[lab > 0])), skel.sum(), it, same, same_full))
    out["iters"] = np.array(iters, np.int32)
    path = os.path.join(HERE, "skeleton.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
