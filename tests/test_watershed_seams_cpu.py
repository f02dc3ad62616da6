"""What tests/test_gpu_watershed_seams.py takes for granted about its inputs (tests/watershed_windows.py), on the CPU
oracle: the families are what they say, a frame with ONE window is labelled like the window alone, a frame with nine is
not, and the float-special frames are sensitive to the mistakes they are there for."""
import itertools

import numpy as np
import pytest

import watershed_windows as ww
from oracle import oracle as orc


def test_family_sizes_and_seeds():
    assert [ww.FAMILY_SIZES[n] for n in ww.FAMILIES] == [19683, 18432, 4096, 19683, 19683]
    for name in ww.FAMILIES:
        fam = ww.family(name)
        n = ww.FAMILY_SIZES[name]
        hw = {"Dh": (1, 9), "Dv": (9, 1)}.get(name, (3, 3))
        assert fam.values.shape == (n,) + hw and fam.values.dtype == np.float32
        assert fam.markers.shape == (n,) + hw and fam.markers.dtype == np.int32
        flat = fam.markers.reshape(n, 9)
        assert ((flat == 1).sum(1) == 1).all() and ((flat == 2).sum(1) == 1).all() and ((flat > 0).sum(1) == 2).all()
        assert (flat.argmax(1) == np.argmax(flat == 2, 1)).all() and (np.argmax(flat == 1, 1) < np.argmax(flat == 2, 1)).all()
    a, b, c = ww.family("A"), ww.family("B"), ww.family("C")
    assert len({v.tobytes() for v in a.values}) == 3 ** 9 and set(np.unique(a.values)) == {0.25, 0.5, 0.75}
    assert (a.markers[:, 0, 0] == 1).all() and (a.markers[:, 2, 2] == 2).all()
    assert set(np.unique(b.values)) == {0.25, 0.75}
    assert len({v.tobytes() + m.tobytes() for v, m in zip(b.values, b.markers)}) == 2 ** 9 * 36
    pairs = {(int(np.argmax(m.ravel() == 1)), int(np.argmax(m.ravel() == 2))) for m in b.markers[:36]}
    assert pairs == set(itertools.combinations(range(9), 2))
    for name in ("Dh", "Dv"):
        d = ww.family(name)
        assert len({v.tobytes() for v in d.values}) == 3 ** 9
        assert (d.markers.reshape(-1, 9)[:, 0] == 1).all() and (d.markers.reshape(-1, 9)[:, 8] == 2).all()
    assert np.array_equal(ww.family("Dh").values.reshape(-1, 9), ww.family("Dv").values.reshape(-1, 9))
    assert len({v.tobytes() for v in c.values}) > 4000  # seeded permutations: a handful may repeat


def test_family_c_is_tie_free():
    v = ww.family("C").values.reshape(-1, 9)
    assert (np.sort(v, axis=1) == (np.arange(1, 10, dtype=np.float32) / 16)[None]).all()


def test_every_window_is_flooded_completely():
    """The window is 4-connected and holds two seeds: the reference labels every pixel of it 1 or 2."""
    for name in ww.FAMILIES:
        e = ww.window_expected(name)
        assert e.dtype == np.int32 and ((e == 1) | (e == 2)).all(), name


def test_positions():
    assert ww.SEAM_POSITIONS == [(32, 32), (32, 64), (64, 32), (64, 64)]
    assert len(set(ww.PHASE_POSITIONS)) == 12 and not set(ww.PHASE_POSITIONS) & set(ww.SEAM_POSITIONS)
    assert set(ww.PHASE_POSITIONS) | set(ww.SEAM_POSITIONS) == set(itertools.product((1, 32, 63, 64), repeat=2))
    for name in ww.FAMILIES:
        hw = ww.family(name).values.shape[1:]
        for vector in (True, False):
            H, W = ww.frame_shape(hw, vector)
            assert W % 4 == (0 if vector else 2)
            for centre in ww.SEAM_POSITIONS + (ww.PHASE_POSITIONS if hw == (3, 3) else []):
                r0, c0 = ww.origin(centre, hw)
                assert 0 <= r0 and r0 + hw[0] <= H and 0 <= c0 and c0 + hw[1] <= W
                if centre in ww.SEAM_POSITIONS:  # the seam cuts the window (a corridor: across its long axis, in the middle)
                    assert hw[0] == 1 or r0 < centre[0] < r0 + hw[0]
                    assert hw[1] == 1 or c0 < centre[1] < c0 + hw[1]


def test_one_window_per_frame_is_labelled_like_the_window_alone():
    """The embedding property: the oracle on the full frame equals the window-alone labels placed at the window, nothing is
    labelled outside the mask.  1 200 seeded (family, window, position, width) draws."""
    rng = np.random.default_rng(1200)
    n_checked = 0
    for name in ww.FAMILIES:
        fam, exp = ww.family(name), ww.window_expected(name)
        hw = fam.values.shape[1:]
        positions = ww.SEAM_POSITIONS + (ww.PHASE_POSITIONS if hw == (3, 3) else [])
        for k in rng.choice(fam.values.shape[0], 240, replace=False):
            centre = positions[int(rng.integers(len(positions)))]
            shape = ww.frame_shape(hw, bool(rng.integers(2)))
            img, mk, mask, e = ww.host_frame(fam.values[k], fam.markers[k], exp[k], shape, centre)
            got = orc.watershed(img, mk, mask)
            assert not got[mask == 0].any()
            if not np.array_equal(got, e):
                r0, c0 = ww.origin(centre, hw)
                pytest.fail(ww.describe("family %s at %s in %s" % (name, centre, shape), int(k), fam.values[k], fam.markers[k],
                                        got[r0:r0 + hw[0], c0:c0 + hw[1]], exp[k]))
            n_checked += 1
    assert n_checked >= 1000


def test_nine_windows_per_frame_are_not_nine_frames():
    """Why every frame holds exactly one window.  The reference pushes every seed with age 0, and entries of equal (value,
    age) leave its binary heap in an order that depends on the heap's shape -- on everything else that is in it.  So nine
    copies of window 18 995 of family A, far apart in one 130 x 130 frame and each behind its own mask, are NOT labelled
    like the window alone: isolated regions of one frame influence each other through the heap."""
    fam, exp = ww.family("A"), ww.window_expected("A")
    k = 18995
    shape = (130, 130)
    img = np.full(shape, ww.OUTSIDE, np.float32)
    mk, mask, e = np.zeros(shape, np.int32), np.zeros(shape, np.uint8), np.zeros(shape, np.int32)
    for r, c in itertools.product((32, 64, 96), repeat=2):
        img[r - 1:r + 2, c - 1:c + 2] = fam.values[k]
        mk[r - 1:r + 2, c - 1:c + 2] = fam.markers[k]
        mask[r - 1:r + 2, c - 1:c + 2] = 1
        e[r - 1:r + 2, c - 1:c + 2] = exp[k]
    got = orc.watershed(img, mk, mask)
    assert not got[mask == 0].any() and (got[mask == 1] > 0).all()
    assert (got != e).sum() > 0
    one = ww.host_frame(fam.values[k], fam.markers[k], exp[k], shape, (64, 64))
    np.testing.assert_array_equal(orc.watershed(*one[:3]), one[3])  # ... while one copy in the same frame is


@pytest.mark.parametrize("shape", [(70, 130), (64, 128)])
def test_special_frames_are_sensitive(shape):
    """The signed-zero frame is labelled differently once -0.0 is a value below +0.0 (what a key made from the bits alone
    would do), the one-ulp frame once neighbouring floats are one level (what a key that loses the last bits would do).  A
    frame without that property would prove nothing on the device."""
    names, img, mk, mask, exp = ww.special_batch(shape)
    assert names[:2] == ["signed_zeros", "one_ulp"] and img.shape == (8,) + shape and img.dtype == np.float32
    sz = img[0]
    minus_zero = (sz == 0) & np.signbit(sz)
    assert minus_zero.sum() > 100 and ((sz == 0) & ~np.signbit(sz)).sum() > 100
    split = np.where(minus_zero, ww.NEG_SUBNORMAL, sz).astype(np.float32)
    assert (split[minus_zero] < 0).all()
    assert (orc.watershed(split, mk[0], mask[0]) != exp[0]).sum() > 0
    ulp = img[1]
    assert len(np.unique(ulp)) == 8 and np.abs(np.diff(np.unique(ulp)[4:]).astype(np.float64)).max() < 2e-7
    tied = np.sign(ulp).astype(np.float32)  # base + k ulp -> base = 1, -(base + k ulp) -> -1
    assert (orc.watershed(tied, mk[1], mask[1]) != exp[1]).sum() > 0


def test_special_frames_hold_every_special_value():
    for shape in [(70, 130), (64, 128)]:
        names, img, mk, mask, exp = ww.special_batch(shape)
        drawn = img[3:][mask[3:] > 0]
        for v in ww.SPECIAL_VALUES:
            assert ((drawn == v) & (np.signbit(drawn) == np.signbit(v))).any(), v
        assert not np.isnan(img).any()  # NaN is outside the contract of pcseg_watershed4_f32
        assert not exp[mask == 0].any()
