"""The CPU half of the workspace-state test (tests/workspace_cases.py): every entry that takes a workspace is claimed by a case,
the input builders are deterministic, and the prior states are what they say.  No GPU needed."""
import numpy as np
import pytest

import workspace_cases as wc
from particle_col_image_segmentation_amd import _lib


def test_every_workspace_entry_is_claimed_by_a_case():
    """a new entry in _lib.WORKSPACE / WORKSPACE_HANDED_ON fails here until a case drives it"""
    declared = set()
    for case in wc.CASES:
        declared |= set(case.entries)
    assert declared == set(_lib.WORKSPACE) | set(_lib.WORKSPACE_HANDED_ON), (
        sorted(declared ^ (set(_lib.WORKSPACE) | set(_lib.WORKSPACE_HANDED_ON))))


def test_case_names_are_unique_and_cases_are_complete():
    names = [case.name for case in wc.CASES]
    assert len(names) == len(set(names))
    for case in wc.CASES:
        assert case.entries and case.shapes and callable(case.build) and callable(case.run), case.name
        assert case.check is not None or case.note, "%s: a case without reference says why" % case.name
        for shape in case.shapes:
            assert wc.other_shape(case, shape) != shape, case.name


def test_the_shapes_cross_the_seams_they_are_chosen_for():
    B, H, W = wc.PRIMARY
    assert H % 32 and (H + 31) // 32 == 3 and W % 4 and W % 64 and H % 32  # ragged words and tiles, the scalar load routes
    B2, H2, W2 = wc.SECOND
    assert H2 % 32 == 0 and W2 % 64 == 0 and W2 % 4 == 0 and B2 != B         # full tiles, the wide routes
    assert wc.PIPELINE[2] % 4 == 0 and wc.PIPELINE_DONOR[2] % 4                # the fused and the ragged plane sums


@pytest.mark.parametrize("case", wc.CASES, ids=lambda c: c.name)
def test_builders_are_deterministic(case):
    for shape in case.shapes[:1] if case.name.startswith("pipeline") else case.shapes:
        a, b, c = case.build(shape, 3), case.build(shape, 3), case.build(shape, 4)
        assert sorted(a) == sorted(b)
        differs = False
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (case.name, k)
            differs = differs or a[k].tobytes() != c[k].tobytes()
        assert differs, "%s: another seed gives the same data" % case.name


def test_align_and_sizes():
    assert [wc.align256(n) for n in (0, 1, 255, 256, 257, 1 << 20)] == [0, 256, 256, 256, 512, 1 << 20]
    for nbytes in (0, 1, 256, 257, 1000, 4096, 65536 + 256):
        body = wc.body_bytes(nbytes)
        assert body % 256 == 0 and body >= max(nbytes, 256) and body - max(nbytes, 256) < 256
        assert wc.padded_bytes(nbytes) == body + wc.RED_ZONE
        if nbytes and nbytes % 256 == 0:
            assert body == wc.align256(nbytes) == nbytes  # the library's sizes are whole carve units: the red zone follows at once


def test_stretch_repeats_and_truncates():
    snap = np.arange(1, 8, dtype=np.uint8)
    assert wc.stretch(snap, 3).tolist() == [1, 2, 3]
    assert wc.stretch(snap, 7).tolist() == snap.tolist()
    long = wc.stretch(snap, 17)
    assert long.dtype == np.uint8 and long.tolist() == (snap.tolist() * 3)[:17]
    assert wc.stretch(np.zeros(0, np.uint8), 5).tolist() == [0] * 5
    assert wc.stretch(snap.reshape(7, 1), 9).shape == (9,)
    assert wc.stretch(snap, 0).size == 0


def test_state_fills():
    assert wc.STATES == ("zeros", "leftover-same", "leftover-other", "ones")
    snap = (np.arange(1000) % 251 + 1).astype(np.uint8)
    for nbytes in (256, 768, 5120):
        n = wc.padded_bytes(nbytes)
        z, o = wc.state_fill("zeros", nbytes), wc.state_fill("ones", nbytes)
        assert z.dtype == o.dtype == np.uint8 and z.shape == o.shape == (n,)
        assert not z.any() and (o == 0xFF).all()
        assert wc.red_zone(o, nbytes).shape == (wc.RED_ZONE,) and n - wc.RED_ZONE == wc.body_bytes(nbytes)
        for state in ("leftover-same", "leftover-other"):
            f = wc.state_fill(state, nbytes, snap)
            assert f.shape == (n,) and f.tolist() == wc.stretch(snap, n).tolist()
            assert f[:min(n, 1000)].tolist() == snap[:min(n, 1000)].tolist()
            # the red zone continues the pattern: a write of the leftover's own bytes past the end would still show
            assert wc.red_zone(f, nbytes).tolist() == wc.stretch(snap, n)[wc.body_bytes(nbytes):].tolist()
            assert wc.red_zone(f, nbytes).all()
            assert not wc.state_fill(state, nbytes, None).any()
    with pytest.raises(ValueError):
        wc.state_fill("random", 256)


def test_first_changed_and_donor():
    a = np.zeros(16, np.uint8)
    b = a.copy()
    assert wc.first_changed(a, b) == -1
    b[5] = b[9] = 1
    assert wc.first_changed(b, a) == 5
    snaps = {("edt_sq_u8", 0): np.ones(4, np.uint8), ("edt_sq_u8", 1): np.full(4, 2, np.uint8), ("ccl8_bool", 0): np.full(4, 3, np.uint8)}
    assert wc.donor(snaps, ("edt_sq_u8", 1))[0] == 2
    assert wc.donor(snaps, ("edt_sq_u8", 7))[0] == 1      # the calls of two shapes need not pair up: the entry's first
    assert wc.donor(snaps, ("fill_holes", 0))[0] == 3     # ... else any other entry's bytes
    assert wc.donor({}, ("fill_holes", 0)) is None


def test_sum_bound_is_the_reordering_bound():
    H, W = wc.PIPELINE[1:]
    assert wc.sum_rtol(wc.PIPELINE) == H * W * 2.0 ** -52 < 1e-11
