"""No entry's result depends on what its workspace held before the call, and no entry writes past the size its query named.

Every workspace of ``ops`` comes from ``ops._workspace``; inside a test that function is replaced (pytest's monkeypatch) by one
that asks the real size query, hands out ``align256(nbytes) + 4096`` bytes filled according to the current state and tells the
library the true size.  The cases of tests/workspace_cases.py run under four states in this order -- zeros (what a fresh
process tends to get), the bytes the same entry left after a call on other data of the same shape, the bytes it left at
another shape (stale regions land in other regions), every byte 0xFF -- and must give, bit for bit, what they gave under
zeros, which in turn is held against the CPU reference.  The 4096 bytes behind every workspace must keep their fill."""
import pytest

import workspace_cases as wc
from device_helpers import Hooks, to_device as _device, settled as _settled, to_host as _host, same as _same

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEED = 5


@pytest.fixture
def hooks(monkeypatch):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")
    from particle_col_image_segmentation_amd import ops
    return ops, Hooks(ops, monkeypatch)


_LEFTOVERS = {}  # (case, shape) -> the workspaces a recording pass left, shared by the cases that need them


def _leftovers(ops, h, case, shape):
    """what every workspace of the case holds after a run on OTHER data of ``shape`` (itself a run under zeros)"""
    key = (case.name, shape)
    if key not in _LEFTOVERS:
        h.begin("zeros", {})
        case.run(ops, _device(case.build(shape, SEED + 1)))
        _, snaps, touched = h.finish()
        assert not touched, touched
        assert snaps, "the recording pass of %s saw no workspace" % case.name
        _LEFTOVERS[key] = snaps
    return _LEFTOVERS[key]


def _ids():
    return [pytest.param(case, shape, id="%s-%dx%dx%d" % ((case.name,) + shape)) for case in wc.CASES for shape in case.shapes]


@pytest.mark.parametrize("case,shape", _ids())
def test_prior_workspace_contents_never_reach_a_result(hooks, case, shape):
    ops, h = hooks
    donors = {"zeros": {}, "ones": {}, "leftover-same": _leftovers(ops, h, case, shape),
              "leftover-other": _leftovers(ops, h, case, wc.other_shape(case, shape))}
    x_host = case.build(shape, SEED)
    x = _device(x_host)
    base = None
    for state in wc.STATES:
        h.begin(state, donors[state])
        raw = case.run(ops, x)
        seen, _, touched = h.finish()
        out = _settled(raw)
        assert not touched, "%s under %s wrote behind its workspace: %s" % (case.name, state, touched)
        assert set(case.entries) <= seen, "%s did not drive %s" % (case.name, sorted(set(case.entries) - seen))
        if state == "zeros":
            base = out
            if case.check is not None:
                case.check(x_host, dict(_host(out), **{k: v for k, v in raw.items() if k.startswith("_")}))
            continue
        assert sorted(out) == sorted(base)
        differ = [k for k in sorted(out) if not _same(case, shape, k, out[k], base[k])]
        assert not differ, "%s: %s differ(s) from the zeros run when the workspaces start as %s" % (case.name, differ, state)


def test_the_hooks_see_every_workspace_and_a_write_behind_it(hooks):
    """the hooks are the choke point they are taken for: one call, one workspace of the queried size in front of an intact red
    zone, its leftover recorded -- and a byte changed behind it is reported with the entry's name and the offset"""
    ops, h = hooks
    from particle_col_image_segmentation_amd import _lib
    h.begin("zeros", {})
    x = torch.zeros((1, 40, 40), dtype=torch.uint8, device="cuda")
    x[0, 5:30, 5:30] = 1
    x[0, 10:20, 10:20] = 0
    filled = ops.fill_holes(x)
    seen, snaps, touched = h.finish()
    assert seen == {"pcseg_fill_holes"} and list(snaps) == [("fill_holes", 0)] and not touched
    nbytes = _lib.load().pcseg_fill_holes_workspace_bytes(1, 40, 40)
    assert snaps[("fill_holes", 0)].shape == (nbytes,) and h.handed[0][1] == nbytes
    assert h.handed[0][2].numel() == wc.padded_bytes(nbytes) and h.handed[0][2].data_ptr() % 256 == 0
    assert int(filled.sum()) == 25 * 25
    # a write behind the workspace is seen, and named
    h.begin("ones", {})
    ops.fill_holes(x)
    h.handed[0][2][wc.body_bytes(nbytes) + 7] = 0
    _, _, touched = h.finish()
    assert len(touched) == 1 and "fill_holes" in touched[0] and "byte 7 " in touched[0]
