"""No entry's result depends on what its workspace held before the call, and no entry writes past the size its query named.

Every workspace of ``ops`` comes from ``ops._workspace``; inside a test that function is replaced (pytest's monkeypatch) by one
that asks the real size query, hands out ``align256(nbytes) + 4096`` bytes filled according to the current state and tells the
library the true size.  The cases of tests/workspace_cases.py run under four states in this order -- zeros (what a fresh
process tends to get), the bytes the same entry left after a call on other data of the same shape, the bytes it left at
another shape (stale regions land in other regions), every byte 0xFF -- and must give, bit for bit, what they gave under
zeros, which in turn is held against the CPU reference.  The 4096 bytes behind every workspace must keep their fill."""
import threading

import numpy as np
import pytest

import workspace_cases as wc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEED = 5


class Hooks:
    """ops._workspace and ops._call with a controlled prior state; ``begin`` a pass, run the case, ``finish`` it."""

    def __init__(self, ops, monkeypatch):
        self.real_workspace, self.real_call = ops._workspace, ops._call
        self.lock = threading.Lock()  # the pipeline launches from its lane threads
        self.begin("zeros", {})
        monkeypatch.setattr(ops, "_workspace", self.workspace)
        monkeypatch.setattr(ops, "_call", self.call)

    def begin(self, state, donors):
        self.state, self.donors = state, donors
        self.handed, self.seen, self.ordinal, self.by_ptr, self.snaps = [], [], {}, {}, {}

    def workspace(self, entry, device, *query):
        _, nbytes = self.real_workspace(entry, device, *query)  # the real size query; its buffer is dropped
        with self.lock:
            key = (entry, self.ordinal.get(entry, 0))
            self.ordinal[entry] = key[1] + 1
        fill = wc.state_fill(self.state, nbytes, wc.donor(self.donors, key))
        whole = torch.from_numpy(fill).to(device)  # (on the current stream, like the call that follows)
        with self.lock:
            self.handed.append((key, nbytes, whole, wc.red_zone(fill, nbytes)))
            self.by_ptr[whole.data_ptr()] = (key, nbytes)
        return whole[:max(nbytes, 256)], nbytes  # what ops._ws would have returned: its numel() is handed on by some callers

    def call(self, entry, *args, ws=None):
        with self.lock:
            self.seen.append("pcseg_" + entry)
        pair = self.real_call(entry, *args, ws=ws)
        if pair is not None:
            known = self.by_ptr.get(pair[0].data_ptr())
            if known is not None:  # what the last call on this workspace leaves in it, cloned on the call's stream
                self.snaps[known[0]] = pair[0][:known[1]].clone()
        return pair

    def finish(self):
        """Waits for the device; returns (entries seen, leftovers by (entry, ordinal), touched red zones as messages)."""
        torch.cuda.synchronize()
        touched = []
        for key, nbytes, whole, want in self.handed:
            got = wc.red_zone(whole, nbytes).cpu().numpy()
            at = wc.first_changed(got, want)
            if at >= 0:
                touched.append("%s (call %d, %d bytes): red zone byte %d is 0x%02x, was 0x%02x" % (key[0], key[1], nbytes, at, got[at], want[at]))
        snaps = {k: v.cpu().numpy() for k, v in self.snaps.items()}
        return set(self.seen), snaps, touched


@pytest.fixture
def hooks(monkeypatch):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")
    from particle_col_image_segmentation_amd import ops
    return ops, Hooks(ops, monkeypatch)


def _device(x):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in x.items()}


def _settled(out):
    """the outputs as copies of their own (some are views of buffers a later pass reuses), private entries apart"""
    torch.cuda.synchronize()
    return {k: (v.clone() if isinstance(v, torch.Tensor) else np.array(v, copy=True)) for k, v in out.items() if not k.startswith("_")}


def _host(out):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _bytes(v):
    return v.cpu().numpy().tobytes() if isinstance(v, torch.Tensor) else np.ascontiguousarray(v).tobytes()


def _same(case, shape, name, got, want):
    """bit for bit; an output the case lists as unordered: bit for bit in front of its first unordered column, within the
    reordering bound of a float64 sum from there on"""
    assert type(got) is type(want) and got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), name
    if name not in case.unordered:
        return _bytes(got) == _bytes(want)  # by their bits: NaN rows and signed zeros included, uint16 too
    col = case.unordered[name]
    g, w = (v.cpu().numpy() if isinstance(v, torch.Tensor) else v for v in (got, want))
    g, w = g.reshape(-1, g.shape[-1]), w.reshape(-1, w.shape[-1])
    if g[:, :col].tobytes() != w[:, :col].tobytes():
        return False
    # a ratio column is a quotient of two such sums: twice the bound, and the division's rounding
    return bool(np.allclose(g[:, col:], w[:, col:], rtol=4 * wc.sum_rtol(shape), atol=0, equal_nan=True))


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
