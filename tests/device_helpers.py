"""Device-side helpers shared by the GPU test files (no tests in here)."""
import threading

import numpy as np
import torch

import workspace_cases as wc


def shifted(t):
    """A copy of the CUDA tensor ``t`` whose base pointer lies one element (uint8: 1 byte, int32 / float32: 4 bytes) past a
    16-byte boundary: the kernels' 16-byte and 4-byte load paths do not apply to it."""
    item = t.element_size()
    buf = torch.empty(t.numel() + 32, dtype=t.dtype, device=t.device)
    start = ((item - buf.data_ptr()) % 16) // item
    out = buf[start:start + t.numel()].view(t.shape)
    assert out.data_ptr() % 16 == item and out.is_contiguous()
    out.copy_(t)
    return out


class Hooks:
    """ops._workspace and ops._call with a controlled prior state; ``begin`` a pass, run the case, ``finish`` it."""

    def __init__(self, ops, monkeypatch):
        self.real_workspace, self.real_call = ops._workspace, ops._call
        self.lock = threading.Lock()  # the pipeline launches from its lane threads
        self.watch = None             # ``watch(entry, args)``: called with every library call's arguments, before the call
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
        if self.watch is not None:
            self.watch(entry, args)
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


def to_device(x):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in x.items()}


def settled(out):
    """the outputs as copies of their own (some are views of buffers a later pass reuses), private entries apart"""
    torch.cuda.synchronize()
    return {k: (v.clone() if isinstance(v, torch.Tensor) else np.array(v, copy=True)) for k, v in out.items() if not k.startswith("_")}


def to_host(out):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _bytes(v):
    return v.cpu().numpy().tobytes() if isinstance(v, torch.Tensor) else np.ascontiguousarray(v).tobytes()


def same(case, shape, name, got, want):
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
