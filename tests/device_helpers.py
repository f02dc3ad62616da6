"""Device-side helpers shared by the GPU test files (no tests in here)."""
import collections
import sys
import threading

import numpy as np
import torch

import output_cases as oc
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


_NUMPY_OF = {torch.uint8: np.uint8, torch.bool: np.uint8, torch.int8: np.int8, torch.int16: np.int16, torch.uint16: np.uint16,
             torch.int32: np.int32, torch.int64: np.int64, torch.float32: np.float32, torch.float64: np.float64}
_OWN_FILL = ("zeros", "zeros_like", "full")   # the calls that keep their own fill between the red zones


class TorchProxy:
    """What ``OutputHooks`` puts in the place of the name ``torch`` inside a module: every attribute is the real torch's,
    but ``empty`` / ``empty_like`` / ``zeros`` / ``zeros_like`` / ``full`` go through the hooks first."""

    def __init__(self, hooks):
        self._hooks = hooks

    def __getattr__(self, name):  # (only what the class does not define arrives here)
        return getattr(torch, name)

    def empty(self, *args, **kwargs):
        return self._hooks.allocate("empty", args, kwargs)

    def empty_like(self, *args, **kwargs):
        return self._hooks.allocate("empty_like", args, kwargs)

    def zeros(self, *args, **kwargs):
        return self._hooks.allocate("zeros", args, kwargs)

    def zeros_like(self, *args, **kwargs):
        return self._hooks.allocate("zeros_like", args, kwargs)

    def full(self, *args, **kwargs):
        return self._hooks.allocate("full", args, kwargs)


Handed = collections.namedtuple("Handed", "wrapper call shape dtype nbytes whole tensor state")


def _cuda(device):
    return device is not None and torch.device(device).type == "cuda"


def modelled(call, args, kwargs):
    """``(shape, dtype, device, value)`` of an allocation the hooks pad -- a dense CUDA tensor of at least one element, asked
    for with nothing but a size (or a contiguous tensor to be like), ``dtype`` and ``device`` -- or None: the call goes to
    torch as it stands (host and pinned memory, zero-size tensors, ``out=`` / ``layout=`` / ``memory_format=`` / ...)."""
    kw = dict(kwargs)
    value = kw.pop("fill_value", None)
    if set(kw) - {"dtype", "device"}:
        return None
    if call in ("empty_like", "zeros_like"):
        if len(args) != 1 or not isinstance(args[0], torch.Tensor) or not args[0].is_contiguous() or args[0].layout != torch.strided:
            return None
        like = args[0]
        shape, dtype, device = tuple(like.shape), kw.get("dtype") or like.dtype, kw.get("device", like.device)
    else:
        if call == "full":
            if len(args) == 2 and value is None:
                args, value = args[:1], args[1]
            if len(args) != 1 or isinstance(value, torch.Tensor) or value is None:
                return None
        shape = args[0] if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)) else args
        if not all(type(v) is int and v >= 0 for v in shape):
            return None
        shape = tuple(shape)
        dtype = kw.get("dtype") or (torch.full((), value).dtype if call == "full" else torch.get_default_dtype())
        device = kw.get("device")
    if not _cuda(device) or dtype not in _NUMPY_OF or int(np.prod(shape, dtype=np.int64)) == 0:
        return None
    return shape, dtype, torch.device(device), value


class OutputHooks:
    """Every output ``ops`` and ``pipeline`` allocate, in a controlled prior state and between two red zones: the name ``torch``
    inside ``modules`` is replaced by a :class:`TorchProxy`.  ``begin`` a pass in one of ``output_cases.OUTPUT_STATES``, run
    the case, ``finish`` it.  An allocation is one uint8 buffer ``[RED_ZONE][body][RED_ZONE]`` (output_cases.output_fill)
    whose body -- 256-byte aligned, as an allocator block is: the kernels pick their vector routes from the address -- is
    handed out as a contiguous view of the dtype and shape asked for.  Every buffer is kept until the next ``begin``.  (A
    workspace that ``ops._ws`` allocates is padded like any other ``torch.empty``; beside :class:`Hooks` that is only the
    buffer of the real size query, which is dropped.)"""

    def __init__(self, modules, monkeypatch):
        self.lock = threading.Lock()  # the pipeline launches from its lane threads
        self.proxy = TorchProxy(self)
        self.begin("zeros")
        for module in modules:
            assert module.torch is torch, module.__name__
            monkeypatch.setattr(module, "torch", self.proxy)

    def begin(self, state):
        assert state in oc.OUTPUT_STATES, state
        self.state, self.handed = state, []

    def allocate(self, call, args, kwargs):
        spec = modelled(call, args, kwargs)
        if spec is None:
            return getattr(torch, call)(*args, **kwargs)
        shape, dtype, device, value = spec
        frame = sys._getframe(2)  # the function that wrote ``torch.empty(...)``: above lambdas and comprehensions
        while frame.f_code.co_name.startswith("<") and frame.f_back is not None:
            frame = frame.f_back
        state = self.state
        nbytes = int(np.prod(shape, dtype=np.int64)) * _NUMPY_OF[dtype]().itemsize
        # (filled on the current stream, like the call that follows)
        whole = torch.from_numpy(oc.output_fill(state, _NUMPY_OF[dtype], nbytes)).to(device)
        tensor = whole[wc.RED_ZONE:wc.RED_ZONE + nbytes].view(dtype).view(shape)
        assert tensor.is_contiguous() and (tensor.data_ptr() % 256 == 0 or not tensor.is_cuda)  # (host memory: the CPU self-test)
        if call in _OWN_FILL:
            tensor.fill_(value) if call == "full" else tensor.zero_()
        with self.lock:
            self.handed.append(Handed(frame.f_code.co_name, call, shape, dtype, nbytes, whole, tensor, state))
        return tensor

    def finish(self):
        """Waits for the device; returns the touched red zones as messages."""
        torch.cuda.synchronize()
        touched = []
        for h in self.handed:
            want = oc.output_fill(h.state, _NUMPY_OF[h.dtype], h.nbytes)
            got = torch.cat([h.whole[:wc.RED_ZONE], h.whole[wc.RED_ZONE + h.nbytes:]]).cpu().numpy()
            for side, g, w, origin in (("front", got[:wc.RED_ZONE], want[:wc.RED_ZONE], -wc.RED_ZONE),
                                       ("back", got[wc.RED_ZONE:], want[wc.RED_ZONE + h.nbytes:], 0)):
                at = wc.first_changed(g, w)
                if at >= 0:  # front: bytes before the output's first (negative), back: bytes past its end
                    touched.append("%s: torch.%s of %s %s, %s red zone byte %d is 0x%02x, was 0x%02x"
                                   % (h.wrapper, h.call, h.shape, str(h.dtype).replace("torch.", ""), side, at + origin, g[at], w[at]))
        return touched


def not_left(t, defined, state):
    """Indices (k, t.dim()) of the elements of ``t`` outside ``defined`` -- a bool tensor over the leading dimensions of ``t``,
    True where the call defines the element -- that no longer hold the fill of ``state``: what an entry promises to leave
    untouched was handed out holding that fill (by their bytes: a NaN fill too)."""
    fill = torch.from_numpy(oc.fill_pattern(state, _NUMPY_OF[t.dtype])).to(t.device)
    changed = (t.contiguous().view(torch.uint8).reshape(tuple(t.shape) + (fill.numel(),)) != fill).any(dim=-1)
    outside = ~defined.reshape(tuple(defined.shape) + (1,) * (t.dim() - defined.dim())).expand(t.shape)
    return torch.nonzero(changed & outside)


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
