"""What a wrapper computes does not depend on how its inputs lie in memory, and no wrapper writes to an input.

Every case of tests/workspace_cases.py (``long_lists`` apart: its point is the list length, and it is the one case above the
small shapes) runs once with plain inputs -- freshly made, contiguous, 256-byte aligned: what every other test hands the
library -- and is held against its CPU reference; then once per layout below with every input the layout applies to replaced
by the same values in that layout.  Each such run must give the plain run's outputs bit for bit (the outputs a case lists as
``unordered``: within the reordering bound of ``device_helpers.same``, the rule of the workspace test), must leave the inputs
-- and the buffers they are views of -- as they were, and hands the library only what the contract of DESIGN.md ("The argument
contract of ops") allows: the images that go through ``ops._plane_view`` are read in place where their rows are dense (the
pointer handed over is the view's, the frame stride its ``stride(0)``), every other tensor argument of every library call is
contiguous.  The in/out tensors of a case are made inside its ``run`` and stay contiguous: their misuse is refused
(tests/ops_contract_cases.py)."""
import numpy as np
import pytest

import workspace_cases as wc
from device_helpers import Hooks, same, settled, shifted, to_host

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEED = 5
FILL = 0x5A  # what the bytes around a view hold

# the arguments that go through ops._plane_view: entry -> (position of the image, position of its frame stride)
PLANE_ARGS = {"edt_sq_lt_f32": (0, 1), "watershed4_f32": (0, 1), "label_borders": (1, 2)}
PIPELINE_LAYOUTS = ("shifted", "padded")  # FramePipeline.run: any (B, C, H, W) float32 device tensor; graph mode is not part of this


def _filled(shape, dtype):
    return torch.full((int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size(),), FILL, dtype=torch.uint8,
                      device="cuda").view(dtype).view(shape)


def lay_shifted(t):
    v = shifted(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size() and v.stride() == t.stride()
    return v, v


def lay_padded(t):
    """a view into a wider buffer: columns 1 .. W of a last dimension W + 3; 1-D: every second element"""
    if t.dim() == 1:
        big = _filled((2 * t.shape[0],), t.dtype)
        v = big[::2]
        assert v.stride() == (2,)
    else:
        W = t.shape[-1]
        big = _filled(tuple(t.shape[:-1]) + (W + 3,), t.dtype)
        v = big[..., 1:1 + W]
        assert v.stride() == big.stride() and v.stride(-1) == 1 and v.stride(-2) == W + 3
        assert v.data_ptr() == big.data_ptr() + t.element_size()
    assert v.shape == t.shape and not v.is_contiguous()
    v.copy_(t)
    return v, big


def lay_frame_strided(t):
    """rows dense, frames one element further apart than H W: an odd frame stride"""
    B, H, W = t.shape
    big = _filled((B, H * W + 1), t.dtype)
    v = big[:, :H * W].view(B, H, W)
    assert v.stride() == (H * W + 1, W, 1) and v.data_ptr() == big.data_ptr() and v.data_ptr() % 16 == 0 and not v.is_contiguous()
    v.copy_(t)
    return v, big


def lay_plane(t):
    """plane 1 of a (B, 3, H, W) stack"""
    B, H, W = t.shape
    big = _filled((B, 3, H, W), t.dtype)
    v = big[:, 1]
    assert v.stride() == (3 * H * W, W, 1) and v.data_ptr() == big.data_ptr() + 4 * H * W and not v.is_contiguous()
    v.copy_(t)
    return v, big


def lay_bool(t):
    v = t.to(torch.bool)
    assert v.dtype == torch.bool and v.is_contiguous() and v.data_ptr() % 16 == 0 and bool((v.view(torch.uint8) == t).all())
    return v, v


# name -> (applies to a host input?, the layout, read in place by _plane_view?)
LAYOUTS = {
    "shifted": (lambda a: a.size > 0, lay_shifted, False),
    "padded": (lambda a: a.size > 0 and a.ndim >= 1, lay_padded, False),
    "frame_strided": (lambda a: a.ndim == 3 and a.shape[0] > 1, lay_frame_strided, True),
    "plane": (lambda a: a.ndim == 3 and a.dtype == np.float32 and a.shape[0] > 1, lay_plane, True),
    "bool": (lambda a: a.dtype == np.uint8 and a.size > 0 and int(a.max()) <= 1, lay_bool, False),
}


def _as_bytes(t):
    return (t.view(torch.uint8) if t.dtype == torch.bool else t).cpu().numpy().tobytes()


class Watch:
    """what ``Hooks.call`` shows of every library call: the tensor arguments, by entry and position"""

    def __init__(self):
        self.calls = []

    def __call__(self, entry, args):
        self.calls.append((entry, args))

    def check(self, in_place):
        """``in_place``: data_ptr -> (frame stride, row length) of the inputs a plane argument must be read in place from"""
        seen_in_place = set()
        for entry, args in self.calls:
            plane = PLANE_ARGS.get(entry, (None, None))
            for i, a in enumerate(args):
                if not isinstance(a, torch.Tensor):
                    continue
                if i != plane[0]:
                    assert a.is_contiguous(), "pcseg_%s: argument %d is handed over with strides %s" % (entry, i, a.stride())
                    continue
                B, H, W = a.shape
                assert a.stride(2) == 1 and a.stride(1) == W and (B == 1 or a.stride(0) >= H * W), (entry, a.stride())
                assert args[plane[1]] == (a.stride(0) if B > 1 else H * W), (entry, args[plane[1]], a.stride())
                if a.data_ptr() in in_place:
                    assert a.stride(0) == in_place[a.data_ptr()], (entry, a.stride())
                    seen_in_place.add(a.data_ptr())
        return seen_in_place


@pytest.fixture
def hooks(monkeypatch):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")
    from particle_col_image_segmentation_amd import ops
    return ops, Hooks(ops, monkeypatch)


def _run(ops, h, case, x):
    watch = Watch()
    h.begin("zeros", {})
    h.watch = watch
    raw = case.run(ops, x)
    h.finish()
    h.watch = None
    return raw, settled(raw), watch


def _ids():
    return [pytest.param(case, shape, id="%s-%dx%dx%d" % ((case.name,) + shape))
            for case in wc.CASES if case.name != "long_lists" for shape in case.shapes]


@pytest.mark.parametrize("case,shape", _ids())
def test_a_result_does_not_depend_on_the_layout_of_the_inputs(hooks, case, shape):
    ops, h = hooks
    pipeline = case.name.startswith("pipeline")
    x_host = case.build(shape, SEED)
    plain = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in x_host.items()}
    assert all(t.is_contiguous() and t.data_ptr() % 256 == 0 for t in plain.values())
    raw, base, watch = _run(ops, h, case, plain)
    if case.check is not None:
        case.check(x_host, dict(to_host(base), **{k: v for k, v in raw.items() if k.startswith("_")}))
    watch.check({})
    del raw
    ran = []
    for name, (applies, lay, in_place) in LAYOUTS.items():
        if pipeline and name not in PIPELINE_LAYOUTS:
            continue
        keys = [k for k, v in x_host.items() if applies(v) and (not pipeline or k == "stack")]
        if not keys:
            continue
        ran.append(name)
        x, bases = dict(plain), {}
        for k in keys:
            x[k], bases[k] = lay(plain[k])
        before = {k: _as_bytes(b) for k, b in bases.items()}
        torch.cuda.synchronize()
        _, out, watch = _run(ops, h, case, x)
        # the inputs, and the buffers around them, are what they were
        for k in keys:
            assert _as_bytes(bases[k]) == before[k], "%s under %s: the buffer of input %r was written to" % (case.name, name, k)
            assert _as_bytes(x[k]) == np.ascontiguousarray(x_host[k]).tobytes(), "%s under %s: input %r changed" % (case.name, name, k)
        for k in x_host:
            if k not in keys:
                assert _as_bytes(plain[k]) == np.ascontiguousarray(x_host[k]).tobytes(), "%s under %s: input %r changed" % (case.name, name, k)
        # ... what the library was handed is what the contract allows
        views = {x[k].data_ptr(): x[k].stride(0) for k in keys if in_place and x[k].dtype == torch.float32}
        read_in_place = watch.check(views)
        if any(e in PLANE_ARGS for e, _ in watch.calls) and not pipeline:
            assert read_in_place == set(views), "%s under %s: a plane argument was copied, not read in place" % (case.name, name)
        # ... and the outputs are the plain run's
        assert sorted(out) == sorted(base)
        differ = [k for k in sorted(out) if not same(case, shape, k, out[k], base[k])]
        assert not differ, "%s: %s differ(s) from the plain run when the inputs are %s" % (case.name, differ, name)
    assert "shifted" in ran and "padded" in ran


def test_the_layouts_are_what_they_claim_and_every_one_is_used():
    """every layout applies to an input of some case (none is dead), and the plane arguments meet both in-place layouts"""
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")
    used = {name: [] for name in LAYOUTS}
    for case in wc.CASES:
        if case.name in ("long_lists", "pipeline", "pipeline_ties"):
            continue
        x_host = case.build(case.shapes[0], SEED)
        for name, (applies, _, _) in LAYOUTS.items():
            if any(applies(v) for v in x_host.values()):
                used[name].append(case.name)
    assert all(used.values()), used
    for name in ("frame_strided", "plane"):
        assert {"edt_lt", "watershed", "borders"} <= set(used[name])
    assert {"edt", "fill_holes", "watershed", "remove_overlapping", "nearest_label", "surface_shells"} <= set(used["bool"])
    t = torch.arange(2 * 5 * 7, dtype=torch.float32, device="cuda").view(2, 5, 7)
    for name, (_, lay, _) in LAYOUTS.items():
        if name == "bool":
            continue
        v, _ = lay(t)
        assert torch.equal(v, t), name
