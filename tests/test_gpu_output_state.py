"""No result depends on what an OUTPUT buffer held before the call, and nothing outside an output is written.

``ops`` and ``pipeline`` allocate their outputs with ``torch.empty`` / ``torch.empty_like`` and fill only a few; fresh device
memory is usually zero, so a kernel that relies on that passes every other test and fails on a recycled block.  Inside a test
the name ``torch`` of both modules is a forwarding proxy (device_helpers.OutputHooks): every CUDA allocation lies between two
red zones of 4096 bytes and starts in a chosen state.  The cases of tests/output_cases.py -- every compute entry of the library
-- run under three states in this order: zeros (held against the CPU reference), every byte 0xFF, every element 1 of its own
dtype; the defined outputs of the last two must equal those of the first bit for bit, no red zone may change, and what
include/pcseg.h promises to leave untouched must still hold the fill.  The workspaces stay in their zeros state throughout
(test_gpu_workspace_state.py varies them): the two properties stay separate."""
import pytest

import output_cases as oc
import workspace_cases as wc
from device_helpers import (Hooks, OutputHooks, not_left, to_device as _device, settled as _settled, to_host as _host, same as _same)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEED = 5


@pytest.fixture
def hooks(monkeypatch):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")
    from particle_col_image_segmentation_amd import ops, pipeline
    return ops, Hooks(ops, monkeypatch), OutputHooks((ops, pipeline), monkeypatch)


def _ids():
    return [pytest.param(case, shape, id="%s-%dx%dx%d" % ((case.name,) + shape)) for case in oc.CASES for shape in case.shapes]


def _overwritten(raw, state):
    """the outputs of ``_raw`` with an element outside their defined part that no longer holds the state's fill"""
    bad = []
    for name, (t, defined) in sorted(raw.get("_raw", {}).items()):
        assert not bool(defined.all()), "%s: every element is defined, nothing is left to watch" % name
        at = not_left(t, defined, state)
        if at.shape[0]:
            bad.append("%s: %d element(s), the first at %s" % (name, at.shape[0], tuple(int(v) for v in at[0])))
    return bad


@pytest.mark.parametrize("case,shape", _ids())
def test_prior_output_contents_never_reach_a_result(hooks, case, shape):
    ops, ws, outputs = hooks
    x_host = case.build(shape, SEED)
    x = _device(x_host)
    base = None
    for state in oc.OUTPUT_STATES:
        ws.begin("zeros", {})
        outputs.begin(state)
        raw = case.run(ops, x)
        seen, _, behind_workspace = ws.finish()
        touched = outputs.finish()
        out = _settled(raw)
        assert outputs.handed, "%s allocated nothing through the hooks" % case.name
        assert not touched, "%s with outputs starting as %s wrote outside an output: %s" % (case.name, state, touched)
        assert not behind_workspace, behind_workspace
        assert set(case.entries) <= seen, "%s did not drive %s" % (case.name, sorted(set(case.entries) - seen))
        assert set(oc.PROMISES.get(case.name, ())) <= set(raw.get("_raw", {})), "%s no longer watches what it is listed for" % case.name
        if state == "zeros":
            base = out
            if case.check is not None:
                case.check(x_host, dict(_host(out), **{k: v for k, v in raw.items() if k.startswith("_")}))
            continue
        assert sorted(out) == sorted(base)
        differ = [k for k in sorted(out) if not _same(case, shape, k, out[k], base[k])]
        assert not differ, "%s: %s differ(s) from the zeros run when the outputs start as %s" % (case.name, differ, state)
        overwritten = _overwritten(raw, state)
        assert not overwritten, "%s with outputs starting as %s wrote what it promises to leave: %s" % (case.name, state, overwritten)


def test_the_hooks_pad_every_output_and_see_a_write_on_either_side(hooks):
    """the proxy is the choke point it is taken for: one call, its outputs handed out of padded buffers of the expected size,
    alignment and fill -- and a byte changed in front of an output or behind it is reported with the wrapper's name, the side
    and the offset"""
    ops, ws, outputs = hooks
    assert ops.torch is outputs.proxy and ops.torch.float64 is torch.float64 and ops.torch.cuda is torch.cuda
    x = torch.zeros((1, 40, 40), dtype=torch.uint8, device="cuda")
    x[0, 5:30, 5:30] = 1
    x[0, 10:20, 10:20] = 0
    for state, body, zone in (("zeros", 0, 0xFF), ("ones", 0xFF, 0xFF), ("unit", 1, 1)):
        ws.begin("zeros", {})
        outputs.begin(state)
        probe = ops.torch.empty((3, 5), dtype=torch.uint8, device="cuda")  # (what a wrapper's output holds before its call)
        assert probe.cpu().tolist() == [[body] * 5] * 3
        filled = ops.fill_holes(x)
        assert not outputs.finish() and ws.finish()[0] == {"pcseg_fill_holes"}
        # (the third: the buffer that ops._ws makes for the real size query, which the workspace hooks drop for their own)
        assert [(h.wrapper, h.call, h.shape, h.dtype) for h in outputs.handed[1:]] == [
            ("fill_holes", "empty_like", (1, 40, 40), torch.uint8), ("_ws", "empty", (ws.handed[0][1],), torch.uint8)]
        h = outputs.handed[1]
        assert h.nbytes == 1600 and h.whole.numel() == 1600 + 2 * wc.RED_ZONE and h.whole.dtype == torch.uint8
        assert h.tensor.data_ptr() == filled.data_ptr() == h.whole.data_ptr() + wc.RED_ZONE and filled.data_ptr() % 256 == 0
        assert filled.is_contiguous() and int(filled.sum()) == 25 * 25
        assert set(h.whole[:wc.RED_ZONE].cpu().tolist()) == set(h.whole[wc.RED_ZONE + 1600:].cpu().tolist()) == {zone}
    # the element pattern of a wider dtype, and the calls that keep their own fill
    outputs.begin("unit")
    wide = ops.torch.empty((7,), dtype=torch.float64, device="cuda")
    zeroed = ops.torch.zeros((2, 3), dtype=torch.int32, device="cuda")
    fives = ops.torch.full((4,), 5, dtype=torch.int64, device="cuda")
    assert wide.cpu().tolist() == [1.0] * 7 and not zeroed.any() and fives.cpu().tolist() == [5] * 4
    assert [h.call for h in outputs.handed] == ["empty", "zeros", "full"] and outputs.handed[1].whole[0].item() == 1
    assert ops.torch.empty((0, 4), device="cuda").numel() == 0 and ops.torch.empty((3,), dtype=torch.int32).device.type == "cpu"
    assert len(outputs.handed) == 3 and not outputs.finish()
    # a write in front of an output and one behind it are seen, and named
    outputs.begin("ones")
    ws.begin("zeros", {})
    ops.fill_holes(x)
    whole = outputs.handed[0].whole
    whole[wc.RED_ZONE - 3] = 0
    touched = outputs.finish()
    assert len(touched) == 1 and touched[0].startswith("fill_holes: torch.empty_like of (1, 40, 40) uint8, front red zone byte -3 ")
    whole[wc.RED_ZONE - 3] = 0xFF
    whole[wc.RED_ZONE + 1600 + 7] = 0
    touched = outputs.finish()
    assert len(touched) == 1 and "fill_holes" in touched[0] and "back red zone byte 7 " in touched[0]
