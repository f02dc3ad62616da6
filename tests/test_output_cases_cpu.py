"""The CPU half of the output-state test (tests/output_cases.py, device_helpers.OutputHooks): every compute entry of the library
is declared by a case or exempt with a reason, the new builders are deterministic, the prior states are what they say, and the
proxy forwards what it does not override.  No GPU needed."""
import numpy as np
import pytest

import output_cases as oc
import workspace_cases as wc
from particle_col_image_segmentation_amd import _lib

torch = pytest.importorskip("torch")


def test_every_entry_is_declared_by_a_case_or_exempt_with_a_reason():
    """a new entry in _lib.SIGNATURES fails here until a case drives it"""
    declared = set()
    for case in oc.CASES:
        declared |= set(case.entries)
    exempt = {name for name in _lib.SIGNATURES if oc.exempt(name)}
    assert all(isinstance(oc.exempt(name), str) and oc.exempt(name) for name in exempt)
    assert set(oc.EXEMPT) <= set(_lib.SIGNATURES) and not declared & exempt
    assert declared == set(_lib.SIGNATURES) - exempt, sorted(declared ^ (set(_lib.SIGNATURES) - exempt))
    assert {n for n in exempt if not n.endswith("_workspace_bytes")} == {
        "pcseg_version", "pcseg_last_error", "pcseg_device_count", "pcseg_timing_enable", "pcseg_timing_report",
        "pcseg_watershed_counters", "pcseg_mixing_tile", "pcseg_surface_thresholds", "pcseg_border_block"}


def test_the_workspace_cases_are_all_here_with_what_they_declared():
    names = [case.name for case in oc.CASES]
    assert len(names) == len(set(names))
    by_name = {case.name: case for case in oc.CASES}
    for case in wc.CASES:
        mine = by_name[case.name]
        assert set(case.entries) <= set(mine.entries) and mine[2:] == case[2:], case.name
        assert set(mine.entries) - set(case.entries) == {"pcseg_" + e for e in oc.ALSO_DRIVEN.get(case.name, ())}
        assert not (set(mine.entries) - set(case.entries)) & (set(_lib.WORKSPACE) | set(_lib.WORKSPACE_HANDED_ON)), case.name
    assert set(oc.ALSO_DRIVEN) <= set(by_name) and set(oc.PROMISES) <= {case.name for case in oc.NEW_CASES}
    for case in oc.NEW_CASES:
        assert case.entries and callable(case.build) and callable(case.run) and callable(case.check), case.name
        assert case.shapes in ((wc.PRIMARY, wc.SECOND), oc.SUMS2_SHAPES), case.name


def test_the_plane_sum_shapes_reach_both_routes():
    assert wc.PRIMARY[2] % 4 and wc.SECOND[2] % 4 == 0                      # the row sums kernel and the fused column kernel
    assert all(s[2] % 4 == 0 for s in oc.SUMS2_SHAPES) and oc.SUMS2_SHAPES[1][1] % 32  # region_sums2 takes W % 4 == 0 only


@pytest.mark.parametrize("case", oc.NEW_CASES, ids=lambda c: c.name)
def test_new_builders_are_deterministic(case):
    for shape in case.shapes:
        a, b, c = case.build(shape, 3), case.build(shape, 3), case.build(shape, 4)
        assert sorted(a) == sorted(b)
        differs = False
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (case.name, k)
            differs = differs or a[k].tobytes() != c[k].tobytes()
        assert differs, "%s: another seed gives the same data" % case.name


def test_plane_sum_inputs_overflow_one_table_and_not_the_other():
    for shape in (wc.PRIMARY, wc.SECOND):
        x = oc.build_plane_sums(shape, 5)
        assert (x["counts"][:-1] > oc.CAP_LOW).all() and 0 < x["counts"][-1] < oc.CAP_LOW
        assert np.array_equal(x["planes"] * 64, np.rint(x["planes"] * 64)) and x["planes"].max() < 1  # sums exact in any order


def test_state_fills_per_dtype():
    assert oc.OUTPUT_STATES == ("zeros", "ones", "unit")
    for dtype in oc.UNIT_DTYPES:
        item = np.dtype(dtype).itemsize
        for n in (1, 7, 300):
            z, o, u = (oc.output_fill(state, dtype, n * item) for state in oc.OUTPUT_STATES)
            assert z.dtype == o.dtype == u.dtype == np.uint8 and z.shape == o.shape == u.shape == (n * item + 2 * wc.RED_ZONE,)
            body = lambda f: f[wc.RED_ZONE:wc.RED_ZONE + n * item]
            zones = lambda f: np.concatenate([f[:wc.RED_ZONE], f[wc.RED_ZONE + n * item:]])
            assert not body(z).any() and (zones(z) == 0xFF).all()             # a stray zero write shows too
            assert (o == 0xFF).all()
            assert (body(u).view(dtype) == 1).all() and (zones(u).view(dtype) == 1).all() and (u.view(dtype) == 1).all()
    assert np.isnan(oc.fill_pattern("ones", np.float64).view(np.float64)[0]) and oc.fill_pattern("ones", np.int32).view(np.int32)[0] == -1
    assert oc.fill_pattern("unit", np.float32).view(np.float32)[0] == 1.0 and oc.fill_pattern("unit", np.uint16).tolist() == [1, 0]
    assert wc.RED_ZONE == 4096
    with pytest.raises(ValueError):
        oc.fill_pattern("random", np.uint8)


def test_only_plain_cuda_allocations_are_modelled():
    from device_helpers import modelled
    i32, cuda = torch.int32, torch.device("cuda", 0)
    assert modelled("empty", ((2, 3),), {"dtype": i32, "device": "cuda"}) == ((2, 3), i32, torch.device("cuda"), None)
    assert modelled("empty", (2, 3), {"dtype": i32, "device": cuda}) == ((2, 3), i32, cuda, None)
    assert modelled("zeros", ((4,),), {"device": cuda})[1] == torch.get_default_dtype()
    assert modelled("full", ((4,), 7), {"device": cuda})[1::2] == (torch.int64, 7)
    assert modelled("full", ((4,),), {"fill_value": -1.0, "dtype": torch.float64, "device": cuda})[1::2] == (torch.float64, -1.0)
    like = torch.zeros((3, 4), dtype=torch.uint8)
    assert modelled("empty_like", (like,), {"device": cuda}) == ((3, 4), torch.uint8, cuda, None)
    assert modelled("zeros_like", (like,), {"dtype": i32, "device": cuda})[1] == i32
    # everything else is torch's own business: host and pinned memory, zero-size tensors, layouts the hooks do not model
    for call, args, kwargs in (("empty", ((2, 3),), {"dtype": i32}), ("empty", ((2, 3),), {"dtype": i32, "device": "cpu"}),
                               ("empty", ((2, 3),), {"dtype": i32, "device": cuda, "pin_memory": True}),
                               ("empty", ((0, 3),), {"dtype": i32, "device": cuda}), ("empty_like", (like,), {}),
                               ("empty_like", (like.t(),), {"device": cuda}),
                               ("empty", ((2, 3),), {"device": cuda, "memory_format": torch.contiguous_format}),
                               ("empty", ((2, 3),), {"device": cuda, "dtype": torch.float16}),
                               ("zeros", ((2, 3),), {"device": cuda, "out": like}), ("full", ((2,), like[0, 0]), {"device": cuda})):
        assert modelled(call, args, kwargs) is None, (call, kwargs)


def test_the_proxy_forwards_and_pads_only_what_it_models(monkeypatch):
    """on the host: the proxy in the place of ``ops.torch`` forwards every name, hands host allocations back as torch made
    them -- and, with the device test switched to "any device", pads, fills, names and watches an allocation as on the GPU"""
    import device_helpers as dh
    from particle_col_image_segmentation_amd import ops, pipeline
    hooks = dh.OutputHooks((ops, pipeline), monkeypatch)
    assert ops.torch is hooks.proxy is pipeline.torch and dh.torch is torch
    for name in ("Tensor", "int32", "float64", "cuda", "arange", "sort", "from_numpy", "full_like", "device"):
        assert getattr(ops.torch, name) is getattr(torch, name), name
    host = ops.torch.empty((3, 4), dtype=torch.int32)
    assert isinstance(host, torch.Tensor) and host.shape == (3, 4) and host.dtype == torch.int32 and not hooks.handed
    assert not ops.torch.zeros((2,), dtype=torch.uint8, device="cpu").any() and ops.torch.full((2,), 3).tolist() == [3, 3]
    assert ops.torch.empty_like(host).shape == (3, 4) and ops.torch.zeros_like(host).dtype == torch.int32 and not hooks.handed
    monkeypatch.setattr(dh, "_cuda", lambda device: device is not None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)

    def some_wrapper(state):
        hooks.begin(state)
        made = {name: (lambda shape, dtype: ops.torch.empty(shape, dtype=dtype, device="cpu"))(shape, dtype)  # (as ops._pair_rows does)
                for name, shape, dtype in (("u8", (5, 3), torch.uint8), ("u16", (4,), torch.uint16), ("i64", (2, 2), torch.int64),
                                           ("f64", (3,), torch.float64))}
        made["zeroed"] = ops.torch.zeros_like(made["i64"])
        return made

    made = some_wrapper("unit")
    assert made["u8"].tolist() == [[1] * 3] * 5 and made["i64"].tolist() == [[1, 1]] * 2 and made["f64"].tolist() == [1.0] * 3
    assert made["u16"].view(torch.int16).tolist() == [1] * 4 and not made["zeroed"].any()
    assert [(h.wrapper, h.call, h.shape, h.nbytes) for h in hooks.handed] == [
        ("some_wrapper", "empty", (5, 3), 15), ("some_wrapper", "empty", (4,), 8), ("some_wrapper", "empty", (2, 2), 32),
        ("some_wrapper", "empty", (3,), 24), ("some_wrapper", "zeros_like", (2, 2), 32)]
    assert all(t.is_contiguous() for t in made.values()) and not hooks.finish()
    made = some_wrapper("ones")
    assert made["u8"].tolist() == [[255] * 3] * 5 and made["i64"].tolist() == [[-1, -1]] * 2 and made["f64"].isnan().all()
    made["f64"][:] = 2.0                       # writing the output itself is no finding
    hooks.handed[3].whole[wc.RED_ZONE + 24] = 0  # ... the byte behind it is
    hooks.handed[0].whole[wc.RED_ZONE - 1] = 7   # ... and the byte in front of another
    touched = hooks.finish()
    assert touched == ["some_wrapper: torch.empty of (5, 3) uint8, front red zone byte -1 is 0x07, was 0xff",
                       "some_wrapper: torch.empty of (3,) float64, back red zone byte 0 is 0x00, was 0xff"]
    made = some_wrapper("zeros")
    assert not any(bool(t.any()) for t in made.values()) and set(hooks.handed[0].whole[:wc.RED_ZONE].tolist()) == {0xFF}


def test_not_left_sees_one_element_beyond_the_bound():
    from device_helpers import not_left
    for state in ("ones", "unit"):
        for dtype, np_dtype in ((torch.int64, np.int64), (torch.uint8, np.uint8), (torch.float64, np.float64)):
            t = torch.from_numpy(np.tile(oc.fill_pattern(state, np_dtype), 2 * 5 * 3).view(np_dtype).reshape(2, 5, 3).copy())
            defined = torch.arange(5)[None, :] < torch.tensor([2, 0])[:, None]
            t[0, :2] = 0                        # the rows a call defines may hold anything
            assert not_left(t, defined, state).shape == (0, 3)
            t[1, 4, 2] = 0                      # one element beyond the bound
            assert not_left(t, defined, state).tolist() == [[1, 4, 2]]
            t[0, 2, 0] = 7
            assert not_left(t, defined, state).tolist() == [[0, 2, 0], [1, 4, 2]]
