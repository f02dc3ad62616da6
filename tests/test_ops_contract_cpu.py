"""The argument checks of ``ops``, run without a GPU: the table of tests/ops_contract_cases.py on CPU tensors.

``ops._on_device`` -- the one predicate every wrapper's first check goes through -- is replaced by "a torch tensor on the CPU"
(a foreign tensor is one on the ``meta`` device), and ``ops._call`` / ``ops._workspace`` by the hook that raises ``Reached`` in
the place of a library call.  Every valid call must reach the hook; every mutated call must be refused, with the error the
table names, before it.  Nothing here loads the library."""
import pytest

import ops_contract_cases as cc

torch = pytest.importorskip("torch")


@pytest.fixture
def backend(monkeypatch):
    from particle_col_image_segmentation_amd import ops
    cc.install(ops, monkeypatch)
    monkeypatch.setattr(ops, "_on_device", lambda t: isinstance(t, torch.Tensor) and t.device.type == "cpu")
    return cc.Backend(ops, "cpu", "meta")


def test_every_public_function_is_in_the_table_or_listed_with_a_reason():
    from particle_col_image_segmentation_amd import ops
    public = cc.public_functions(ops)
    table = {e.fn for e in cc.ENTRIES}
    listed = set(cc.HOST_ONLY) | set(cc.COMPOSED)
    assert len(public) > 70 and "border_block" in public and "watershed" in public and "Points" not in public
    assert not table & listed and not set(cc.HOST_ONLY) & set(cc.COMPOSED)
    assert sorted(table | listed) == public, (sorted(set(public) - table - listed), sorted((table | listed) - set(public)))
    assert all(len(reason) > 10 for reason in list(cc.HOST_ONLY.values()) + list(cc.COMPOSED.values()))
    assert len({e.name for e in cc.ENTRIES}) == len(cc.ENTRIES)


@pytest.mark.parametrize("e", [pytest.param(e, id=i) for i, e in cc.valid_params()])
def test_every_tensor_parameter_has_its_mutations(backend, e):
    kw = cc.arguments(e, backend)
    tensors = {k for k, v in kw.items() if isinstance(v, torch.Tensor)}
    assert tensors == set(e.args) and tensors, "the table does not state the tensor arguments %s" % sorted(tensors ^ set(e.args))
    assert set(e.inout) <= tensors and set(e.accepts) <= tensors and set(e.accepts_rank) <= tensors
    muts = cc.mutations(e)
    assert len({(m.arg, m.kind) for m in muts}) == len(muts)
    for name in tensors:
        kinds = [m.kind for m in muts if m.arg == name]
        ranks = e.accepts_rank.get(name, ())
        assert "foreign" in kinds and "numpy" in kinds and any(k.startswith("dtype:") for k in kinds), (name, kinds)
        assert "rank+" in kinds or len(e.args[name].shape) + 1 in ranks, (name, kinds)
        assert "rank-" in kinds or len(e.args[name].shape) - 1 in ranks, (name, kinds)
        if name in e.inout:
            assert "strided" in kinds
    # every argument with a frame axis is tied to the other arguments through it (or is the only one that has it)
    with_b = [n for n in tensors if "B" in e.args[n].shape]
    if len(with_b) >= 2 or "B" in e.bound:
        for n in with_b:
            assert "axis%d" % e.args[n].shape.index("B") in [m.kind for m in muts if m.arg == n]


@pytest.mark.parametrize("e", [pytest.param(e, id=i) for i, e in cc.valid_params()])
def test_the_valid_call_reaches_the_library(backend, e):
    with pytest.raises(cc.Reached):
        cc.invoke(e, backend.ops, cc.arguments(e, backend))


@pytest.mark.parametrize("e,m", [pytest.param(e, m, id=i) for i, e, m in cc.mutation_params()])
def test_a_mutated_call_is_refused_before_the_library(backend, e, m):
    kw = cc.arguments(e, backend, m)
    try:
        cc.invoke(e, backend.ops, kw)
    except cc.Reached as reached:
        pytest.fail("%s with %s as %s reached pcseg_%s: expected %s" % (e.fn, m.arg, m.kind, reached.entry, m.raises.__name__))
    except (TypeError, ValueError) as err:
        assert type(err) is m.raises, "%s with %s as %s raised %r: expected %s" % (e.fn, m.arg, m.kind, err, m.raises.__name__)
    else:
        pytest.fail("%s with %s as %s returned" % (e.fn, m.arg, m.kind))


def test_the_hook_stands_in_front_of_both_ways_into_the_library(backend):
    """what the two tests above rest on: a wrapper without workspace, one whose workspace _call makes and one that asks for it
    itself all end in ``Reached``, with the entry's name"""
    ops = backend.ops
    for fn, kw, entry in ((ops.median5, dict(x=backend.tensor(torch.uint8, (1, 4, 4))), "median5_u8"),
                          (ops.fill_holes, dict(mask=backend.tensor(torch.uint8, (1, 4, 4))), "fill_holes"),
                          (ops.label_contingency, dict(labels_t=backend.tensor(torch.int32, (1, 4, 4)),
                                                       labels_s=backend.tensor(torch.int32, (1, 4, 4)), cap_t=2, cap_s=2), "label_contingency")):
        with pytest.raises(cc.Reached) as info:
            fn(**kw)
        assert info.value.entry == entry
