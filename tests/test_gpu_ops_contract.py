"""The argument checks of ``ops`` on the device: the table of tests/ops_contract_cases.py with real device tensors and the
device predicate as it is -- here a foreign tensor is a CPU tensor.  As in the CPU run, ``ops._call`` and ``ops._workspace``
raise ``Reached`` in the place of every library call: no refusal case is ever run against the library (several of them would
have read out of bounds before the wrappers compared their arguments)."""
import pytest

import ops_contract_cases as cc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture
def backend(monkeypatch):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")
    from particle_col_image_segmentation_amd import ops
    cc.install(ops, monkeypatch)
    return cc.Backend(ops, "cuda", "cpu")


@pytest.mark.parametrize("e", [pytest.param(e, id=i) for i, e in cc.valid_params()])
def test_the_valid_call_reaches_the_library_and_every_mutated_one_is_refused(backend, e):
    """one test per entry (a thousand tiny device tests would cost the suite a test's overhead each): every failure is listed"""
    with pytest.raises(cc.Reached):
        cc.invoke(e, backend.ops, cc.arguments(e, backend))
    wrong = []
    for m in cc.mutations(e):
        try:
            cc.invoke(e, backend.ops, cc.arguments(e, backend, m))
        except cc.Reached as reached:
            wrong.append("%s as %s reached pcseg_%s" % (m.arg, m.kind, reached.entry))
        except (TypeError, ValueError) as err:
            if type(err) is not m.raises:
                wrong.append("%s as %s raised %r, expected %s" % (m.arg, m.kind, err, m.raises.__name__))
        else:
            wrong.append("%s as %s returned" % (m.arg, m.kind))
    assert not wrong, "%s: %s" % (e.fn, wrong)
