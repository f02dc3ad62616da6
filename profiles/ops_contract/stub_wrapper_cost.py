"""Host-only: what the argument checks of a wrapper cost per call -- no GPU, no kernel.
``python profiles/ops_contract/stub_wrapper_cost.py PACKAGE_ROOT`` (the tree whose ``ops`` is timed: this one, or the parent's
from ``git archive``) builds the stub library of profiles/ops_call/stub_cost.py -- every name of ``_lib.SIGNATURES`` exported as
a function that returns 0, a size query 256 --, loads it in the place of libpcseg.so, gives torch a current stream of 0, and
times whole wrappers on CPU tensors that answer ``is_cuda`` with True (a tensor subclass with torch's dispatch overhead
switched off: it behaves, and costs, like a plain tensor): ``median5`` (one ``_req``), ``watershed`` and ``region_reduce`` with a
class map and planes (the two wrappers that gained the most checks).  What is timed is the checks, the output allocations
(CPU ``torch.empty``) and the marshalling; the stub returns at once.  Prints one JSON line, us per call, the best of 15 repeats
of 20 000 calls; pin the process to one core (``taskset -c N``).  Needs ``cc``."""
import json
import os
import subprocess
import sys
import tempfile
import time
import types

ROOT = os.path.abspath(sys.argv[1])
sys.path.insert(0, ROOT)


def best_us(fn, n=20000, repeats=15):
    for _ in range(1000):
        fn()
    best = None
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return round(best * 1e6 / n, 3)


def main():
    import torch
    from particle_col_image_segmentation_amd import _lib
    with tempfile.TemporaryDirectory() as tmp:
        src, so = os.path.join(tmp, "stub.c"), os.path.join(tmp, "libstub.so")
        with open(src, "w") as f:
            for name in _lib.SIGNATURES:
                f.write("unsigned long %s() { return %d; }\n" % (name, 256 if name.endswith("_workspace_bytes") else 0))
        subprocess.run(["cc", "-O2", "-shared", "-fPIC", "-o", so, src], check=True)
        os.environ["PCSEG_LIB"] = so
        _lib.load()
    from particle_col_image_segmentation_amd import ops
    assert os.path.abspath(ops.__file__).startswith(ROOT + os.sep), ops.__file__
    torch.cuda.current_stream = lambda: types.SimpleNamespace(cuda_stream=0)

    class OnDevice(torch.Tensor):
        __torch_function__ = torch._C._disabled_torch_function_impl
        is_cuda = property(lambda self: True)

    def dev(t):
        return t.as_subclass(OnDevice)

    B, C, H, W = 1, 5, 8, 8
    mask = dev(torch.zeros((B, H, W), dtype=torch.uint8))
    img = dev(torch.zeros((B, H, W), dtype=torch.float32))
    labels = dev(torch.zeros((B, H, W), dtype=torch.int32))
    counts = dev(torch.zeros((B,), dtype=torch.int32))
    planes = dev(torch.zeros((B, C, H, W), dtype=torch.float32))
    print(json.dumps({"root": ROOT,
                      "median5": best_us(lambda: ops.median5(mask)),
                      "watershed": best_us(lambda: ops.watershed(img, labels, mask, mode=2)),
                      "region_reduce": best_us(lambda: ops.region_reduce(labels, counts, mask, planes, cap=40))}))


if __name__ == "__main__":
    main()
