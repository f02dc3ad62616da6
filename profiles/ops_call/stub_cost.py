"""Host-only cross-check of what ``ops._call`` costs per call: no GPU, no kernel.
``python profiles/ops_call/stub_cost.py`` builds a stub library that exports every name of ``_lib.SIGNATURES`` as a function
returning 0 (a size query: 256), loads it in the place of libpcseg.so (PCSEG_LIB), gives torch a current stream of 0, and
times on CPU tensors the spelled-out form of a call -- ``_lib.check(lib.pcseg_X(_ptr(..), .., _stream()), name)``, the form every
wrapper had -- against ``ops._call`` for one entry without workspace (``median5_u8``) and one with a handed-on workspace
(``region_shape``).  Prints one JSON line, us per call, the best of 15 repeats of 100 000 calls; pin the process to one core
(``taskset -c N``) for figures that repeat to 0.05 us.  Needs ``cc``."""
import json
import os
import subprocess
import sys
import tempfile
import time
import types

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)


def best_us(fn, n=100000, repeats=15):
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
        lib = _lib.load()
    from particle_col_image_segmentation_amd import ops
    torch.cuda.current_stream = lambda: types.SimpleNamespace(cuda_stream=0)
    x = torch.zeros((1, 64, 64), dtype=torch.uint8)
    out, counts = torch.empty_like(x), torch.zeros((1,), dtype=torch.int32)
    ws = (torch.empty(256, dtype=torch.uint8), 256)
    B, H, W = x.shape
    _ptr, _stream = ops._ptr, ops._stream

    def spelled_median5():
        lib = _lib.load()
        _lib.check(lib.pcseg_median5_u8(_ptr(x), _ptr(out), B, H, W, _stream()), "median5")

    def spelled_region_shape():
        lib = _lib.load()
        _lib.check(lib.pcseg_region_shape(_ptr(x), _ptr(counts), _ptr(out), _ptr(counts), B, H, W, 7, _ptr(ws[0]), ws[1], _stream()),
                   "region_shape")

    def call_median5():
        ops._call("median5_u8", x, out, B, H, W)

    def call_region_shape():
        ops._call("region_shape", x, counts, out, counts, B, H, W, 7, ws=ws)

    print(json.dumps({"median5_u8": {"spelled_out": best_us(spelled_median5), "_call": best_us(call_median5)},
                      "region_shape": {"spelled_out": best_us(spelled_region_shape), "_call": best_us(call_region_shape)}}))


if __name__ == "__main__":
    main()
