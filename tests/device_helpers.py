"""Device-side helpers shared by the GPU test files (no tests in here)."""
import torch


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
