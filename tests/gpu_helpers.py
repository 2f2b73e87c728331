"""Device-buffer helpers shared by the kernel-by-kernel GPU tests (tests/test_gpu_glue.py,
tests/test_gpu_magic_kernels.py, tests/test_gpu_mistral_kernels.py,
tests/test_gpu_encoder_kernels.py)."""
import torch


class Out:
    """A device output of ``shape`` filled with ``sentinel``, with one guard row behind it."""

    def __init__(self, dev, shape, dtype, sentinel, init=None):
        self.n = 1
        for s in shape:
            self.n *= s
        row = max(self.n // max(shape[0], 1), 1)
        self.sentinel = sentinel
        self.buf = torch.full((self.n + row,), sentinel, dtype=dtype, device=dev)
        self.t = self.buf[:self.n].view(*shape)
        if init is not None:
            self.t.copy_(init)

    def cpu(self):
        assert bool((self.buf[self.n:] == self.sentinel).all()), "guard row overwritten"
        return self.t.cpu()


def offset(t, dev):
    """``t`` on the device, one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=dev)
    v = buf[1:].view(*t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v
