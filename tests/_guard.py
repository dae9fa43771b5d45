"""Guarded outputs for the per-element kernel tests (tests/test_gpu_dw_elementwise.py,
tests/test_gpu_pw_elementwise.py, tests/test_gpu_conv_elementwise.py, tests/test_gpu_bn_elementwise.py): a
16-byte-aligned slice of a larger allocation pre-filled with a NaN bit pattern.  The 64-element margins before and
after must stay bitwise untouched (a 16-byte store past a ragged row) and no output element may remain NaN (an
element never written)."""
import numpy as np
import torch

MARGIN = 64
NAN_BITS = {torch.float32: (torch.int32, 0x7FC0DEAD), torch.bfloat16: (torch.int16, 0x7FC1)}


class Guarded:
    """An output of `shape` (NHWC or flat) inside a NaN-filled allocation with sentinel margins."""

    def __init__(self, shape, dtype):
        self.shape, self.n = shape, int(np.prod(shape))
        self.itype, self.bits = NAN_BITS[dtype]
        self.buf = torch.empty(self.n + 2 * MARGIN, dtype=dtype, device="cuda")
        self.buf.view(self.itype).fill_(self.bits)
        self.ptr = self.buf.data_ptr() + MARGIN * self.buf.element_size()
        assert self.ptr % 16 == 0

    def result(self):
        """The output as fp64 on the host, after the margin and NaN checks."""
        torch.cuda.synchronize()
        ints = self.buf.view(self.itype).cpu()
        assert bool((ints[:MARGIN] == self.bits).all()), "store before the output"
        assert bool((ints[MARGIN + self.n:] == self.bits).all()), "store past the output"
        out = self.buf[MARGIN:MARGIN + self.n].double().cpu().numpy().reshape(self.shape)
        assert not np.isnan(out).any(), "{} elements never written".format(int(np.isnan(out).sum()))
        return out
