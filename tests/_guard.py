"""Guarded outputs for the per-element kernel tests (tests/test_gpu_dw_elementwise.py,
tests/test_gpu_pw_elementwise.py, tests/test_gpu_conv_elementwise.py, tests/test_gpu_conv_bf16_elementwise.py,
tests/test_gpu_bn_elementwise.py, tests/test_gpu_head_elementwise.py): a 16-byte-aligned slice of a larger allocation pre-filled with a NaN bit pattern.
The 64-element margins before and after must stay bitwise untouched (a 16-byte store past a ragged row) and no output
element may remain NaN (an element never written).

uint8 outputs (ReLU masks) are filled with 0xA5, which no mask byte is: a byte still 0xA5 was never written.
`offset` (elements) places the output that far past the aligned position -- a misaligned output; the elements in
between belong to the leading margin."""
import numpy as np
import torch

MARGIN = 64
BYTE_FILL = 0xA5
NAN_BITS = {torch.float32: (torch.int32, 0x7FC0DEAD), torch.bfloat16: (torch.int16, 0x7FC1),
            torch.uint8: (torch.uint8, BYTE_FILL)}


class Guarded:
    """An output of `shape` (NHWC or flat) inside a NaN-filled allocation with sentinel margins."""

    def __init__(self, shape, dtype, offset=0):
        self.shape, self.n = shape, int(np.prod(shape))
        self.dtype, self.lead = dtype, MARGIN + offset
        self.itype, self.bits = NAN_BITS[dtype]
        self.buf = torch.empty(self.n + 2 * MARGIN + offset, dtype=dtype, device="cuda")
        self.buf.view(self.itype).fill_(self.bits)
        self.ptr = self.buf.data_ptr() + self.lead * self.buf.element_size()
        assert (self.ptr - offset * self.buf.element_size()) % 16 == 0

    def _ints(self):
        torch.cuda.synchronize()
        ints = self.buf.view(self.itype).cpu()
        assert bool((ints[:self.lead] == self.bits).all()), "store before the output"
        assert bool((ints[self.lead + self.n:] == self.bits).all()), "store past the output"
        return ints[self.lead:self.lead + self.n]

    def result(self):
        """The output as fp64 on the host, after the margin and NaN checks."""
        self._ints()
        out = self.buf[self.lead:self.lead + self.n].double().cpu().numpy().reshape(self.shape)
        if self.dtype == torch.uint8:
            assert not (out == BYTE_FILL).any(), "{} bytes never written".format(int((out == BYTE_FILL).sum()))
        else:
            assert not np.isnan(out).any(), "{} elements never written".format(int(np.isnan(out).sum()))
        return out

    def raw(self):
        """The output in its own type on the host (fp32, uint8, or the bf16 bit patterns as int16), after the margin
        checks and the never-written check of result()."""
        ints = self._ints().numpy().reshape(self.shape)
        assert not (ints == self.bits).any(), "{} elements never written".format(int((ints == self.bits).sum()))
        if self.dtype == torch.float32:
            return ints.view(np.float32)
        return ints

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf.view(self.itype) == self.bits).all())
