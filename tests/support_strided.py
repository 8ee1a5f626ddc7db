"""Operands and outputs of a GEMM as views into larger allocations, and the check that a kernel respected them.  Plain torch, any device.

A kernel that takes a leading dimension promises three things no contiguous, fully initialised operand can test:
  * it addresses row m at m * ld, not m * width;
  * it writes nothing outside the rows x width region of an output (no rows >= M of a ragged last panel, no columns >= N);
  * whatever it reads outside the region of an input (an over-read K tail, the rows behind a ragged panel) never enters a result.

`make` builds one matrix as a view: GUARD rows in front and behind (more than the tallest tile, so every over-read the kernels make stays
inside the allocation), a row pitch ld >= width, an optional column offset (col = width, ld = 3 * width: the middle third of a packed buffer).
Everything outside the region of an INPUT is NaN, with one Inf per row, so that padding contracted into a result shows (0 x NaN is NaN where
0 x the next row's finite data was 0).  Everything outside the region of an OUTPUT is one fixed finite bit pattern and the region itself starts
as NaN.  `problems` compares the outside of an output BITWISE (integer view) with that pattern and requires the region to be finite everywhere.
"""
import torch

GUARD = 512
_INT = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}
# the output padding: a finite value no kernel here produces by accident (bf16 0x3F9D = 1.2265625; fp32 0x3F9D70A4 = 1.23; fp64 1.23)
_FILL = {torch.bfloat16: 0x3F9D, torch.float32: 0x3F9D70A4, torch.float64: 0x3FF3AE147AE147AE}


class Strided:
    """buf: the whole allocation (GUARD + rows + GUARD, ld); view: the rows x width region; ld: row pitch in elements; ptr: address of view[0, 0]"""

    def __init__(self, buf, rows, width, col, guard, output):
        self.buf, self.rows, self.width, self.col, self.guard, self.output = buf, rows, width, col, guard, output
        self.ld = buf.shape[1]
        self.view = buf[guard:guard + rows, col:col + width]
        self.ptr = self.view.data_ptr() if rows and width else buf.data_ptr()
        assert self.ptr % 16 == 0, "the base pointer of a view must stay 16-byte aligned: ld and col multiples of 16 bytes"

    @property
    def offset(self):
        """element index of view[0, 0] in buf.view(-1): what a kernel adds m * ld + n to"""
        return self.guard * self.ld + self.col

    def flat(self):
        return self.buf.view(-1)

    def _outside(self, t):
        g, r, c, w = self.guard, self.rows, self.col, self.width
        return [("guard rows in front", t[:g]), ("guard rows behind", t[g + r:]), ("columns left of the region", t[g:g + r, :c]),
                ("columns right of the region", t[g:g + r, c + w:])]

    def problems(self):
        """what the kernel did wrong to this OUTPUT, as a list of strings (empty: nothing)"""
        assert self.output
        out = []
        ints = self.buf.view(_INT[self.buf.dtype])
        fill = _fill_value(self.buf.dtype, ints.dtype)
        for name, part in self._outside(ints):
            bad = int((part != fill).sum().item()) if part.numel() else 0
            if bad:
                out.append(f"stray write: {bad} element(s) changed in the {name}")
        nonfinite = int((~torch.isfinite(self.view)).sum().item())
        if nonfinite:
            out.append(f"{nonfinite} of {self.view.numel()} elements of the valid region are not finite (unwritten, or padding entered the result)")
        return out


def _fill_value(dtype, int_dtype):
    v = _FILL[dtype]
    bits = torch.iinfo(int_dtype).bits
    return v - (1 << bits) if v >= 1 << (bits - 1) else v


def make(rows, width, dtype, device, *, ld=None, col=0, values=None, output=False, guard=GUARD):
    """One matrix as a view.  ld=None: contiguous rows (ld = width), still with guard rows.  values: the (rows, width) content of an input."""
    ld = width if ld is None else ld
    assert ld >= col + width and output == (values is None)
    buf = torch.empty((guard + rows + guard, ld), dtype=dtype, device=device)
    if output:
        buf.view(_INT[dtype]).fill_(_fill_value(dtype, _INT[dtype]))
    else:
        buf.fill_(float("nan"))
        if ld > width:                                             # one Inf per row, in the padding (alternating sign, moving column)
            r = torch.arange(buf.shape[0], device=device)
            j = r % (ld - width)                                   # the j-th padding column: left of the region, then right of it
            inf = torch.full((buf.shape[0],), float("inf"), dtype=dtype, device=device)
            inf[1::2] = float("-inf")
            buf[r, torch.where(j < col, j, j + width)] = inf
        else:
            buf[:guard, 0] = float("inf")
            buf[guard + rows:, 0] = float("-inf")
    s = Strided(buf, rows, width, col, guard, output)
    if output:
        s.view.fill_(float("nan"))
    else:
        s.view.copy_(values)
    return s
