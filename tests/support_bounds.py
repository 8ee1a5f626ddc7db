"""What tests/support_strided.py does for the GEMMs, for the kernels that take no leading dimension (and for the attention core, which takes five):
operands as views into larger allocations and the checks that a kernel respected them.  Plain torch, any device.

Beside `make` / `Strided.problems` of support_strided (used as they are for every matrix), three pieces:
  * `make1d`: a 1-D operand (mean, rstd, lse, gamma, dgamma, dbeta, table, dtable, key_bias, rowscale ...) through the same guard-and-pattern
    mechanism -- GUARD elements in front and behind; NaN with an Inf next to the region around an input, the fixed bit pattern around an output, whose
    own region starts as NaN.  It is a Strided of one row (width n, pitch n), so `problems`, `flat` and `offset` are the ones the matrices have.
  * `snapshot` / `changed`: the integer view of every input ALLOCATION (region, padding and guards) before a call, compared bitwise after it: several
    entry points const_cast their inputs into an argument struct they share with the outputs.
  * `Workspace`: exactly `nbytes` bytes of 0xFF (a NaN in every fp32 / bf16 word a kernel might read before it wrote it) inside a larger byte allocation
    whose head and tail hold a fixed byte pattern; `problems` = head and tail bitwise unchanged.  `ptr` is 256-byte aligned.

`Arena` is the bookkeeping of one call: it hands out operands either guarded (the above) or plain (ordinary contiguous torch tensors, zero-filled
workspace, NaN-filled outputs) under the same names, takes the snapshot, and collects every finding after the call, so that one function per entry point
serves both the plain call and the guarded one whose results must be bit-identical."""
import torch

from tests import support_strided as SS

GUARD = SS.GUARD
WS_PAD = 4096                    # pattern bytes in front of and behind a workspace (a multiple of 256: the workspace itself stays 256-byte aligned)
WS_FILL = 0xA5


class Strided1d(SS.Strided):
    """a vector of n elements between `guard` elements: buf is (1, guard + n + guard), the region buf[0, guard:guard + n]"""

    def __init__(self, buf, n, guard, output):
        super().__init__(buf, 1, n, guard, 0, output)

    @property
    def vec(self):
        return self.view[0]


def make1d(n, dtype, device, *, values=None, output=False, guard=GUARD):
    """One vector as a view.  values: the (n,) content of an input.  guard elements (a multiple of 16 bytes) in front and behind."""
    assert output == (values is None) and (guard * torch.empty((), dtype=dtype).element_size()) % 16 == 0
    buf = torch.empty((1, guard + n + guard), dtype=dtype, device=device)
    if output:
        buf.view(SS._INT[dtype]).fill_(SS._fill_value(dtype, SS._INT[dtype]))
    else:
        buf.fill_(float("nan"))
        buf[0, guard - 1] = float("inf")                           # the elements a kernel reaches first when it runs one past either end
        buf[0, guard + n] = float("-inf")
    s = Strided1d(buf, n, guard, output)
    if output:
        s.view.fill_(float("nan"))
    else:
        s.view[0].copy_(values.reshape(-1))
    return s


def _ints(t):
    if t.dtype in SS._INT:
        return t.view(SS._INT[t.dtype])
    return t                                                       # integer operands (index tables, sequence offsets) compare as they are


def snapshot(inputs):
    """{name: bitwise copy of the whole allocation} of a dict of inputs (Strided, or plain tensors)"""
    return {k: _ints(v.buf if isinstance(v, SS.Strided) else v).clone() for k, v in inputs.items() if v is not None}


def changed(inputs, snap):
    """names of the inputs whose allocation differs bitwise from its snapshot, with the number of changed elements"""
    out = []
    for k, before in snap.items():
        v = inputs[k]
        now = _ints(v.buf if isinstance(v, SS.Strided) else v)
        bad = int((now != before).sum().item())
        if bad:
            out.append(f"input {k}: {bad} element(s) modified by the call")
    return out


class Workspace:
    """buf: uint8 [WS_PAD | nbytes | WS_PAD]; ptr: address of the first workspace byte; nbytes: what *_workspace(...) returned"""

    def __init__(self, nbytes, device, pad=WS_PAD):
        self.nbytes, self.pad = int(nbytes), pad
        whole = torch.empty((pad + self.nbytes + pad + 256,), dtype=torch.uint8, device=device)
        self.buf = whole[(-whole.data_ptr()) % 256:][:pad + self.nbytes + pad]      # (a host allocation is only 64-byte aligned)
        self.buf.fill_(WS_FILL)
        self.buf[pad:pad + self.nbytes] = 0xFF
        self.ptr = self.buf.data_ptr() + pad

    def flat(self):
        return self.buf

    @property
    def offset(self):
        return self.pad

    def problems(self):
        out = []
        for name, part in (("in front of", self.buf[:self.pad]), ("behind", self.buf[self.pad + self.nbytes:])):
            bad = int((part != WS_FILL).sum().item())
            if bad:
                out.append(f"stray write: {bad} byte(s) changed {name} the workspace")
        return out


class Arena:
    """Operands of ONE call of an entry point.  guarded=False: ordinary contiguous tensors (the plain call).  guarded=True: every operand a view
    (support_strided.make / make1d), the workspace a Workspace.  short=True: `workspace` states one byte less than it was asked for."""

    def __init__(self, device, guarded, short=False):
        self.device, self.guarded, self.short = device, guarded, short
        self.inputs, self.outputs, self.ws, self.snap = {}, {}, [], None

    # ---- inputs
    def mat_in(self, name, values, ld=None, col=0):
        """(address, row pitch) of a 2-D input with these values; the pitch is `ld` when guarded and given, the width otherwise"""
        if values is None:
            return None, 0
        rows, width = values.shape
        if self.guarded:
            s = SS.make(rows, width, values.dtype, self.device, ld=ld, col=col, values=values)
            self.inputs[name] = s
            return s.ptr, s.ld
        t = values.contiguous().clone()
        self.inputs[name] = t
        return t.data_ptr(), width

    def vec_in(self, name, values):
        if values is None:
            return None
        if self.guarded and values.dtype in SS._INT:
            s = make1d(values.numel(), values.dtype, self.device, values=values)
            self.inputs[name] = s
            return s.ptr
        t = values.contiguous().clone()                            # (an integer vector has no NaN to be surrounded with: plain in both modes, still snapshotted)
        self.inputs[name] = t
        return t.data_ptr()

    # ---- outputs
    def mat_out(self, name, rows, width, dtype, ld=None, col=0, present=True):
        if not present:
            return None, 0
        if self.guarded:
            s = SS.make(rows, width, dtype, self.device, ld=ld, col=col, output=True)
            self.outputs[name] = s
            return s.ptr, s.ld
        t = torch.full((rows, width), float("nan"), dtype=dtype, device=self.device)
        self.outputs[name] = t
        return t.data_ptr(), width

    def vec_out(self, name, n, dtype=torch.float32, present=True):
        if not present:
            return None
        if self.guarded:
            s = make1d(n, dtype, self.device, output=True)
            self.outputs[name] = s
            return s.ptr
        t = torch.full((n,), float("nan"), dtype=dtype, device=self.device)
        self.outputs[name] = t
        return t.data_ptr()

    def workspace(self, nbytes):
        """(address, the size to state to the entry point)"""
        nbytes = int(nbytes)
        if self.guarded:
            w = Workspace(nbytes, self.device)
            self.ws.append(w)
            return w.ptr, nbytes - (1 if self.short else 0)
        t = torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=self.device)
        self.ws.append(t)
        return t.data_ptr(), nbytes - (1 if self.short else 0)

    # ---- the call
    def launch(self, fn, *args):
        """snapshot the inputs, call, wait; returns the entry point's return code"""
        self.snap = snapshot(self.inputs)
        rc = fn(*args)
        if torch.device(self.device).type == "cuda":
            torch.cuda.synchronize()
        return rc

    def result(self, name):
        """the region of an output as a tensor: (rows, width), or (n,) for a vector"""
        o = self.outputs[name]
        if isinstance(o, Strided1d):
            return o.vec
        return o.view if isinstance(o, SS.Strided) else o

    def problems(self, unwritten_ok=()):
        """every finding of the guarded call: stray writes around outputs and workspaces, non-finite output regions, modified inputs.
        unwritten_ok: names of outputs whose region the entry point documents as partly unwritten (they are only held to "no stray write")."""
        out = []
        for k, o in self.outputs.items():
            if isinstance(o, SS.Strided):
                out += [f"{k}: {s}" for s in o.problems() if not (k in unwritten_ok and "not finite" in s)]
            elif k not in unwritten_ok and not bool(torch.isfinite(o).all()):
                out.append(f"{k}: non-finite elements in the plain call's result")
        for w in self.ws:
            if isinstance(w, Workspace):
                out += w.problems()
        out += changed(self.inputs, self.snap or {})
        return out


def rowscale_values(n, gen, device):
    """a DropPath-like row scale of n entries in [0.5, 1.5) with one dropped sample: entry 1, or the only entry"""
    v = torch.rand(n, generator=gen, device=device) + 0.5
    v[0 if n == 1 else 1] = 0.0
    return v


def bits(t):
    """integer view of a (possibly non-contiguous) float tensor, for bitwise comparison"""
    return t.contiguous().view(SS._INT[t.dtype])
