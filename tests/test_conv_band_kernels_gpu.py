"""Every row of tests/conv_band_cases.py on the device: one launch of usf_conv2d_same_band_f32 per cap of the band into a guarded
buffer (NaN samples behind the input), every element held to the fp64 statement with conv_kernel_cases.check at the module's
bound MARGIN * K32 * U * A, and
  (b) the same bits for every cap of the band (the sum order of an element does not depend on the banding),
  (c) a sample's bits do not depend on its position in the batch (rolled by one; a one-sample batch against the first sample),
  (d) on the three shapes of 256 pixels and fewer the band entry point meets the bound usf_conv2d_same_f32 / _ctx_f32 meet on the
      same inputs (whether the two agree bit for bit is printed, not asserted),
  (e) nothing written in front of or behind y, nothing left unwritten.
The reference runs in fp64 on the device, once per row."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_band_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = {c.name: c for c in T.cases()}


def _ext():
    from usflows_amd import _ext
    return _ext


def _rows_nan(t, roll=0):
    """[B, ...] -> a device buffer of B + 1 samples, the last one NaN; returns (buffer kept alive, view of the B samples)"""
    t = t.roll(roll, 0) if roll else t
    flat = torch.full((t.numel() + t[0].numel(),), float("nan"), dtype=torch.float32, device=DEV)
    flat[:t.numel()] = t.flatten().to(DEV)
    return flat, flat[:t.numel()].view(t.shape)


class Launch:
    """one row's operands on the device; ``run(band_rows)`` launches into a fresh guarded buffer and returns (rc, buffer)"""

    def __init__(self, c, d, roll=0, B=None):
        self.c = c = T.Case(c, B=B) if B is not None else c
        if B is not None:
            d = T.Case({k: (v[:B] if k in ("x", "ctx") and v is not None else v) for k, v in d.items()})
        self.d = d
        dev = lambda t: None if t is None else t.to(DEV).contiguous()
        pl, bias = T.pack(c, d.w, d.bias)
        self.planes, self.bias, self.in_mul, self.w_ctx = dev(pl), dev(bias), dev(d.in_mul), dev(d.w_ctx)
        self.keep, self.x = _rows_nan(d.x, roll)
        self.ctx = None
        if d.ctx is not None:
            self.keep_ctx, self.ctx = _rows_nan(d.ctx, roll) if c.ctx_stride else (None, dev(d.ctx[:1]))

    def on_device(self):
        dev = lambda t: None if t is None else t.to(DEV)
        return T.Case(x=self.x, w=dev(self.d.w), bias=dev(self.d.bias), in_mul=self.in_mul, ctx=dev(self.d.ctx), w_ctx=self.w_ctx)

    def _buffer(self):
        c = self.c
        buf = torch.full((c.B * c.cout * c.H * c.W + 2 * T.GUARD,), T.sentinel(), dtype=torch.float32, device=DEV)
        return buf, buf.data_ptr() + 4 * T.GUARD

    def run(self, band_rows, old=False):
        """old: the resident-sample entry points (usf_conv2d_same_f32 / _ctx_f32) on the same operands"""
        c, ext = self.c, _ext()
        lib, p = ext.load(), (lambda t: None if t is None else t.data_ptr())
        buf, y = self._buffer()
        st = ext.current_stream(torch.device(DEV))
        head = (self.x.data_ptr(), y, c.B, c.cin, c.cout, c.H, c.W, c.ks, self.planes.data_ptr(), p(self.bias), p(self.in_mul), c.in_act,
                c.in_slope, c.out_act, c.out_slope)
        if not old:
            rc = lib.usf_conv2d_same_band_f32(*head, p(self.ctx), c.get("ctx_stride", 0), p(self.w_ctx), band_rows, st)
        elif c.entry == "ctx":
            rc = lib.usf_conv2d_same_ctx_f32(*head, p(self.ctx), c.ctx_stride, p(self.w_ctx), st)
        else:
            rc = lib.usf_conv2d_same_f32(*head, None, 0, st)
        torch.cuda.synchronize()
        return rc, buf

    def y_of(self, buf):
        c = self.c
        return buf[T.GUARD:T.GUARD + c.B * c.cout * c.H * c.W].view(c.B, c.cout, c.H, c.W)


@pytest.mark.parametrize("name", list(CASES))
def test_band_kernel(name):
    c = CASES[name]
    ext = _ext()
    d = T.data(c)
    L = Launch(c, d)
    ref64, A64 = T.reference(c, L.on_device())
    first = None
    for br in c.band_rows:
        a = ext.conv2d_same_band_variant(c.B, c.cin, c.cout, c.H, c.W, c.ks, ctx=c.entry == "ctx", band_rows=br)
        assert a["served"] == 1, (name, br)
        rc, buf = L.run(br)
        assert rc == 0, (rc, ext.load().usf_last_error())
        y = L.y_of(buf)
        print(f"{name}: cap {br} band {a['band_rows']} x {a['bands']} groups {a['groups']} grid {a['grid']} "
              f"worst {T.measure(c, y, ref64, A64):.3f} U A of {T.BOUND:.1f} allowed")
        found = T.check(c, buf, ref64, A64, T.BOUND)                 # (a) and (e)
        assert found == [], (name, br, found)
        if first is None:
            first = buf
        else:
            assert torch.equal(T.bits(buf), T.bits(first)), f"{name}: cap {br} gives other bits than cap {c.band_rows[0]}"   # (b)
    y = L.y_of(first)
    br = c.band_rows[0]
    # (c) the same samples one position further; the first sample alone
    if c.B > 1:
        Lr = Launch(c, d, roll=1)
        rcr, bufr = Lr.run(br)
        assert rcr == 0 and torch.equal(T.bits(Lr.y_of(bufr).roll(-1, 0)), T.bits(y)), f"{name}: a sample's bits depend on its position"
        L1 = Launch(c, d, B=1)
        rc1, buf1 = L1.run(br)
        assert rc1 == 0 and torch.equal(T.bits(L1.y_of(buf1)), T.bits(y[:1])), f"{name}: a sample's bits depend on the batch"
    # (d) 256 pixels and fewer: the resident-sample kernels on the same inputs meet the same bound
    if c.H * c.W <= 256:
        rco, bufo = L.run(0, old=True)
        assert rco == 0 and T.check(c, bufo, ref64, A64, T.BOUND) == []
        print(f"{name}: usf_conv2d_same{'_ctx' if c.entry == 'ctx' else ''}_f32 worst {T.measure(c, L.y_of(bufo), ref64, A64):.3f} U A; "
              f"bit for bit the band kernel's: {torch.equal(T.bits(bufo), T.bits(first))}")


def test_a_refused_shape_is_answered_1_and_writes_nothing():
    c = T.Case(CASES["plain_32_32_28x28"], cin=48, cout=48)
    c.rows = c.cout_arg = 48
    L = Launch(c, T.data(c))
    rc, buf = L.run(0)
    assert rc == 1 and bool((T.bits(buf) == T.SENTINEL_BITS).all())


def test_the_binding_returns_what_the_entry_point_wrote():
    """_ext.conv2d_same_band: the wrapper networks.py calls, plain and with a context, against the raw launches above"""
    ext = _ext()
    for name in ("plain_3_17_17x17", "ctx_9_32_17x17"):
        c = CASES[name]
        L = Launch(c, T.data(c))
        rc, buf = L.run(0)
        y = ext.conv2d_same_band(L.x, L.planes, c.cout, c.ks, ctx=L.ctx, w_ctx=L.w_ctx, bias=L.bias, in_mul=L.in_mul, in_act=c.in_act,
                                 in_slope=c.in_slope, out_act=c.out_act, out_slope=c.out_slope)
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(T.bits(y), T.bits(L.y_of(buf))), name
    x = torch.zeros(2, 48, 28, 28, device=DEV)
    assert ext.conv2d_same_band(x, ext.conv2d_weight_planes(torch.zeros(48, 48, 3, 3, device=DEV)), 48, 3) is None
