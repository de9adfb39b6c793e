"""Every row of tests/conv_kernel_cases.py launched once on the device and held to the fp64 statement on EVERY element:
the probe's answer for this device, guards around y and NaN samples behind every input, the per-element bound
MARGIN * K32 * U * A next to the suite's max-norm bound, bit-reproducibility, and sample independence (rolled by one
position; batch (a) against batch (b)).  The reference runs in fp64 on the device (the same torch statement the CPU file holds
the fp32 statement to)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_kernel_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = {c.name: c for c in K.cases()}


def _ext():
    from usflows_amd import _ext
    return _ext


def knobs(kv):
    """conv_kernel_cases.knobs on the loaded library"""
    return K.knobs(_ext().load(), kv)


def _rows_nan(t, roll=0, lead=0):
    """[B, ...] -> a device buffer of B + 1 samples, the last one NaN (``lead`` floats in front: the view starts off a 16-byte
    boundary); returns (buffer kept alive, view of the B samples)"""
    t = t.roll(roll, 0) if roll else t
    flat = torch.full((lead + t.numel() + t[0].numel(),), float("nan"), dtype=torch.float32, device=DEV)
    flat[lead:lead + t.numel()] = t.flatten().to(DEV)
    return flat, flat[lead:lead + t.numel()].view(t.shape)


class Launch:
    """one case's operands on the device; ``run`` launches into a fresh guarded buffer and returns (rc, buffer)"""

    def __init__(self, c, d, roll=0, B=None):
        self.c = c = K.Case(c, B=B) if B is not None else c
        if B is not None:
            d = K.Case({k: (v[:B] if k in ("x", "ctx", "res_x", "gate_h", "gate_add", "gate_x") and v is not None else v) for k, v in d.items()})
        self.d, self.keep = d, []
        dev = lambda t: None if t is None else t.to(DEV).contiguous()
        rows = lambda t, lead=0: None if t is None else self._keep(_rows_nan(t, roll, lead))
        pl, bias = K.planes(c, d.w, d.bias)
        self.planes, self.bias, self.in_mul = dev(pl), dev(bias), dev(d.in_mul)
        self.x = rows(d.x, 1 if c.xoff else 0)
        self.ctx = rows(d.ctx) if (d.ctx is not None and c.ctx_stride) else dev(d.ctx[:1] if d.ctx is not None else None)
        self.w_ctx, self.res_mul, self.gate_mul = dev(d.w_ctx), dev(d.res_mul), dev(d.gate_mul)
        self.res_x, self.gate_h, self.gate_add, self.gate_x = rows(d.res_x), rows(d.gate_h), rows(d.gate_add), rows(d.gate_x)

    def _keep(self, pair):
        self.keep.append(pair[0])
        return pair[1]

    def on_device(self):
        """the operands as the statements of conv_kernel_cases read them"""
        dev = lambda t: None if t is None else t.to(DEV)
        return K.Case(x=self.x, w=dev(self.d.w), bias=dev(self.d.bias), in_mul=self.in_mul, ctx=dev(self.d.ctx), w_ctx=self.w_ctx,
                      res_x=self.res_x, res_mul=self.res_mul, gate_h=self.gate_h, gate_mul=self.gate_mul, gate_add=self.gate_add,
                      gate_x=self.gate_x)

    def run(self):
        c, ext = self.c, _ext()
        lib, p = ext.load(), (lambda t: None if t is None else t.data_ptr())
        n = c.B * c.cout * c.H * c.W
        lead = 1 if c.yoff else 0
        full = torch.full((lead + n + 2 * K.GUARD,), K.sentinel(), dtype=torch.float32, device=DEV)
        buf = full[lead:]
        y = buf.data_ptr() + 4 * K.GUARD
        assert (self.x.data_ptr() % 16 != 0) == c.xoff and (y % 16 != 0) == c.yoff
        st = ext.current_stream(torch.device(DEV))
        head = (self.x.data_ptr(), y, c.B, c.cin, c.cout_arg, c.H, c.W, c.ks, self.planes.data_ptr())
        with knobs(c.knobs):
            if c.entry in ("plain", "gated"):
                rc = lib.usf_conv2d_same_f32(*head, p(self.bias), p(self.in_mul), c.in_act, c.in_slope, c.get("out_act", 0), c.get("out_slope", 0.0),
                                             p(self.gate_x), c.C, st)
            elif c.entry == "ctx":
                rc = lib.usf_conv2d_same_ctx_f32(*head, p(self.bias), p(self.in_mul), c.in_act, c.in_slope, c.out_act, c.out_slope,
                                                 p(self.ctx), c.ctx_stride, p(self.w_ctx), st)
            elif c.entry == "res":
                rc = lib.usf_conv2d_same_res_f32(*head, p(self.bias), p(self.in_mul), c.in_act, c.in_slope, p(self.res_x), p(self.res_mul),
                                                 c.res_sign, st)
            else:
                rc = lib.usf_conv2d_same_gate_f32(*head, p(self.gate_h), c.gate_slope, p(self.gate_mul), p(self.gate_add), st)
        torch.cuda.synchronize()
        return rc, buf

    def y_of(self, buf):
        c = self.c
        return buf[K.GUARD:K.GUARD + c.B * c.cout * c.H * c.W].view(c.B, c.cout, c.H, c.W)


def _variant(c):
    ext = _ext()
    with knobs(c.knobs):
        a = ext.conv2d_same_variant(c.entry, c.B, c.cin, c.cout_arg, c.H, c.W, c.ks, not (c.xoff or c.yoff), 0)
    return a, ((a["kernel"], a["S"], a["NB"], a["CP"], a["NCT"], a["CTX"]) if a["kernel"] else (0,) * 6)


def _hold(name):
    c = CASES[name]
    a, got = _variant(c)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert got == c.expect, f"{name}: the probe answers {got} on this device ({cus} compute units), the table expects {c.expect} at 256"
    d = K.data(c)
    L = Launch(c, d)
    rc, buf = L.run()
    if c.expect[0] == 0:
        # refused: the fused forms answer 1 (the caller runs two passes), plain / ctx calls with no kernel answer -3; nothing is written
        assert rc == (1 if c.entry in ("res", "gate_mul", "gate_add") else -3), rc
        assert bool((K.bits(buf) == K.SENTINEL_BITS).all())
        return
    assert rc == 0, (rc, _ext().load().usf_last_error())
    ref64, A64 = K.reference(c, L.on_device())
    found = K.check(c, buf, ref64, A64)
    print(f"{name}: kernel {a['kernel']} S {a['S']} worst {K.measure(c, L.y_of(buf), ref64, A64):.3f} U A of {K.MARGIN * K.K32} allowed")
    assert found == [], (name, found)
    y = L.y_of(buf)
    # (d) two launches, the same bits
    rc2, buf2 = L.run()
    assert rc2 == 0 and torch.equal(K.bits(buf2), K.bits(buf)), f"{name}: a second launch gives other bits"
    # (e) sample independence: the same samples one position further
    if c.B > 1:
        Lr = Launch(c, d, roll=1)
        rcr, bufr = Lr.run()
        assert rcr == 0 and torch.equal(K.bits(Lr.y_of(bufr).roll(-1, 0)), K.bits(y)), f"{name}: a sample's bits depend on its position"
    # ... and batch (a) inside batch (b): the same kernel at another S
    if name.endswith("_b") and name[:-1] + "a" in CASES:
        ca = CASES[name[:-1] + "a"]
        assert K.family(ca) == K.family(c)
        La = Launch(c, d, B=ca.B)
        rca, bufa = La.run()
        assert rca == 0 and torch.equal(K.bits(La.y_of(bufa)), K.bits(y[:ca.B])), f"{name}: batch (a)'s bits differ from batch (b)'s"


def _names(pred):
    return [n for n, c in CASES.items() if pred(c)]


@pytest.mark.parametrize("name", _names(lambda c: c.expect[0] == 3))
def test_wave_specialised_kernel(name):
    _hold(name)


@pytest.mark.parametrize("name", _names(lambda c: c.knobs == {"conv_wsp": 0}))
def test_register_weight_kernel(name):
    """conv_wsp=0: all 12 instantiations, the forms it accepts and the two it refuses"""
    _hold(name)


@pytest.mark.parametrize("name", _names(lambda c: c.expect[0] in (0, 1) and c.knobs != {"conv_wsp": 0}))
def test_first_kernel(name):
    _hold(name)


def test_every_case_is_launched():
    ran = set(_names(lambda c: c.expect[0] == 3)) | set(_names(lambda c: c.knobs == {"conv_wsp": 0})) | \
        set(_names(lambda c: c.expect[0] in (0, 1) and c.knobs != {"conv_wsp": 0}))
    assert ran == set(CASES)


def test_ctx_entry_without_context_is_the_plain_entry():
    """the header: ctx == NULL is exactly usf_conv2d_same_f32 -- on each of the three kernels"""
    for name in ("wsp_16_32_7x7_a", "wreg_16_32_7x7_a", "first_5_5_6x6"):
        c = CASES[name]
        L = Launch(c, K.data(c))
        rc, buf = L.run()
        Lc = Launch(K.Case(c, entry="ctx", ctx_stride=0), K.data(c))
        Lc.ctx = Lc.w_ctx = None
        rcc, bufc = Lc.run()
        assert rc == 0 and rcc == 0 and torch.equal(K.bits(buf), K.bits(bufc)), name


def test_device_weight_planes_are_the_builders():
    """usf_conv2d_weight_planes_f32 against the planes built on the CPU from the header's layout text: the same bits"""
    ext = _ext()
    seen = set()
    for c in CASES.values():
        key = (c.cin, c.cout, c.ks)
        if c.entry == "gated" or key in seen:
            continue
        seen.add(key)
        d = K.data(c)
        want, _ = K.planes(c, d.w, d.bias)
        got = ext.conv2d_weight_planes(d.w.to(DEV))
        torch.cuda.synchronize()
        assert got.shape == want.shape and torch.equal(got.cpu().view(torch.int16), want.view(torch.int16)), key
    assert len(seen) >= 20
