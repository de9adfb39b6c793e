"""Every row of tests/image_grad_cases.py launched once on the device and held to the fp64 statement on EVERY element: the
probe's answer on this device, sentinels in front of and behind every output, one NaN sample behind x and dy, a workspace
full of NaN, the per-element bound MARGIN * K * U * A next to the suite's earlier max-norm bound, bit-reproducibility; refused
rows leave every sentinel; queued weight gradients (usf_conv_wgrad_plan_f32 + usf_conv_wgrad_jobs_f32 +
usf_partial_sum_jobs_f32) and the deferred form give the bits of the single calls.  The reference runs in fp64 on the device
(the same torch statements the CPU file holds the fp32 statements to)."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_grad_cases as G  # noqa: E402
from test_conv_kernels_gpu import _rows_nan  # noqa: E402  (B samples and a NaN one behind them)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WG = {c.name: c for c in G.wg_cases()}
LN = {c.name: c for c in G.ln_cases()}
GR = {c.name: c for c in G.gr_cases()}
CTX = {c.name: c for c in G.ctx_cases()}


def _ext():
    from usflows_amd import _ext
    return _ext


def _nan(n):
    return torch.full((max(int(n), 16),), float("nan"), dtype=torch.float32, device=DEV)


def _report(family, name, buf, ref, A, lo=G.GUARD):
    share = G.ratio(buf[lo:lo + ref.numel()].view(ref.shape), ref, A) / (G.MARGIN * G.K[family])
    print(f"IGK {family} {name} {share:.4f} of the bound")


class WgLaunch:
    """one weight-gradient row's operands on the device; ``run`` launches into fresh guarded buffers"""

    def __init__(self, c):
        self.c = c
        d = G.wg_data(c)
        self.keep = []
        self.x = self._rows(d.x, 1 if c.fault == "xoff" else 0)
        self.dy = self._rows(d.dy)
        self.in_mul = None if d.in_mul is None else d.in_mul.to(DEV)
        self.pre_sub = None if d.pre_sub is None else d.pre_sub.to(DEV)
        assert (self.x.data_ptr() % 16 != 0) == (c.fault == "xoff") and self.dy.data_ptr() % 16 == 0

    def _rows(self, t, lead=0):
        keep, view = _rows_nan(t, 0, lead)
        self.keep.append(keep)
        return view

    def on_device(self):
        return G.Case(x=self.x, dy=self.dy, in_mul=self.in_mul, pre_sub=self.pre_sub)

    def buffers(self):
        c = self.c
        lib = _ext().load()
        with G.knobs(lib, c.knobs):
            ws_n = lib.usf_conv_wgrad_workspace(c.B, c.cin, c.cout, c.H, c.W, c.ks)
        return G.guarded(c.cout * c.cin * c.ks * c.ks, DEV), G.guarded(c.cout, DEV), _nan(ws_n), ws_n

    def head(self, bufW, bufb, ws, ws_n):
        c, p = self.c, (lambda t: None if t is None else t.data_ptr())
        return (self.x.data_ptr(), self.dy.data_ptr(), c.B, c.cin, c.cout, c.H, c.W, c.ks, p(self.in_mul), p(self.pre_sub), c.act, c.slope,
                bufW.data_ptr() + 4 * G.GUARD, bufb.data_ptr() + 4 * G.GUARD if c.bias else None, ws.data_ptr(),
                ws_n - 1 if c.fault == "short_ws" else ws_n)

    def run(self):
        ext = _ext()
        bufW, bufb, ws, ws_n = self.buffers()
        with G.knobs(ext.load(), self.c.knobs):
            rc = ext.load().usf_conv_wgrad_f32(*self.head(bufW, bufb, ws, ws_n), ext.current_stream(torch.device(DEV)))
        torch.cuda.synchronize()
        return rc, bufW, bufb


def _hold_wg(name):
    c, ext = WG[name], _ext()
    with G.knobs(ext.load(), c.knobs):
        a = ext.conv_wgrad_variant(max(c.B, 1), c.cin, c.cout, c.H, c.W, c.ks, c.mask, 0, 0)
    # (no row's expectation depends on the device's compute units or occupancy answer -- the CPU file proves it -- so every
    # field is compared on every row, `blocks` included; the answer the device gave is printed)
    got = G.wg_expect(a) if c.B > 0 else (0,) * 10
    assert got == c.expect, f"{name}: the probe answers {got} on this device ({a['cus']} compute units, {a['blocks_per_cu']} blocks each), the table {c.expect}"
    L = WgLaunch(c)
    rc, bufW, bufb = L.run()
    if c.rc != 0:
        assert rc == c.rc, (name, rc)
        assert G.untouched(bufW) and G.untouched(bufb), f"{name}: a refused call wrote"
        return
    assert rc == 0, (rc, ext.load().usf_last_error())
    r = G.wg_forward(c, L.on_device(), torch.float64)
    found = G.check("dW", bufW, r.dW, r.A_dW, "wg_dW")
    _report("wg_dW", name, bufW, r.dW, r.A_dW)
    if c.bias:
        found += G.check("db", bufb, r.db, r.A_db, "wg_db")
        _report("wg_db", name, bufb, r.db, r.A_db)
    else:
        assert G.untouched(bufb), f"{name}: db == NULL, yet the buffer next to dW was written"
    print(f"IGP {name} kernel {a['kernel']} <{a['CIT']},{a['COT']},{a['T']}> rsplit {a['rsplit']} blocks {a['blocks']} blocks_per_cu {a['blocks_per_cu']}")
    assert found == [], (name, found)
    rc2, bufW2, bufb2 = L.run()
    assert rc2 == 0 and torch.equal(G.bits(bufW2), G.bits(bufW)) and torch.equal(G.bits(bufb2), G.bits(bufb)), f"{name}: a second launch gives other bits"


def _wg_names(pred):
    return [n for n, c in WG.items() if pred(c)]


@pytest.mark.parametrize("name", _wg_names(lambda c: c.rc == 0 and c.expect[0] == 1 and c.expect[3] == 9))
def test_conv_wgrad_kernel_3x3(name):
    _hold_wg(name)


@pytest.mark.parametrize("name", _wg_names(lambda c: c.rc == 0 and c.expect[0] == 1 and c.expect[3] == 1))
def test_conv_wgrad_kernel_1x1_staged(name):
    _hold_wg(name)


@pytest.mark.parametrize("name", _wg_names(lambda c: c.rc == 0 and c.expect[0] == 2))
def test_conv_wgrad_kernel_1x1_direct(name):
    _hold_wg(name)


@pytest.mark.parametrize("name", _wg_names(lambda c: c.rc != 0))
def test_conv_wgrad_refusals_write_nothing(name):
    _hold_wg(name)


def test_every_weight_gradient_row_is_launched():
    ran = set(_wg_names(lambda c: c.rc != 0)) | set(_wg_names(lambda c: c.rc == 0 and c.expect[0] in (1, 2)))
    assert ran == set(WG)


def test_the_workspace_is_sized_for_every_form_the_plan_serves():
    """usf_conv_wgrad_workspace > 0 exactly where the masked or the unmasked call is served, and then the larger grid's slots
    (64 + 64 channels above 48 pixels: only the direct kernel serves them -- the workspace used to answer 0 there and every
    such call failed with "workspace too small")"""
    ext = _ext()
    lib, served_one_form = ext.load(), 0
    for cin in (16, 24, 32, 48, 64):
        for cout in (16, 32, 48, 64):
            for H, W in G.PICTURES + [(6, 8), (5, 10), (1, 49), (5, 13), (5, 1)]:
                for ks in (1, 3):
                    for B in (9, 300):
                        u, m = (ext.conv_wgrad_variant(B, cin, cout, H, W, ks, masked, 0, 0) for masked in (False, True))
                        ws = lib.usf_conv_wgrad_workspace(B, cin, cout, H, W, ks)
                        assert (ws > 0) == bool(u["kernel"] or m["kernel"]), (cin, cout, H, W, ks, B, ws)
                        if ws > 0:
                            assert ws == (4 * max(u["blocks"], m["blocks"]) + 64) * max(u["nacc"], m["nacc"])
                            served_one_form += bool(u["kernel"]) != bool(m["kernel"])
    assert served_one_form > 0


# ---- queued weight gradients ---------------------------------------------------------------------------------------------------
def _table(jobs, blocks_of):
    ext = _ext()
    raw, off, n = ext._job_table(jobs, blocks_of)
    t = torch.frombuffer(raw, dtype=torch.uint8).to(DEV)
    return t, off, n


def _psum_blocks(j):
    return ((j.n + 255) // 256 if j.vec4 else (j.n + 63) // 64) * j.rows


def _run_psums(pairs):
    """the sums the calls left: all first rounds in one usf_partial_sum_jobs_f32 launch, then all last rounds in another"""
    ext = _ext()
    st = ext.current_stream(torch.device(DEV))
    seen = set()
    for stage in (0, 1):
        js = [j2[stage] for j2 in pairs if j2[stage].nparts > 0]
        if js:
            seen |= {(stage, int(j.vec4)) for j in js}
            t, off, n = _table(js, _psum_blocks)
            assert ext.load().usf_partial_sum_jobs_f32(t.data_ptr(), t.data_ptr() + off, n, st) == 0
            torch.cuda.synchronize()
    return seen


@pytest.mark.parametrize("group", list(G.JOB_GROUPS))
def test_queued_weight_gradients_give_the_bits_of_the_single_calls(group):
    ext = _ext()
    lib, st = ext.load(), ext.current_stream(torch.device(DEV))
    members = [WgLaunch(WG[n]) for n in G.JOB_GROUPS[group]]
    single = [L.run() for L in members]
    assert all(rc == 0 for rc, _, _ in single)
    # planned: nothing is launched by the call, one usf_conv_wgrad_jobs_f32 for all of them with the largest lds_bytes
    planned, wjobs, job2s = [], [], []
    for L in members:
        bufW, bufb, ws, ws_n = L.buffers()
        job2, wjob = (ext.PsumJob * 2)(), ext.WgradJob()
        with G.knobs(lib, L.c.knobs):
            rc = lib.usf_conv_wgrad_plan_f32(*L.head(bufW, bufb, ws, ws_n), C.addressof(job2), C.addressof(wjob), st)
        assert rc == 0 and wjob.blocks == L.c.expect[5] > 0, (L.c.name, rc, wjob.blocks)
        torch.cuda.synchronize()
        assert G.untouched(bufW) and G.untouched(bufb)
        planned.append((bufW, bufb, ws))
        wjobs.append(wjob)
        job2s.append(job2)
    tiles = {(w.CIT, w.COT, w.T) for w in wjobs}
    assert len(tiles) == 1
    lds = [w.lds_bytes for w in wjobs]
    t, off, n = _table(wjobs, lambda w: w.blocks)
    assert lib.usf_conv_wgrad_jobs_f32(t.data_ptr(), t.data_ptr() + off, n, *next(iter(tiles)), max(lds), st) == 0
    torch.cuda.synchronize()
    seen = _run_psums(job2s)
    for L, (rc, sW, sb), (bufW, bufb, _) in zip(members, single, planned):
        assert torch.equal(G.bits(bufW), G.bits(sW)) and torch.equal(G.bits(bufb), G.bits(sb)), f"{group}: {L.c.name} differs from its single call"
    print(f"IGJ {group}: {len(members)} jobs, {n} blocks, lds_bytes {sorted(set(lds))}, sums seen (round, vec4) {sorted(seen)}")
    if group == "jobs_T1_1x1_mixed_lds":
        assert max(lds) > 2 * min(lds)
    if group in ("jobs_T9_1x1", "jobs_T1_1x1_mixed_lds"):
        assert {(0, 1), (1, 0)} <= seen                  # first rounds four columns per thread, last rounds (the dW map) scalar
    # deferred: the kernel is launched by the call, only the sums wait
    deferred, job2s = [], []
    for L in members:
        bufW, bufb, ws, ws_n = L.buffers()
        job2 = (ext.PsumJob * 2)()
        with G.knobs(lib, L.c.knobs):
            assert lib.usf_conv_wgrad_deferred_f32(*L.head(bufW, bufb, ws, ws_n), job2, st) == 0
        torch.cuda.synchronize()
        assert G.untouched(bufW) and G.untouched(bufb)
        deferred.append((bufW, bufb, ws))
        job2s.append(job2)
    _run_psums(job2s)
    for L, (rc, sW, sb), (bufW, bufb, _) in zip(members, single, deferred):
        assert torch.equal(G.bits(bufW), G.bits(sW)) and torch.equal(G.bits(bufb), G.bits(sb)), f"{group}: deferred {L.c.name} differs"


def test_deferred_direct_kernel_gives_the_bits_of_the_immediate_call():
    """the direct 1 x 1 kernel is launched by the plan call itself (wjob.blocks == 0); its sums wait like the others'"""
    ext = _ext()
    lib, st = ext.load(), ext.current_stream(torch.device(DEV))
    for name in ("red_300_slots_k1_direct", "k1_2x2_plain_b"):
        L = WgLaunch(WG[name])
        rc, sW, sb = L.run()
        bufW, bufb, ws, ws_n = L.buffers()
        job2, wjob = (ext.PsumJob * 2)(), ext.WgradJob()
        with G.knobs(lib, L.c.knobs):
            assert lib.usf_conv_wgrad_plan_f32(*L.head(bufW, bufb, ws, ws_n), C.addressof(job2), C.addressof(wjob), st) == 0
        assert wjob.blocks == 0
        torch.cuda.synchronize()
        assert G.untouched(bufW) and G.untouched(bufb)
        _run_psums([job2])
        assert rc == 0 and torch.equal(G.bits(bufW), G.bits(sW)) and torch.equal(G.bits(bufb), G.bits(sb)), name


# ---- LayerNorm backward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LN))
def test_layernorm_channels_bwd(name):
    c, ext = LN[name], _ext()
    lib = ext.load()
    a = ext.layernorm_channels_bwd_variant(c.B, c.C, c.P)
    assert (a["kernel"], a["width"], a["blocks"], a["rounds"]) == c.expect, (name, a)
    d = G.ln_data(c)
    kx, x = _rows_nan(d.x)
    ky, dy = _rows_nan(d.dy)
    gamma = d.gamma.to(DEV)
    ws_n = lib.usf_layernorm_channels_bwd_workspace(c.B, c.C, c.P)

    def run():
        bdx, bgb, ws = G.guarded(x.numel(), DEV), G.guarded(2 * c.C, DEV), _nan(ws_n)
        rc = lib.usf_layernorm_channels_bwd_f32(x.data_ptr(), dy.data_ptr(), bdx.data_ptr() + 4 * G.GUARD, c.B, c.C, c.P, gamma.data_ptr(),
                                                d.eps, c.act, c.slope, bgb.data_ptr() + 4 * G.GUARD, ws.data_ptr(), ws_n,
                                                ext.current_stream(torch.device(DEV)))
        torch.cuda.synchronize()
        return rc, bdx, bgb

    rc, bdx, bgb = run()
    if c.rc != 0:
        assert rc == c.rc and ws_n == 0 and G.untouched(bdx) and G.untouched(bgb), (name, rc)
        return
    assert rc == 0, (rc, lib.usf_last_error())
    r = G.ln_forward(c, G.Case(x=x, dy=dy, gamma=gamma, eps=d.eps), torch.float64)
    found = G.check("dx", bdx, r.dx, r.A_dx, "ln_dx")
    found += G.check("dgamma", bgb, r.dgamma, r.A_dgamma, "ln_dgamma", behind=False)
    found += G.check("dbeta", bgb, r.dbeta, r.A_dbeta, "ln_dbeta", lo=G.GUARD + c.C, front=False)
    assert bool((G.bits(bgb[:G.GUARD]) == G.SENTINEL_BITS).all())
    _report("ln_dx", name, bdx, r.dx, r.A_dx)
    _report("ln_dgamma", name, bgb, r.dgamma, r.A_dgamma)
    _report("ln_dbeta", name, bgb, r.dbeta, r.A_dbeta, lo=G.GUARD + c.C)
    assert found == [], (name, found)
    if c.act == G.LEAKY and c.slope == 0.0:
        zero = (x == 0)
        assert bool(zero.any()) and bool((bdx[G.GUARD:G.GUARD + x.numel()].view(x.shape)[zero] == 0).all())     # the gate is x > 0, not x >= 0
    rc2, bdx2, bgb2 = run()
    assert rc2 == 0 and torch.equal(G.bits(bdx2), G.bits(bdx)) and torch.equal(G.bits(bgb2), G.bits(bgb)), f"{name}: a second launch gives other bits"


# ---- gated residual, context gradient ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GR))
def test_gated_residual_bwd(name):
    c, ext = GR[name], _ext()
    lib = ext.load()
    d = G.gr_data(c)
    if c.B == 0:
        buf = G.guarded(2 * c.CP, DEV)
        z = torch.zeros(2 * c.CP, device=DEV)
        assert lib.usf_gated_residual_bwd_f32(z.data_ptr(), z.data_ptr(), buf.data_ptr() + 4 * G.GUARD, 0, c.CP, ext.current_stream(torch.device(DEV))) == 0
        torch.cuda.synchronize()
        assert G.untouched(buf)
        return
    kd, dy = _rows_nan(d.dy)
    kv, vg = _rows_nan(d.vg)

    def run():
        buf = G.guarded(vg.numel(), DEV)
        rc = lib.usf_gated_residual_bwd_f32(dy.data_ptr(), vg.data_ptr(), buf.data_ptr() + 4 * G.GUARD, c.B, c.CP, ext.current_stream(torch.device(DEV)))
        torch.cuda.synchronize()
        return rc, buf

    rc, buf = run()
    assert rc == 0
    r = G.gr_forward(c, G.Case(dy=dy, vg=vg), torch.float64)
    found = G.check("dvg", buf, r.dvg, r.A_dvg, "gr_dvg")
    _report("gr_dvg", name, buf, r.dvg, r.A_dvg)
    assert found == [], (name, found)
    rc2, buf2 = run()
    assert rc2 == 0 and torch.equal(G.bits(buf2), G.bits(buf))


@pytest.mark.parametrize("name", list(CTX))
def test_conv_ctx_wgrad(name):
    c, ext = CTX[name], _ext()
    lib = ext.load()
    d = G.ctx_data(c)
    kd, dy = _rows_nan(d.dy)
    kc, ctx = _rows_nan(d.ctx) if c.ctx_stride else (None, d.ctx.to(DEV))

    def run():
        buf = G.guarded(c.cout * c.ks * c.ks, DEV)
        rc = lib.usf_conv_ctx_wgrad_f32(dy.data_ptr(), ctx.data_ptr(), c.ctx_stride, c.B, c.cout, c.H, c.W, c.ks, buf.data_ptr() + 4 * G.GUARD,
                                        ext.current_stream(torch.device(DEV)))
        torch.cuda.synchronize()
        return rc, buf

    rc, buf = run()
    assert rc == 0
    r = G.ctx_forward(c, G.Case(dy=dy, ctx=ctx), torch.float64)
    found = G.check("dw_ctx", buf, r.dw, r.A_dw, "ctx_dw")
    _report("ctx_dw", name, buf, r.dw, r.A_dw)
    assert found == [], (name, found)
    rc2, buf2 = run()
    assert rc2 == 0 and torch.equal(G.bits(buf2), G.bits(buf))


# ---- the Python side's gates at the shape only one form of the weight gradient serves ----------------------------------------------
def _close(got, want, tol, what):
    want, got = want.double().cpu(), got.double().cpu()
    err, s = (got - want).abs().max().item(), max(want.abs().max().item(), 1e-30)
    assert got.shape == want.shape and err <= tol * s, f"{what}: max abs err {err:.3e} vs scale {s:.3e}"


@pytest.mark.parametrize("HW,masked_served", [((8, 8), False), ((7, 8), True)])
def test_a_masked_first_convolution_of_64_channels_trains(HW, masked_served):
    """64 -> 64 channels at kernel 1: above 56 pixels usf_conv_wgrad_f32 serves the call without an input mask only.  The gate
    of a conditioner's FIRST convolution -- the one a coupling hands its mask to -- asks for the masked form: at 8 x 8 the net
    declines device training and trains on the composite path (it used to: usf_conv_wgrad_workspace answered 0), at 7 x 8 it
    trains on the device; either way the gradients are those of fp64 autograd"""
    import copy
    import torch.nn.functional as F  # noqa: F401
    from usflows_amd import image_training as it
    from usflows_amd.networks import ConvNet2D
    H, W = HW
    B, C = 19, 64
    assert it.wgrad_served(B, C, C, H, W, 1, False) and it.wgrad_served(B, C, C, H, W, 1, True) == masked_served
    assert _ext().load().usf_conv_wgrad_workspace(B, C, C, H, W, 1) > 0
    torch.manual_seed(11)
    net = ConvNet2D(c_in=C, c_hidden=C, num_layers=1, nonlinearity=torch.nn.ReLU(), padding="same", kernel_size=1, normalize_layers=False,
                    gating=False)
    first = next(m for m in net.nn if isinstance(m, torch.nn.Conv2d))
    assert (first.in_channels, first.out_channels, first.kernel_size) == (C, C, (1, 1))
    ref = copy.deepcopy(net).double()
    net = net.to(DEV)
    assert it.conv_shape_ok(first, B, H, W, masked=True) == (masked_served and it.conv_shape_ok(first, B, H, W))
    x = torch.randn(B, C, H, W)
    dy = torch.randn(B, C, H, W)
    mask = (torch.rand(C * H * W) < 0.5).float()
    on_device = net.train_on_device(x.to(DEV).requires_grad_(True))
    assert on_device == it.conv_shape_ok(first, B, H, W, masked=True) and (masked_served or not on_device)

    # (as MaskedCoupling does: the mask is handed to the net where its first convolution runs on the device, else applied before)
    hand_over = on_device or net.first_conv_on_device(x.to(DEV))

    def grads(mod, t, g, m):
        for p in mod.parameters():
            p.grad = None
        t = t.clone().requires_grad_(True)
        y = mod(t, in_mul=m) if (mod is net and hand_over) else mod(t * m.view(1, C, H, W))
        y.backward(g)
        return y.detach(), t.grad, [p.grad.clone() for p in mod.parameters()]

    y, dx, gp = grads(net, x.to(DEV), dy.to(DEV), mask.to(DEV))           # (raised "does not serve this shape" had the gate said yes at 8 x 8)
    y6, dx6, gp6 = grads(ref, x.double(), dy.double(), mask.double())
    _close(y, y6, 2e-5, "y")
    _close(dx, dx6, 2e-5, "dx")
    for (k, _), a_, b_ in zip(net.named_parameters(), gp, gp6):
        _close(a_, b_, 2e-5, k)


def test_channel_affine_of_64_channels_at_8x8_trains_on_the_device():
    """the 1 x 1 convolution over 64 channels of an 8 x 8 picture (never masked): the direct kernel serves it, and since the
    workspace is sized for it the device path takes it"""
    import torch.nn.functional as F
    from usflows_amd.image_training import ChannelAffine, channel_affine_train_ok
    g = torch.Generator().manual_seed(64)
    B, C, HW = 21, 64, (8, 8)
    x, dy = torch.randn(B, C, *HW, generator=g), torch.randn(B, C, *HW, generator=g)
    Wm, b = torch.randn(C, C, generator=g) / C ** 0.5, torch.randn(C, generator=g)
    assert channel_affine_train_ok(x.to(DEV), C)
    for pre_sub in (False, True):
        xd, Wd, bd = x.to(DEV).requires_grad_(True), Wm.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        y = ChannelAffine.apply(xd, Wd, bd, pre_sub)
        y.backward(dy.to(DEV))
        x6, W6, b6 = x.double().requires_grad_(True), Wm.double().requires_grad_(True), b.double().requires_grad_(True)
        y6 = F.conv2d(x6 - b6.view(1, C, 1, 1), W6.view(C, C, 1, 1)) if pre_sub else F.conv2d(x6, W6.view(C, C, 1, 1), b6)
        y6.backward(dy.double())
        for got, want, what in ((y, y6, "y"), (xd.grad, x6.grad, "dx"), (Wd.grad, W6.grad, "dW"), (bd.grad, b6.grad, "db")):
            _close(got, want, 1e-5, what)
