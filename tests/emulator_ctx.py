"""tests/emulator.py with the context form of the fused planes coupling (usf_coupling_planes_ctx, include/usflows_hip_internal.h):
``emulate_coupling_planes`` restated with ConditionalDenseNN's context term -- the first layer's pre-activation starts at
b_in + b_ctx + ctx[row * ctx_stride] * w_ctx -- and the launch list's prefix op (USF_OP_CALL / USF_FN_COUPLING_PLANES_CTX: the
four context arguments of the USF_OP_COUPLING_PLANES op behind it).  ``install`` puts both over tests/emulator.py's interpreter and
over the binding's direct call."""
import torch

import emulator
from emulator import PtrMap, _SLOT_OF_FEATURE, planes_decode, planes_encode, planes_view
from usflows_amd import _ext


def emulate_coupling_planes_ctx(d, pm: PtrMap, dtype=torch.float32, ctx=None):
    """emulator.emulate_coupling_planes + the context term; ctx = (ctx pointer, ctx_stride, w_ctx pointer, b_ctx pointer) or None"""
    M, fmt = d.M, d.format
    npl = 2 if fmt == 1 else 3
    npan = -(-M // 16)
    zv = planes_view(pm, d.z, npan, d.z_nkb, fmt)
    Z = planes_decode(zv, M)

    def weights(ptr, rows, ld, plane, K):
        Wp = pm.view(ptr, npl, rows * ld, plane).view(npl, rows, ld)
        W = Wp[0].float() + Wp[1].float()
        if npl == 3:
            W = W + Wp[2].float()
        slot = torch.tensor([32 * (c // 32) + _SLOT_OF_FEATURE[c % 32] for c in range(K)])
        return W[:, :K][:, slot]

    assert not (ctx is not None and d.act == _ext.ACT_GATE), "USF_ACT_GATE takes no context"

    def act(v, l):
        if d.act == _ext.ACT_LEAKY_RELU:
            v = torch.where(v > 0, v, v * d.slope)
        if l < 2 and d.hidden_out[l]:
            planes_encode(planes_view(pm, d.hidden_out[l], npan, 8, fmt), v.to(torch.float32), 0)
        return v

    A = Z[:, 32 * d.kb_p0: 32 * (d.kb_p0 + d.nk_p)].to(dtype)
    pre = A @ weights(d.W_in, 256, d.ldw_in, d.w_in_plane, 32 * d.nk_p).to(dtype).t() + pm.vec(d.b_in, 256).to(dtype)
    if ctx is not None:
        cptr, stride, wptr, bptr = ctx
        assert stride in (0, 1)
        c = pm.vec(cptr, M if stride else 1).to(dtype)
        c = c if stride else c.expand(M)
        pre = pre + pm.vec(bptr, 256).to(dtype) + c[:, None] * pm.vec(wptr, 256).to(dtype)[None, :]
    h = act(pre, 0)
    for j in range(d.n_hidden - 1):
        h = act(h @ weights(d.W_hid[j], 256, d.ldw_hid, d.w_hid_plane, 256).to(dtype).t() + pm.vec(d.b_hid[j], 256).to(dtype), j + 1)
    out = h @ weights(d.W_out, 32 * d.nk_t, d.ldw_out, d.w_out_plane, 256).to(dtype).t() + pm.vec(d.b_out, 32 * d.nk_t).to(dtype)
    v = Z[:, 32 * d.kb_t0: 32 * (d.kb_t0 + d.nk_t)].to(dtype) + d.sign * out
    if fmt == 1 and d.range_flag and not bool((v.abs() < 65000.0).all() and (h.abs() < 65000.0).all()):
        pm.view(d.range_flag, 1, 1, 1, dtype=torch.int32)[0, 0] = 1
    planes_encode(zv, v.to(torch.float32), d.kb_t0)


class _Pending:
    """how many context launches were interpreted (the tests assert the context form really ran)"""
    seen = 0


def register(monkeypatch):
    """the prefix op's branch of tests/emulator.py's interpreter (emulator.CALL_HANDLERS): USF_FN_COUPLING_PLANES_CTX takes four
    arguments and applies to a USF_OP_COUPLING_PLANES op behind it -- anything else is refused, as usf_run_ops refuses it"""
    _Pending.seen = 0

    def prefix(call, nxt, pm, dtype=torch.float32):
        if call.n_args != 4:
            raise ValueError("USF_FN_COUPLING_PLANES_CTX takes 4 arguments")
        if nxt is None or nxt.kind != _ext.OP_COUPLING_PLANES:
            raise ValueError("USF_FN_COUPLING_PLANES_CTX must be followed by a USF_OP_COUPLING_PLANES op")
        _Pending.seen += 1
        emulate_coupling_planes_ctx(nxt.u.coupling_planes, pm, dtype, tuple(int(call.a[j]) for j in range(4)))

    monkeypatch.setitem(emulator.CALL_HANDLERS, _ext.FN_COUPLING_PLANES_CTX, prefix)
    return _Pending


def install(monkeypatch):
    """``register`` + the binding's direct call (_ext.coupling_planes_ctx_op) on the CPU"""
    register(monkeypatch)

    def ctx_op(op, ctx, ctx_stride, w_ctx, b_ctx, device):        # the binding's direct call (_ext.coupling_planes_ctx_op)
        if ctx is None:
            return emulator._emu_coupling_planes_op(op, device)
        plan = emulator._LAST_RUN["plan"]
        pm = PtrMap()
        for t in list(plan["ws"].values()) + [ctx, w_ctx, b_ctx]:
            pm.add(t)
        for group in ("mats", "vecs"):
            for t in plan["pk"][group].values():
                pm.add(t)
        _Pending.seen += 1
        emulate_coupling_planes_ctx(op.u.coupling_planes, pm, torch.float64,
                                    (ctx.data_ptr(), int(ctx_stride), w_ctx.data_ptr(), b_ctx.data_ptr()))

    monkeypatch.setattr(_ext, "coupling_planes_ctx_op", ctx_op)
    return _Pending
