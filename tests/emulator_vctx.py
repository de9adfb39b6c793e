"""tests/emulator.py with the vector-context form of the fused additive coupling (usf_coupling_additive_vctx_f32,
include/usflows_hip_internal.h): ``emulate_coupling`` restated with ConditionalDenseNN's rank-C context term -- the first layer's
pre-activation becomes v + (b_ctx + sum_c ctx[row, c] W_ctx_t[c, :]) over the C real columns only -- and the launch list's prefix
op (USF_OP_CALL / USF_FN_COUPLING_VCTX: the six context arguments of the USF_OP_COUPLING op behind it).  ``install`` puts both
over tests/emulator.py's interpreter, and fills the workspace's context rows the way the engine does (``_fill_context``)."""
import ctypes as C

import torch

import emulator
from emulator import PtrMap
from usflows_amd import _ext


def emulate_coupling_vctx(d, pm: PtrMap, dtype, ctx):
    """emulator.emulate_coupling + the vector context; ctx = (ctx pointer, ld_ctx, ctx_dim, W_ctx_t pointer, ldw_ctx, b_ctx pointer)"""
    cptr, ld_ctx, cdim, wptr, ldw, bptr = ctx
    M = d.M
    assert d.act != _ext.ACT_GATE, "USF_ACT_GATE takes no context"
    assert not (d.context or d.W_ctx or d.b_ctx), "the descriptor's own context fields must be NULL"
    assert 1 <= cdim <= _ext.VCTX_MAX and ld_ctx % 4 == 0 and (ld_ctx == 0 or ld_ctx >= -(-cdim // 4) * 4) and ldw % 4 == 0
    assert cptr % 16 == 0 and wptr % 16 == 0 and bptr % 16 == 0

    def finish(v, l):
        if d.act == _ext.ACT_LEAKY_RELU:
            v = torch.where(v > 0, v, v * d.slope)
        if d.hidden_out[l]:
            pm.view(d.hidden_out[l], M, d.hidden[l], d.ld_hidden_out).copy_(v.to(torch.float32))
        return v

    h0 = d.hidden[0]
    zp = pm.view(d.z + 4 * d.off_pass, M, d.n_pass, d.ldz).to(dtype)
    h = zp @ pm.view(d.W_in, h0, d.n_pass, d.ldw_in).to(dtype).t() + pm.vec(d.b_in, h0).to(dtype)
    # only the cdim real columns: whatever the padding columns [cdim, round_up(cdim, 4)) hold never enters
    c = pm.view(cptr, M if ld_ctx else 1, cdim, ld_ctx if ld_ctx else cdim).to(dtype)
    c = c if ld_ctx else c.expand(M, cdim)
    Wt = pm.view(wptr, cdim, h0, ldw).to(dtype)
    h = finish(h + (pm.vec(bptr, h0).to(dtype) + c @ Wt), 0)
    for j in range(d.n_hidden - 1):
        W = pm.view(d.W_hid[j], d.hidden[j + 1], d.hidden[j], d.ldw_hid[j]).to(dtype)
        h = finish(h @ W.t() + pm.vec(d.b_hid[j], d.hidden[j + 1]).to(dtype), j + 1)
    Wo = pm.view(d.W_out, d.n_trans, d.hidden[d.n_hidden - 1], d.ldw_out).to(dtype)
    t = h @ Wo.t() + pm.vec(d.b_out, d.n_trans).to(dtype)
    zt = pm.view(d.z + 4 * d.off_trans, M, d.n_trans, d.ldz).to(dtype)
    assert d.out == d.z
    pm.view(d.out + 4 * d.off_trans, M, d.n_trans, d.ldo).copy_((zt + d.sign * t).to(torch.float32))


class _Pending:
    """the context arguments a prefix op left for the coupling op behind it"""
    ctx = None
    seen = 0            # vector-context launches interpreted (the tests assert the vector form really ran)


def _op_of(member) -> "_ext.Op":
    """the usf_op a union member (op.u.<member>) lives in"""
    return _ext.Op.from_address(C.addressof(member) - _ext.Op.u.offset)


def install(monkeypatch):
    """tests/emulator.py's run_plan hands every op kind it does not know to ``emulate_coupling``: the prefix op is caught there and
    the coupling op behind it becomes the vector-context form.  The engine's ``_execute`` / ``_execute_plain`` fill the context
    rows with the engine's own ``_fill_context`` and run the list through run_plan."""
    from usflows_amd.engine import FlowEngine
    real_coupling = emulator.emulate_coupling
    _Pending.ctx, _Pending.seen = None, 0

    def coupling_or_prefix(d, pm, dtype=torch.float32):
        op = _op_of(d)
        if op.kind == _ext.OP_CALL:
            a = op.u.call.a
            assert op.u.call.fn == _ext.FN_COUPLING_VCTX and op.u.call.n_args == 6 and _Pending.ctx is None
            _Pending.ctx = tuple(int(a[j]) for j in range(6))
            return
        ctx, _Pending.ctx = _Pending.ctx, None
        if ctx is None:
            return real_coupling(d, pm, dtype)
        assert op.kind == _ext.OP_COUPLING
        for cp in emulator._LAST_RUN["plan"]["pk"]["coupling"].values():     # (run_plan's pointer map predates the transposed image)
            pm.add(cp.get("fused", {}).get("W_ctx_t"))
        _Pending.seen += 1
        emulate_coupling_vctx(d, pm, dtype, ctx)

    monkeypatch.setattr(emulator, "emulate_coupling", coupling_or_prefix)

    def execute(self, plan, x, out, context, dtype=torch.float64):
        if context is not None:
            self._fill_context(plan, context, x.shape[0])
        emulator.run_plan(self, plan, x, out, None, dtype=dtype)

    monkeypatch.setattr(FlowEngine, "_execute_plain", execute)
    monkeypatch.setattr(FlowEngine, "_execute", execute)
    return _Pending
