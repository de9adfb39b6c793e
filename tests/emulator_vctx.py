"""tests/emulator.py with the vector-context form of the fused additive coupling (usf_coupling_additive_vctx_f32,
include/usflows_hip_internal.h): ``emulate_coupling`` restated with ConditionalDenseNN's rank-C context term -- the first layer's
pre-activation becomes v + (b_ctx + sum_c ctx[row, c] W_ctx_t[c, :]) over the C real columns only -- and the launch list's prefix
op (USF_OP_CALL / USF_FN_COUPLING_VCTX: the six context arguments of the USF_OP_COUPLING op behind it).  ``install`` puts both
over tests/emulator.py's interpreter, and fills the workspace's context rows the way the engine does (``_fill_context``)."""
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
    """how many vector-context launches were interpreted (the tests assert the vector form really ran)"""
    seen = 0


def register(monkeypatch):
    """the prefix op's branch of tests/emulator.py's interpreter (emulator.CALL_HANDLERS): USF_FN_COUPLING_VCTX takes six
    arguments and applies to a USF_OP_COUPLING op behind it -- anything else is refused, as usf_run_ops refuses it"""
    _Pending.seen = 0

    def prefix(call, nxt, pm, dtype=torch.float32):
        if call.n_args != 6:
            raise ValueError("USF_FN_COUPLING_VCTX takes 6 arguments")
        if nxt is None or nxt.kind != _ext.OP_COUPLING:
            raise ValueError("USF_FN_COUPLING_VCTX must be followed by a USF_OP_COUPLING op")
        _Pending.seen += 1
        emulate_coupling_vctx(nxt.u.coupling, pm, dtype, tuple(int(call.a[j]) for j in range(6)))

    monkeypatch.setitem(emulator.CALL_HANDLERS, _ext.FN_COUPLING_VCTX, prefix)
    return _Pending


def install(monkeypatch):
    """``register`` + the engine's ``_execute`` / ``_execute_plain``: they fill the context rows with the engine's own
    ``_fill_context`` and run the list through run_plan."""
    from usflows_amd.engine import FlowEngine
    register(monkeypatch)

    def execute(self, plan, x, out, context, dtype=torch.float64):
        if context is not None:
            self._fill_context(plan, context, x.shape[0])
        emulator.run_plan(self, plan, x, out, None, dtype=dtype)

    monkeypatch.setattr(FlowEngine, "_execute_plain", execute)
    monkeypatch.setattr(FlowEngine, "_execute", execute)
    return _Pending
