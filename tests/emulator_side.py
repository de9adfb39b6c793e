"""tests/emulator.py with the fp32 side buffer of the planes inference plans (usf_gemm_planes_side / usf_coupling_planes_side,
include/usflows_hip_internal.h): the two prefix ops of the launch list (USF_OP_CALL / USF_FN_GEMM_PLANES_SIDE: side, side_kb0,
side_kbn, both_kb0, both_kbn in front of a USF_OP_GEMM_PLANES op; USF_FN_COUPLING_PLANES_SIDE: side, side_nkb in front of a
USF_OP_COUPLING_PLANES op) as the header documents them.  The GEMM's side blocks leave as fp32 and their planes are POISONED unless
they lie in the both range -- the kernel does not write them, so nothing behind it may read them -- and the coupling takes its
residual from the side buffer alone.  ``register`` puts both over tests/emulator.py's interpreter."""
import torch

import emulator
from emulator import PtrMap, _slot_feature, planes_decode, planes_encode, planes_view
from usflows_amd import _ext


def side_view(pm: PtrMap, ptr, npanels, nkb):
    """[npanels, nkb, 64 lanes, 8 slots] fp32 view of a side buffer at raw address ptr (2 KiB per chunk, 32 bytes per lane)"""
    n = npanels * nkb * 2048
    return pm.view(ptr, 1, n, n, dtype=torch.uint8)[0].view(torch.float32).view(npanels, nkb, 64, 8)


def side_encode(v, X):
    """logical fp32 matrix X [M, 32 nkb] into a side view: lane 16 g + j, slot u = feature slot_feature(8 g + u) of row j"""
    npan, nkb = v.shape[0], v.shape[1]
    Xp = torch.zeros(npan * 16, nkb * 32)
    Xp[: X.shape[0]] = X
    Xp = Xp.view(npan, 16, nkb, 32)
    for g in range(4):
        for u in range(8):
            v[:, :, 16 * g: 16 * g + 16, u] = Xp[:, :, :, _slot_feature(8 * g + u)].permute(0, 2, 1)


def side_decode(v, M):
    npan, nkb = v.shape[0], v.shape[1]
    out = torch.zeros(npan, 16, nkb, 32)
    for g in range(4):
        for u in range(8):
            out[:, :, :, _slot_feature(8 * g + u)] = v[:, :, 16 * g: 16 * g + 16, u].permute(0, 2, 1)
    return out.reshape(npan * 16, nkb * 32)[:M]


def emulate_gemm_planes_side(d, pm: PtrMap, dtype, side, s0, sn, b0, bn):
    if not side or side % 16:
        raise ValueError("usf_gemm_planes_side: side must be a 16-byte aligned buffer")
    if d.C_f32 or d.base_part or d.residual:
        raise ValueError("usf_gemm_planes_side: the side output needs planes output and no residual")
    if sn <= 0 or s0 < 0 or s0 + sn > d.c_kbn or bn < 0 or (bn > 0 and (b0 < s0 or b0 + bn > s0 + sn)):
        raise ValueError("usf_gemm_planes_side: bad block ranges")
    M, fmt = d.M, d.format
    npan = -(-M // 16)
    emulator.emulate_gemm_planes(d, pm, dtype)
    Cv = planes_view(pm, d.C_planes, npan, d.c_nkb, fmt)
    # the side value is the float the planes hold (bf16x3: the accumulator itself; fp16x2: the sum of its two planes), rows of the
    # last panel beyond M included
    blocks = Cv[:, d.c_kb0 + s0: d.c_kb0 + s0 + sn]
    side_encode(side_view(pm, side, npan, sn), planes_decode(blocks, npan * 16))
    for kb in range(s0, s0 + sn):
        if not (b0 <= kb < b0 + bn):
            Cv[:, d.c_kb0 + kb] = float("nan")              # not written by the kernel: whoever reads it gets NaN


def emulate_coupling_planes_side(d, pm: PtrMap, dtype, side, side_nkb):
    if not side or side % 16:
        raise ValueError("usf_coupling_planes_side: side must be a 16-byte aligned buffer")
    if side_nkb != d.nk_t:
        raise ValueError("usf_coupling_planes_side: side_nkb must equal nk_t")
    if d.hidden_out[0] or d.hidden_out[1] or d.act == _ext.ACT_GATE:
        raise ValueError("usf_coupling_planes_side: inference launches only")
    M, fmt = d.M, d.format
    npan = -(-M // 16)
    zv = planes_view(pm, d.z, npan, d.z_nkb, fmt)
    # the conditioning blocks must be readable as they are (the both range); the transformed blocks' residual is the side value,
    # whose split is exact: the plain emulation on a z that holds it computes what the kernel computes
    keep = zv[:, d.kb_p0: d.kb_p0 + d.nk_p].clone()
    planes_encode(zv, side_decode(side_view(pm, side, npan, d.nk_t), npan * 16), d.kb_t0)
    if fmt == 0:
        assert torch.equal(zv[:, d.kb_p0: d.kb_p0 + d.nk_p].view(torch.int16), keep.view(torch.int16)), \
            "a block the first layer reads does not hold the planes of its side value"
    else:
        # fp16x2: the side value is the SUM of the two planes, whose own split may choose another pair with that sum; the first
        # layer reads the pair the GEMM stored
        zv[:, d.kb_p0: d.kb_p0 + d.nk_p] = keep
    emulator.emulate_coupling_planes(d, pm, dtype)


class _Seen:
    gemm = 0
    coupling = 0


def register(monkeypatch):
    """the two prefix ops' branches of tests/emulator.py's interpreter (emulator.CALL_HANDLERS); a prefix with the wrong argument
    count or in front of another kind of op is refused, as usf_run_ops refuses it"""
    _Seen.gemm = _Seen.coupling = 0

    def gemm_prefix(call, nxt, pm, dtype=torch.float32):
        if call.n_args != 5 or nxt is None or nxt.kind != _ext.OP_GEMM_PLANES:
            raise ValueError("USF_FN_GEMM_PLANES_SIDE takes 5 arguments and a USF_OP_GEMM_PLANES op behind it")
        _Seen.gemm += 1
        emulate_gemm_planes_side(nxt.u.gemm_planes, pm, dtype, *(int(call.a[j]) for j in range(5)))

    def coupling_prefix(call, nxt, pm, dtype=torch.float32):
        if call.n_args != 2 or nxt is None or nxt.kind != _ext.OP_COUPLING_PLANES:
            raise ValueError("USF_FN_COUPLING_PLANES_SIDE takes 2 arguments and a USF_OP_COUPLING_PLANES op behind it")
        _Seen.coupling += 1
        emulate_coupling_planes_side(nxt.u.coupling_planes, pm, dtype, int(call.a[0]), int(call.a[1]))

    monkeypatch.setitem(emulator.CALL_HANDLERS, _ext.FN_GEMM_PLANES_SIDE, gemm_prefix)
    monkeypatch.setitem(emulator.CALL_HANDLERS, _ext.FN_COUPLING_PLANES_SIDE, coupling_prefix)
    return _Seen
