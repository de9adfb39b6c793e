"""The small-batch kernel, the exact-f32 tiles and the bf16x3 tiles behind usf_linear_f32 on a real MI355X, instantiation by
instantiation, one launch per case of tests/linear_kernel_cases.py against fp64: descriptors built by hand from the header's
contract, a NaN with a payload of its own in every element the launch must not read into a result or write.
Bound on every element of C[:M, :N]: max(4 err32, 2e-6 max(1, max |ref64|)) with err32 the error of the same layer in fp32 on the
CPU (tests/test_kernels_gpu.py: test_linear_parity's rule; tests/test_coupling_kernels_gpu.py); nothing is tuned to the kernels."""
import ctypes as C

import pytest
import torch

import linear_kernel_cases as lk
from test_coupling_kernels_gpu import _same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _launch(c, p, overrides=None, side=None):
    """ONE usf_linear_f32 launch under the case's knobs on device copies of the case's buffers (`overrides`: CPU tensors that
    replace some of them; side: with or without A_planes_out, default the case's): (C after it, planes after it or None, the
    read-only buffers after it), CPU tensors"""
    from usflows_amd import _ext
    lib = _ext.load()
    host = {name: p[name] for name in lk.INPUTS if name in p}
    host.update(overrides or {})
    side = c.side if side is None else side
    bufs = {name: t.to(DEV) for name, t in host.items()}
    bufs["C"] = p["C0"].to(DEV)
    if side:
        bufs["planes"] = p["planes0"].to(DEV)
    assert _same_bits(bufs["C"].cpu(), p["C0"]) and _same_bits(bufs["A"].cpu(), host["A"])          # NaN payloads survive the copy
    d = lk.descriptor(c, lambda name: bufs[name].data_ptr(), _ext.LinearDesc, side=side)
    with lk.knobs(c.knobs):
        assert lib.usf_linear_variant(C.byref(d)) == lk.instantiation(c)[1]
        rc = lib.usf_linear_f32(C.byref(d), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.usf_last_error()
    torch.cuda.synchronize()
    for name, t in host.items():
        view = (lambda x: x.view(torch.int16)) if t.dtype == torch.bfloat16 else (lambda x: x.view(torch.int32))
        assert torch.equal(view(bufs[name].cpu()), view(t)), f"the launch changed its input {name}"
    return bufs["C"].cpu(), (bufs["planes"].cpu() if side else None)


@pytest.mark.parametrize("c", lk.CASES, ids=lk.case_id)
def test_linear_kernel_vs_fp64(c):
    """accuracy of C[:M, :N], nothing else written in any buffer (bit for bit, NaN payloads included), the same bits from a
    second launch, and rows that do not depend on each other: the launch on row-permuted A / residual / addend / gate gives the
    row-permuted C bit for bit (in all three kernels a row's sum runs over k in an order that does not depend on the lane, wave
    or block that holds the row).  A_planes_out cases: C as without the side output, the planes of the rows [0, M) and columns
    [0, K) as usf_split_planes_f32 makes them, the rows [M, ceil32(M)) still the caller's zeros"""
    p = lk.prepared(c)
    got, planes = _launch(c, p)
    m = lk.measure(got, c)
    print(f"LK|{'|'.join(map(str, lk.instantiation(c)))}|{m['err']:.3e}|{m['err32']:.3e}|{m['bound']:.3e}")
    assert lk.check(got, c) == []
    # reproducibility
    again, planes2 = _launch(c, p)
    assert _same_bits(again, got)
    # rows are independent
    perm = torch.randperm(c.M, generator=torch.Generator().manual_seed(c.M))

    def permuted(t):
        out = t.clone()
        out[: c.M] = t[perm]
        return out

    moved = {name: permuted(p[name]) for name in ("A", "extra") if name in p}
    got_perm, _ = _launch(c, p, overrides=moved)
    want = got.clone()
    want[: c.M, : c.N] = got[perm, : c.N]                                        # (the slack columns of C keep their own NaNs)
    assert _same_bits(got_perm, want), "rows depend on their position"
    if c.side:
        from usflows_amd import _ext
        M, K, mp, L = c.M, c.K, lk.ceil_to(c.M, 32), lk.layout(c)
        assert planes2.dtype == torch.bfloat16 and torch.equal(planes.view(torch.int16), planes2.view(torch.int16))
        plain, none = _launch(c, p, side=False)
        assert none is None and _same_bits(plain, got), "C depends on A_planes_out"
        want = torch.full((3, mp, L["ldp"]), 1.0, dtype=torch.bfloat16, device=DEV)
        _ext.split_planes(p["A"].to(DEV), want, M=M, N=K, ldx=L["lda"])
        torch.cuda.synchronize()
        want = want.cpu()
        assert torch.equal(planes[:, :M, :K].contiguous().view(torch.int16), want[:, :M, :K].contiguous().view(torch.int16))
        assert torch.equal(want[:, :M, :K].float().sum(0), p["A"][:M, :K])          # (and those are the planes of A: exact sum)
        assert (planes[:, M:mp].view(torch.int16) == 0).all(), "rows [M, ceil32(M)) of the planes written"
        assert torch.isfinite(planes[:, :M, K: lk.ceil_to(K, 32)].float()).all()
        assert (planes[:, mp].float() == lk.SENTINEL).all(), "written behind a plane"


# ---- the header's words and the engine's packer agree -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(128, 64), (100, 136)])
def test_engine_packer_splits_the_planes_of_the_header(N, K):
    """FlowEngine._split_planes gives the hand-built W_split planes bit for bit: [3, N, ceil32(K)], round-to-nearest residual
    split, zero in [K, ceil32(K))"""
    from usflows_amd.engine import FlowEngine
    c = next(c for c in lk.CASES if c.family == "bf16x3" and (c.N, c.K) == (N, K) and c.M < 2000)
    p = lk.prepared(c)
    kp = lk.ceil_to(K, 32)
    W = p["W"][:N, :K].contiguous().to(DEV)
    planes = FlowEngine._split_planes({"mats": {}}, W)
    torch.cuda.synchronize()
    assert planes.dtype == torch.bfloat16 and tuple(planes.shape) == (3, N, kp)
    assert torch.equal(planes.cpu().view(torch.int16), p["W_split"][:, :N, :kp].contiguous().view(torch.int16))
