"""The exact-f32 MFMA kernel and the bf16x3 kernel behind usf_coupling_additive_f32 on a real MI355X, instantiation by
instantiation, one launch per case of tests/coupling_kernel_cases.py against fp64: descriptors built by hand from the header's
padding contract, NaN in every element the launch must not read into a result or write, a sentinel in the hidden_out buffers.
Bound on every compared value: max(4 err32, 2e-6 max(1, max |ref|)) with err32 the error of the same layer in fp32 on the CPU
(tests/test_kernels_gpu.py: test_linear_parity's rule, test_tiny_layer_coupling_kernel's floor); nothing is tuned to the kernels."""
import ctypes as C

import pytest
import torch

import coupling_kernel_cases as ck

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _tiny_kernel_off():
    """the exact-f32 cases with M <= 256 and everything <= 64 would otherwise be the tiny-layer kernel's"""
    from usflows_amd import _ext
    _ext.load()
    with ck.tiny_kernel_off():
        yield


_DEVICE_IMAGES = {}


def _device_images(c):
    """the case's weight images on the device, one copy per distinct weight set"""
    key = (c.n_pass, c.hidden, c.n_trans, c.family == "bf16x3")
    if key not in _DEVICE_IMAGES:
        im, dev = ck.case_images(c), {}
        for name, v in im.items():
            if torch.is_tensor(v):
                dev[name] = v.to(DEV)
            elif isinstance(v, list):
                for l, t in enumerate(v):
                    dev[f"{name}{l}"] = t.to(DEV)
        _DEVICE_IMAGES[key] = dev
    return _DEVICE_IMAGES[key]


def _launch(c, z, ctx, gates):
    """ONE usf_coupling_additive_f32 launch on device copies of the given CPU inputs: (z after it, hidden_out buffers after it
    or None), CPU tensors"""
    from usflows_amd import _ext
    lib = _ext.load()
    p = ck.prepared(c)
    bufs = dict(_device_images(c))
    bufs["z"] = z.to(DEV)
    if ctx is not None:
        bufs["context"] = ctx.to(DEV)
    for l, gt in enumerate(gates or []):
        bufs[f"gate{l}"] = gt.to(DEV)
    houts = None
    if c.mode in ("hidden_out", "gate"):
        houts = [torch.full((c.M + ck.EXTRA_ROWS, p["Hp"] + ck.HIDDEN_SLACK), ck.SENTINEL, device=DEV) for _ in c.hidden]
        for l, h in enumerate(houts):
            bufs[f"hidden_out{l}"] = h
    assert torch.equal(bufs["z"].cpu().view(torch.int32), z.view(torch.int32))          # NaN payloads survive the copy
    d = ck.descriptor(c, lambda name: bufs[name].data_ptr(), _ext.CouplingDesc)
    assert lib.usf_coupling_variant(C.byref(d)) == ck.VARIANT[c.family]
    rc = lib.usf_coupling_additive_f32(C.byref(d), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.usf_last_error()
    torch.cuda.synchronize()
    return bufs["z"].cpu(), (None if houts is None else [h.cpu() for h in houts])


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("c", ck.CASES, ids=ck.case_id)
def test_coupling_kernel_vs_fp64(c):
    """accuracy of the transformed columns and of hidden_out, nothing else written (bit for bit, NaN payloads included), the same
    bits from a second launch, and rows that do not depend on each other: the launch on row-permuted inputs gives the permuted
    output bit for bit (a row's sums run over k in an order that does not depend on the lane that holds the row)"""
    from usflows_amd import _ext
    assert ck.variant(c, _ext.load(), _ext.CouplingDesc) == ck.VARIANT[c.family]
    p = ck.prepared(c)
    got_z, got_h = _launch(c, p["z"], p["ctx"], p["gates"])
    m = ck.measure(got_z, got_h, c)
    print(f"CK|{c.family}|{len(c.hidden)}|{p['Hp']}|{c.mode}|{m['err']:.3e}|{m['err32']:.3e}|{m['bound']:.3e}|"
          + ";".join(f"{e:.3e}/{e32:.3e}/{b:.3e}" for e, e32, b in m["hidden"]))
    assert ck.check(got_z, got_h, c) == []
    # reproducibility
    z2, h2 = _launch(c, p["z"], p["ctx"], p["gates"])
    assert _same_bits(z2, got_z) and all(_same_bits(a, b) for a, b in zip(h2 or [], got_h or []))
    # rows are independent
    perm = torch.randperm(c.M, generator=torch.Generator().manual_seed(c.M))

    def permuted(t):
        if t is None:
            return None
        out = t.clone()
        out[: c.M] = t[perm]
        return out

    z3, h3 = _launch(c, permuted(p["z"]), permuted(p["ctx"]), None if p["gates"] is None else [permuted(gt) for gt in p["gates"]])
    assert _same_bits(z3, permuted(got_z)), "rows depend on their position"
    assert all(_same_bits(a, permuted(b)) for a, b in zip(h3 or [], got_h or [])), "hidden_out rows depend on their position"


# ---- the header's contract and the engine's packer agree ------------------------------------------------------------------------------
def _engine_images(n_pass, hidden, n_trans, split, with_ctx):
    """FlowEngine._fused_images on raw nn.Linear-shaped parameters that hold the weight set of coupling_kernel_cases among the
    columns / rows of other features, as a conditioner's do (mask-aware selection)"""
    from usflows_amd.engine import FlowEngine
    w = ck.weights(n_pass, hidden, n_trans)
    nh = len(hidden)
    g = torch.Generator().manual_seed(n_pass + n_trans)
    D = n_pass + n_trans + 5
    feat = torch.randperm(D, generator=g)
    pass_idx, tr_idx = feat[:n_pass], feat[n_pass: n_pass + n_trans]
    first = torch.randn(hidden[0], D, generator=g)
    first[:, pass_idx] = w["Ws"][0]
    last, b_last = torch.randn(D, hidden[-1], generator=g), torch.randn(D, generator=g)
    last[tr_idx], b_last[tr_idx] = w["Ws"][nh], w["bs"][nh]
    dev = lambda t: t.to(DEV).contiguous()      # noqa: E731
    raw = dict(device=torch.device(DEV), h=list(hidden), first=(dev(first), dev(w["bs"][0])),
               hidden=[(dev(w["Ws"][l]), dev(w["bs"][l])) for l in range(1, nh)], last=(dev(last), dev(b_last)),
               pass_idx=pass_idx.to(torch.int32), tr_idx=tr_idx.to(torch.int32), ctx=(dev(w["Wc"][:, None]), dev(w["bc"])))
    cp = dict(pass_n=n_pass, tr_n=n_trans, has_ctx=with_ctx, raw=raw)
    eng = FlowEngine.__new__(FlowEngine)
    eng.ctx_dim = 1
    f = eng._fused_images(cp, ck.padded_width(max(hidden)), split)
    torch.cuda.synchronize()
    return f


@pytest.mark.parametrize("family,hidden", [("f32", (65, 128)), ("bf16x3", (136, 256, 130))])
def test_engine_packer_builds_the_images_of_the_header(family, hidden):
    """the images FlowEngine._fused_images builds equal the hand-built ones bit for bit, permuted planes included"""
    c = next(c for c in ck.CASES if c.family == family and c.hidden == hidden and c.n_trans % 32 and c.n_pass % 32)
    im = ck.case_images(c)
    f = _engine_images(c.n_pass, c.hidden, c.n_trans, family == "bf16x3", True)
    bits16 = lambda t: t.cpu().contiguous().view(torch.int16)      # noqa: E731
    assert f["Hp"] == im["Hp"]
    for name in ("W_in", "b_in", "W_out", "b_out", "W_ctx", "b_ctx"):
        assert f[name].shape == im[name].shape and _same_bits(f[name].cpu(), im[name]), name
    assert len(f["hid"]) == len(hidden) - 1
    for l, (W, b) in enumerate(f["hid"]):
        assert _same_bits(W.cpu(), im["W_hid"][l]) and _same_bits(b.cpu(), im["b_hid"][l]), l
    if family == "bf16x3":
        s = f["split"]
        assert s["in"].shape == im["split_in"].shape and torch.equal(bits16(s["in"]), bits16(im["split_in"]))
        assert s["out"].shape == im["split_out"].shape and torch.equal(bits16(s["out"]), bits16(im["split_out"]))
        assert len(s["hid"]) == len(hidden) - 1
        for l, P in enumerate(s["hid"]):
            assert P.shape == im["split_hid"][l].shape and torch.equal(bits16(P), bits16(im["split_hid"][l])), l
    else:
        assert "split" not in f
