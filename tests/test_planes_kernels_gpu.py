"""gemm_planes_kernel and coupling_planes_kernel on a real MI355X, instantiation by instantiation: one launch per case of
tests/planes_kernel_cases.py through the C ABI against fp64, descriptors built by hand from the headers, a NaN with a payload of
its own wherever the launch must not read into a result or write.  Every element of every row < M is held to the project's own
bounds (GEMM: max(4 err32, 6e-8 sqrt(32 nk)); coupling: max(4 err32, 2e-6); relative to max |ref64|, err32 = the same layer in
fp32 on the CPU), every other byte of every buffer is accounted for, a second launch gives the same bits, permuted rows give the
permuted result bit for bit, the inputs are unchanged and the fp16x2 range flag stays down.  Nothing is tuned to the kernels."""
import ctypes as C

import pytest
import torch

import planes_kernel_cases as pk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLANE_BUFFERS = ("A", "Rbuf", "S", "z")          # handed over GUARD bytes in


def _lib():
    from usflows_amd import _ext
    return _ext, _ext.load()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


def _raw(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _gemm_launch(c, p, knob_pairs=()):
    """ONE launch on device copies of the case's buffers: dict(C, S, part, flag) of CPU tensors"""
    ext, lib = _lib()
    host = {name: p[name] for name in pk.GEMM_INPUTS if name in p}
    bufs = {name: t.to(DEV) for name, t in host.items()}
    bufs["C"] = p["C0"].to(DEV)
    if "S0" in p:
        bufs["S"] = p["S0"].to(DEV)
    if "part0" in p:
        bufs["part"] = p["part0"].to(DEV)
    bufs["flag"] = torch.zeros(4, dtype=torch.int32, device=DEV)

    def ptr(name):
        base = bufs[name].data_ptr()
        if name in PLANE_BUFFERS or (name == "C" and c.form != "fp32"):
            return base + pk.GUARD
        return base + 4 * p["c_off"] if name == "C" else base

    d, side = pk.gemm_descriptor(c, ptr, ext.GemmPlanesDesc, p)
    st = torch.cuda.current_stream().cuda_stream
    with pk.knobs(knob_pairs):
        assert lib.usf_gemm_planes_variant(C.byref(d)) == pk.gemm_variant_code(c)
        rc = lib.usf_gemm_planes_side(C.byref(d), *side, st) if side else lib.usf_gemm_planes_bf16x3(C.byref(d), st)
    assert rc == 0, lib.usf_last_error()
    torch.cuda.synchronize()
    for name, t in host.items():
        assert torch.equal(_raw(bufs[name].cpu()), _raw(t)), f"the launch changed its input {name}"
    got = dict(C=bufs["C"].cpu(), flag=int(bufs["flag"].cpu().abs().sum()))
    if "S" in bufs:
        got["S"] = bufs["S"].cpu()
    if "part" in bufs:
        got["part"] = bufs["part"].cpu()
    return got


def _same_buffers(a, b):
    return a.keys() == b.keys() and all(a[k] == b[k] if k == "flag" else torch.equal(_raw(a[k]), _raw(b[k])) for k in a)


@pytest.mark.parametrize("c", pk.GEMM_CASES, ids=pk.gemm_case_id)
def test_gemm_planes_kernel_vs_fp64(c):
    p = pk.gemm_prepared(c)
    if c.kind == "persist":
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert pk.gemm_grid(c)[2] > (cus // 8) * 8, "no persistent block takes a second tile on this part"
    got = _gemm_launch(c, p)
    bad, fig = pk.gemm_check(c, got, p)
    print(f"PK|gemm|{'|'.join(map(str, pk.gemm_instantiation(c)))}|{c.kind}|{fig['err']:.3e}|{fig['err32']:.3e}|{fig['bound']:.3e}")
    assert bad == []
    assert _same_buffers(_gemm_launch(c, p), got), "a second launch gives other bits"
    rows = pk.gemm_rows(c, got, p)
    del got
    # the DEAD form and the full path write the same rows < M (the padding rows of the last panel, NaN here, are "any value": the
    # full path turns their dead slots into NaN, the DEAD form leaves the bias there -- usf_planes.hip says so)
    if c.dead == "negzero":
        twin = c._replace(dead="zero")
        assert pk.gemm_instantiation(twin)[3] == 1 and pk.gemm_instantiation(c)[3] == 0
        tp = pk.gemm_prepared(twin)
        assert _same(pk.gemm_rows(twin, _gemm_launch(twin, tp), tp), rows), "a -0 in the dead rows changes the result"
    if c.kind in ("dead", "scan"):
        assert _same(pk.gemm_rows(c, _gemm_launch(c, p, (("planes_skip_dead", 0),)), p), rows), "planes_skip_dead = 0 gives other bits"
    q = pk.gemm_prepared(c, c.M + 1)
    got_perm = _gemm_launch(c, q)
    assert _same(pk.gemm_rows(c, got_perm, q), [r[..., q["perm"], :] for r in rows]), "rows depend on their position"


def _coupling_launch(c, p, mode=None, knob_pairs=(), side_form=True):
    ext, lib = _lib()
    mode = mode or c.mode
    host = pk.coupling_buffers(c, p, side_form=side_form)
    bufs = {name: t.to(DEV) for name, t in host.items()}
    bufs["flag"] = torch.zeros(4, dtype=torch.int32, device=DEV)

    def ptr(name):
        guarded = name in PLANE_BUFFERS or name.startswith("hout") or name.startswith("gate")
        return bufs[name].data_ptr() + (pk.GUARD if guarded else 0)

    d, entry, extra = pk.coupling_descriptor(c, ptr, ext.CouplingPlanesDesc, p, mode=mode)
    st = torch.cuda.current_stream().cuda_stream
    with pk.knobs(knob_pairs):
        code = lib.usf_coupling_planes_variant(C.byref(d), int("ctx" in mode), int(mode == "side"))
        assert code == pk.coupling_variant_code(c._replace(mode=mode)), lib.usf_last_error()
        rc = getattr(lib, entry)(C.byref(d), *extra, st)
    assert rc == 0, lib.usf_last_error()
    torch.cuda.synchronize()
    for name in pk.coupling_inputs(c):
        if name in bufs:
            assert torch.equal(_raw(bufs[name].cpu()), _raw(host[name])), f"the launch changed its input {name}"
    got = dict(z=bufs["z"].cpu(), flag=int(bufs["flag"].cpu().abs().sum()))
    if mode in ("hout", "hout_ctx", "gate"):
        for l in range(c.nh):
            got[f"hout{l}"] = bufs[f"hout{l}"].cpu()
    return got


@pytest.mark.parametrize("c", pk.COUPLING_CASES, ids=pk.coupling_case_id)
def test_coupling_planes_kernel_vs_fp64(c):
    p = pk.coupling_prepared(c)
    got = _coupling_launch(c, p)
    bad, fig = pk.coupling_check(c, got, p)
    print(f"PK|coupling|{pk.coupling_variant_code(c)}|{c.mode}|{fig['err']:.3e}|{fig['err32']:.3e}|{fig['bound']:.3e}")
    assert bad == []
    assert _same_buffers(_coupling_launch(c, p), got), "a second launch gives other bits"
    off = (("coupling_act_max", 0), ("coupling_descend", 0))
    assert _same_buffers(_coupling_launch(c, p, knob_pairs=off), got), "coupling_act_max = 0 / coupling_descend = 0 give other bits"
    rows = pk.coupling_rows(c, got)
    if c.mode in ("hout", "hout_ctx"):
        # MODE 1 writes the z of MODE 0
        plain = _coupling_launch(c, p, mode="ctx" if c.mode == "hout_ctx" else "plain")
        assert torch.equal(plain["z"], got["z"]) and plain["flag"] == 0, "the training forward's z is not the inference launch's"
    if c.mode == "side":
        # the plain launch on a z whose transformed blocks hold the planes of the side values writes the same rows
        plain = _coupling_launch(c, p, mode="plain", side_form=False)
        assert _same(pk.coupling_rows(c, plain), rows) and plain["flag"] == 0, "the fp32 residual changes the result"
    q = pk.coupling_prepared(c, c.M + 1)
    got_perm = _coupling_launch(c, q)
    assert _same(pk.coupling_rows(c, got_perm), [r[..., q["perm"], :] for r in rows]), "rows depend on their position"
