"""usflows_amd/optim.py on the MI355X: usf_adam_step_f32 against torch's Adam (fp64 as the truth, torch's own CPU fp32 run
as the yardstick of what fp32 can give) and against the fp32 emulator, the step captured as a graph and replayed (the
device step counter), the clip kernels, and Flow.fit replaying its step with Adam and with a gradient clip.

Tolerances.  Per tensor, ``dist(a, b) = max |a - b|``.  A device result passes when, element by element,
|device - fp64| <= 2 * dist(torch CPU fp32, fp64) + 2e-6 |fp64| + 2.5e-7 max |fp64| -- the last two terms are the floor of
tests/test_sophia.py (an ATen kernel may or may not contract a * b + c).  Device against emulator: that floor alone."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import emulator_optim as emu  # noqa: E402
from golden_util import load_case  # noqa: E402
from model_util import build_flow  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 3, 255, 256, 257, 16383, 16384, 16385, 2 * 16384 + 1]
STEPS = 12
G1 = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1)
G2 = dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.0)
VARIANTS = {
    "adam": (torch.optim.Adam, dict()),
    "adamw_amsgrad_maximize": (torch.optim.AdamW, dict(amsgrad=True, maximize=True)),
}


def _floor(ref):
    return 2e-6 * ref.abs() + 2.5e-7 * ref.abs().max()


# ---- one set of inputs, shared ----------------------------------------------------------------------------------------
def _inputs():
    g = torch.Generator().manual_seed(42)
    init = [torch.randn(n, generator=g) for n in SIZES]
    init.append(torch.randn(40, generator=g))          # index -3: no gradient during the first two steps
    init.append(torch.randn(9, 4, generator=g))        # index -2: used transposed (a non-contiguous leaf)
    init.append(torch.randn(300, generator=g))         # index -1: the second group
    scale = [10.0 ** (torch.rand(x.shape, generator=g) * 4.0 - 3.0) for x in init]
    grads = [[torch.randn(x.shape, generator=g) * s for x, s in zip(init, scale)] for _ in range(STEPS)]
    return init, grads


INIT, GRADS = _inputs()
LATE, NONCONTIG = len(SIZES), len(SIZES) + 1


def _run_torch(variant, device, dtype, ours=False):
    """STEPS steps; returns (per tensor dict of p / exp_avg / exp_avg_sq / max_exp_avg_sq, per tensor host step, optimiser)"""
    cls, extra = VARIANTS[variant]
    if ours:
        from usflows_amd import optim
        cls = optim.AdamW if cls is torch.optim.AdamW else optim.Adam
    ps = []
    for i, x in enumerate(INIT):
        t = x.clone().to(dtype).to(device)
        ps.append(torch.nn.Parameter(t.t() if i == NONCONTIG else t))
    opt = cls([dict(params=ps[:-1], **G1), dict(params=ps[-1:], **G2)], **extra)
    for s in range(STEPS):
        for i, p in enumerate(ps):
            gr = GRADS[s][i].to(dtype).to(device)
            p.grad = None if (i == LATE and s < 2) else (gr.t() if i == NONCONTIG else gr)
        opt.step()
    out = []
    for p in ps:
        st = opt.state[p]
        out.append({k: v.detach().cpu() for k, v in [("p", p)] + [(k, st[k]) for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq") if k in st]})
    return out, [float(opt.state[p]["step"]) for p in ps], opt


_REF = {}


def _refs(variant):
    """torch on the CPU in fp64 and fp32, computed once per variant"""
    if variant not in _REF:
        _REF[variant] = (_run_torch(variant, "cpu", torch.float64), _run_torch(variant, "cpu", torch.float32))
    return _REF[variant]


def _check_against_torch(got, variant, what):
    (r64, steps64, _), (r32, _, _) = _refs(variant)
    out, steps, _ = got
    assert steps == steps64, (steps, steps64)
    for i, (d, a, b) in enumerate(zip(out, r64, r32)):
        assert set(d) == set(a)
        for k in a:
            ref = a[k].double()
            d_cpu = (b[k].double() - ref).abs().max().item()
            err = (d[k].double() - ref).abs()
            ok = err <= 2 * d_cpu + _floor(ref)
            print(f"{what} tensor {i} {k}: device - fp64 {err.max().item():.3e}, torch fp32 - fp64 {d_cpu:.3e}")
            assert bool(ok.all()), (what, i, k, err.max().item(), d_cpu)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_kernel_against_torch(variant):
    got = _run_torch(variant, DEV, torch.float32, ours=True)
    opt = got[2]
    assert opt._tables and set(opt._tables) == {0, 1}, "usf_adam_step_f32 did not run"
    assert sorted(opt._tables[0][3].cpu().tolist()) == [STEPS - 2, STEPS]      # the late parameter counts in a slot of its own
    _check_against_torch(got, variant, variant)


def test_parameters_with_different_step_counts_get_separate_counters():
    from usflows_amd import optim
    ps = [torch.nn.Parameter(torch.ones(5, device=DEV)), torch.nn.Parameter(torch.ones(7, device=DEV))]
    opt = optim.Adam(ps, lr=1e-2)
    ps[0].grad = torch.ones(5, device=DEV)
    opt.step()
    ps[1].grad = torch.ones(7, device=DEV)
    opt.step()
    assert opt._tables[0][3].cpu().tolist() == [2, 1]
    assert [float(opt.state[p]["step"]) for p in ps] == [2.0, 1.0]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_kernel_against_the_emulator(variant):
    cls, extra = VARIANTS[variant]
    out, _, _ = _run_torch(variant, DEV, torch.float32, ours=True)
    for i, x in enumerate(INIT):
        if i == NONCONTIG:
            continue                                   # (torch's arithmetic on the device, not the kernel)
        hp = G2 if i == len(INIT) - 1 else G1
        p = x.clone()
        m, v, vmax = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
        t = 0
        for s in range(STEPS):
            if i == LATE and s < 2:
                continue
            t += 1
            emu.adam_step(p, GRADS[s][i], m, v, vmax, t, lr=hp["lr"], betas=hp["betas"], eps=hp["eps"],
                          weight_decay=hp["weight_decay"], maximize=extra.get("maximize", False),
                          amsgrad=extra.get("amsgrad", False), decoupled=cls is torch.optim.AdamW)
        want = dict(p=p, exp_avg=m, exp_avg_sq=v)
        if extra.get("amsgrad"):
            want["max_exp_avg_sq"] = vmax
        for k, ref in want.items():
            err = (out[i][k].double() - ref.double()).abs()
            assert bool((err <= _floor(ref.double())).all()), (i, k, err.max().item())


def test_a_replayed_step_advances_the_bias_corrections():
    """Three eager steps, ONE step() captured with the deferred-upload protocol of Flow.fit, eight replays: torch's eleven
    steps.  With betas (0.5, 0.9), 1 - beta2^4 = 0.34 against 1 - beta2^11 = 0.69: a step count frozen into the capture
    is far outside the tolerance."""
    from usflows_amd import optim
    kw = dict(lr=1e-2, betas=(0.5, 0.9), weight_decay=0.1)
    g = torch.Generator().manual_seed(9)
    init = [torch.randn(n, generator=g) for n in (257, 16385)]
    grads = [torch.randn(n, generator=g) for n in (257, 16385)]

    def cpu(dtype):
        ps = [torch.nn.Parameter(x.clone().to(dtype)) for x in init]
        o = torch.optim.Adam(ps, **kw)
        for _ in range(11):
            for p, gr in zip(ps, grads):
                p.grad = gr.clone().to(dtype)
            o.step()
        return ps, o

    (p64, o64), (p32, o32) = cpu(torch.float64), cpu(torch.float32)
    ps = [torch.nn.Parameter(x.clone().to(DEV)) for x in init]
    opt = optim.Adam(ps, **kw)
    for p, gr in zip(ps, grads):
        p.grad = gr.clone().to(DEV)
    for _ in range(3):
        opt.step()
    for p in ps:
        p.grad = p.grad.clone()                # new addresses: the table is rebuilt INSIDE the capture, its upload deferred
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    opt.defer_uploads(True)
    try:
        with torch.cuda.graph(graph):
            opt.step()
    finally:
        opt.defer_uploads(False)
    opt.flush_uploads()
    assert [float(opt.state[p]["step"]) for p in ps] == [3.0, 3.0]          # a capture runs nothing
    for _ in range(8):
        graph.replay()
        opt.note_graph_replays(1)
    torch.cuda.synchronize()
    sd = opt.state_dict()
    assert [float(s["step"]) for s in sd["state"].values()] == [11.0, 11.0]
    assert opt._tables[0][3].cpu().tolist() == [11]
    for i, p in enumerate(ps):
        for k, got, r64, r32 in [("p", p, p64[i], p32[i])] + [(k, opt.state[p][k], o64.state[p64[i]][k], o32.state[p32[i]][k])
                                                              for k in ("exp_avg", "exp_avg_sq")]:
            ref = r64.detach().double()
            d_cpu = (r32.detach().double() - ref).abs().max().item()
            err = (got.detach().cpu().double() - ref).abs()
            assert bool((err <= 2 * d_cpu + _floor(ref)).all()), (i, k, err.max().item(), d_cpu)


# ---- the clip kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["below", "above", "zero", "nan"])
def test_clip_kernels_against_the_fp64_formula(case):
    from usflows_amd import optim
    g = torch.Generator().manual_seed(13)
    grads = [torch.randn(n, generator=g) for n in SIZES]
    max_norm = 1e6 if case == "below" else 1.0
    if case == "zero":
        grads = [torch.zeros_like(x) for x in grads]
    if case == "nan":
        grads[4][7] = float("nan")
    ps = [torch.nn.Parameter(torch.zeros_like(x).to(DEV)) for x in grads]
    ps.append(torch.nn.Parameter(torch.zeros(3, device=DEV)))           # no gradient: not part of the norm
    for p, x in zip(ps, grads):
        p.grad = x.clone().to(DEV)
    clip = optim.GradClip(ps, max_norm)
    clip()
    torch.cuda.synchronize()
    assert clip._tables, "the clip kernels did not run"
    total = sum((x.double() ** 2).sum() for x in grads)
    coef = min(max_norm / (float(total.sqrt()) + 1e-6), 1.0) if case != "nan" else float("nan")
    for p, x in zip(ps, grads):
        got = p.grad.cpu()
        if case in ("below", "zero"):
            assert torch.equal(got, x)
        elif case == "nan":
            assert bool(torch.isnan(got).all())
        else:
            ref = x.double() * coef
            assert bool(((got.double() - ref).abs() <= 2.0 ** -22 * ref.abs()).all())
    # and the emulator states the same arithmetic: the same fp64 sums in the same order; the coefficient may still round
    # to the neighbouring fp32 value where the device's fp64 sqrt / division differ from the host's in the last bit, which
    # moves a product by at most one unit in its last place (2^-23 relative)
    if case == "above":
        e = [x.clone() for x in grads]
        emu.clip_grad_norm(e, max_norm)
        for p, x in zip(ps, e):
            assert bool(((p.grad.cpu().double() - x.double()).abs() <= 2.0 ** -23 * x.double().abs()).all())


# ---- Flow.fit ---------------------------------------------------------------------------------------------------------
FIT_STEPS, FIT_LR = 12, 1e-3


def _fit_pair(make_flow, data, optim, optim_params, clip=None):
    """the same fit replayed and eager (use_train_graph False); no RuntimeWarning (a failed capture) in either"""
    ds = torch.utils.data.TensorDataset(data, torch.zeros(data.shape[0]))
    res = []
    for graph in (True, False):
        flow = make_flow()
        flow.use_train_graph = graph
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            losses = flow.fit(ds, optim=optim, optim_params=optim_params, batch_size=32, shuffle=False, gradient_clip=clip,
                              device=torch.device(DEV), epochs=FIT_STEPS // 4)
        res.append((flow, losses))
    return res


def _check_pair(res, lr):
    """tests/test_gm_live.py's replayed-against-eager criterion: losses to 2e-4; parameters to its bound for optimisers that
    move an entry by up to lr per step whatever the gradient's size (two runs are then at most 2 lr apart per step: there
    12.1e-3 = 2 * 1e-3 * 6 steps * 1.01, here 2 * lr * 12 steps * 1.01), and at most 2 % of a large tensor's entries off"""
    (fg, lg), (fe, le) = res
    st = fg.__dict__.get("_train_graph_state")
    assert st is not None and st["graph"] is not None and st["replays"] > 0, (st and st.get("replays"))
    assert not getattr(fg, "_train_graph_failed", False)
    assert "_train_graph_state" not in fe.__dict__
    for a, b in zip(lg, le):
        assert abs(a - b) < 2e-4 * abs(b), (lg, le)
    for (k, a), (_, b) in zip(fg.state_dict().items(), fe.state_dict().items()):
        d = (a.double() - b.double()).abs()
        s = max(b.abs().max().item(), 1e-3)
        assert d.max().item() <= 2 * lr * FIT_STEPS * 1.01 + 2e-3 * s, (k, d.max().item())
        if d.numel() >= 256:
            assert (d > 1e-4 * s + 1e-6).double().mean().item() < 0.02, k
    return st


def _flat_flow():
    spec, sd, _ = load_case("synth_d16_k3_densenn_relu")
    return build_flow(spec, sd, device=DEV)


FLAT_DATA = torch.rand(32 * FIT_STEPS // 3, 16, generator=torch.Generator().manual_seed(0))       # 4 batches x 3 epochs


def test_fit_replays_the_step_with_torch_adam():
    res = _fit_pair(_flat_flow, FLAT_DATA, torch.optim.Adam, dict(lr=FIT_LR, weight_decay=0.1))
    st = _check_pair(res, FIT_LR)
    from usflows_amd import optim
    assert type(st["optim"]) is optim.Adam
    steps = {float(s["step"]) for s in st["optim"].state.values()}
    assert steps == {float(FIT_STEPS)}, steps


def test_fit_replays_the_step_with_sophiag_and_a_gradient_clip():
    from usflows_amd.sophia import SophiaG
    res = _fit_pair(_flat_flow, FLAT_DATA, SophiaG, dict(lr=FIT_LR), clip=0.5)
    st = _check_pair(res, FIT_LR)
    assert st["clip"] is not None and st["clip"]._tables, "the clip kernels did not run inside the replayed step"


def test_fit_replays_the_step_of_an_image_flow_with_adam():
    """the small image flow of smoke(): its gradients are allocated inside the capture, the tables uploaded after it"""
    from usflows_amd.flows import USFlow
    from usflows_amd.networks import ConvNet2D
    import usflows_amd.transforms as T
    dims, cond = [16, 7, 7], dict(c_in=16, c_hidden=32, num_layers=1, padding="same", kernel_size=3, normalize_layers=True, gating=True)

    def make():
        torch.manual_seed(7)
        base = torch.distributions.Laplace(torch.zeros(dims, device=DEV), torch.ones(dims, device=DEV))
        f = USFlow(base, dims, 2, ConvNet2D, dict(cond), householder=1, affine_conjugation=True)
        g = torch.Generator().manual_seed(4)
        with torch.no_grad():       # (a tame start, as tests/test_image_flows.py: the default initialisation is ill-conditioned)
            for m in f.modules():
                if isinstance(m, T.LUTransform):
                    d = m.dim
                    m.L_raw.copy_(torch.eye(d) + 0.1 * torch.randn(d, d, generator=g).tril(-1))
                    m.U_raw.copy_(torch.diag(0.75 + 0.5 * torch.rand(d, generator=g)) + 0.1 * torch.randn(d, d, generator=g).triu(1))
                elif isinstance(m, T.ScaleTransform):
                    m.scale.fill_(1.0)
        return f.to(DEV)

    data = torch.rand(32 * FIT_STEPS // 3, *dims, generator=torch.Generator().manual_seed(1))
    res = _fit_pair(make, data, torch.optim.Adam, dict(lr=FIT_LR, weight_decay=0.1))
    _check_pair(res, FIT_LR)
