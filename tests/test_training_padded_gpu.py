"""The device training path at padded feature dims on MI355X (tests/padded_cases.py: where the segment layout LD and the natural
layout LDn differ, D = 2, 3, 10, 34, 100, ...): Flow.log_prob of an input that requires grad -- log_prob row-wise, d/dx and every
parameter gradient -- against autograd through the fp64 oracle, eagerly and from the replayed tape, at batches on both sides of
the path's own thresholds (the tiny-layer coupling kernel: 0 < B <= 256; the single-launch weight gradients: B <=
GRAD_JOB_MAX_ROWS = 256; the fused coupling kernel: B >= fused_min_rows), and the no_grad passes of the same flows."""
import pytest
import torch

from golden_util import load_case
from model_util import build_flow
from oracle import usflows_oracle as orc
from usflows_amd import _ext
from padded_cases import PADDED_GOLDEN, SWEEP_AFFINE, SWEEP_BASES, SWEEP_CONDS, SWEEP_DIMS, Reference, sweep_input, sweep_spec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCHES = [1, 37, 256, 257]
COMBOS = [(c, conj, hh, b) for c in SWEEP_CONDS for conj, hh in SWEEP_AFFINE for b in SWEEP_BASES]    # 8 per D


def _device_log_prob(flow, x):
    """Flow.log_prob on the device training path (asserted: the flow's TrainPath served the call, no composite fallback)"""
    eng = flow.engine()
    before = eng.launch_count
    lp = flow.log_prob(x)
    assert lp.requires_grad and eng.launch_count > before, "the device training path did not run"
    assert flow._train_obj is not None and not getattr(flow, "_train_failed", False), "composite fallback"
    return lp


def _grads_on_device(flow, x0, g_lp):
    for p in flow.parameters():
        p.grad = None
    x = x0.to(DEV).requires_grad_(True)
    lp = _device_log_prob(flow, x)
    (lp * g_lp.to(DEV)).sum().backward()
    return lp.detach(), x.grad


@pytest.mark.parametrize("name", PADDED_GOLDEN)
def test_input_gradient_on_the_device_path_at_padded_dims(name):
    """the padded golden cases (the live flat configuration at D = 2, 10, 100 among them): d log_prob / dx within
    max(2e-5, 3 x the fp32 oracle's error) of its scale, log_prob row-wise, every parameter gradient; eager, then replayed"""
    spec, sd, a = load_case(name)
    flow = build_flow(spec, sd, device=DEV)
    eng = flow.engine()
    x0 = a["x"]
    g_lp = torch.randn(x0.shape[0], generator=torch.Generator().manual_seed(2))
    ref = Reference(spec, sd, x0, g_lp)
    for run in ("eager", "replayed"):
        lp, gx = _grads_on_device(flow, x0, g_lp)
        ref.check_log_prob(lp)
        ref.check_input_grad(gx, (name, run))
        assert ref.check_param_grads(flow, (name, run)) >= 5
    assert eng.LD > eng.LDn, (eng.LD, eng.LDn)


_flows = {}


def _sweep_flow(D, combo, hidden=None):
    key = (D, combo, None if hidden is None else tuple(hidden))
    if key not in _flows:
        spec, sd = sweep_spec(D, *combo)
        if hidden is not None:
            spec.hidden_dims = list(hidden)
            sd = orc.synth_state_dict(spec, seed=11 + D)
            if "base_distribution.loc" in sd:
                spec.base_loc = sd["base_distribution.loc"]
        _flows[key] = (spec, sd, build_flow(spec, sd, device=DEV))
    return _flows[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_flows():
    yield
    _flows.clear()


def _check_no_grad_passes(flow, spec, sd, x0, ref):
    """log_prob / backward / _forward of the same flow and batch without autograd (the inference plans of the same workspace)"""
    sd64 = orc.to_dtype(sd, torch.float64)
    with torch.no_grad():
        lp = flow.log_prob(x0.to(DEV))
        z = flow.backward(x0.to(DEV))
        z_ref = orc.flow_backward(sd64, spec, x0.double())
        xf = flow._forward(z_ref.float().to(DEV))
        xs = flow.sample([x0.shape[0]], seed=3)
    ref.check_log_prob(lp)
    s = max(1.0, z_ref.abs().max().item())
    assert (z.cpu().double() - z_ref).abs().max().item() < 2e-5 * s, "backward"
    x_ref = orc.flow_forward(sd64, spec, z_ref.float().double())
    s = max(1.0, x_ref.abs().max().item())
    assert (xf.cpu().double() - x_ref).abs().max().item() < 2e-5 * s, "_forward"
    assert xs.shape == x0.shape and torch.isfinite(xs).all(), "sample"


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("D", SWEEP_DIMS)
def test_device_training_path_at_padded_dims(D, B):
    """every (conditioner, affine form, base) combination once per D, two per batch size: log_prob, d/dx and every parameter
    gradient eagerly and from the replayed tape, then the no_grad log_prob / backward / _forward / sample of the same flow"""
    i = BATCHES.index(B)
    for combo in (COMBOS[2 * i], COMBOS[2 * i + 1]):
        spec, sd, flow = _sweep_flow(D, combo)
        x0, g_lp = sweep_input(spec, sd, B)
        ref = Reference(spec, sd, x0, g_lp)
        for run in ("eager", "replayed"):
            lp, gx = _grads_on_device(flow, x0, g_lp)
            ref.check_log_prob(lp)
            ref.check_input_grad(gx, (combo, run))
            ref.check_param_grads(flow, (combo, run))
        _check_no_grad_passes(flow, spec, sd, x0, ref)


def test_device_training_path_at_a_padded_dim_on_the_fused_coupling():
    """B >= fused_min_rows at D = 34 (LD 40 > LDn 36) with a conditioner of 192 hidden units: the fused bf16x3 coupling kernel in
    the forward pass, the input gradient written at row stride LDn inside the wider gradient buffer"""
    combo = ("DenseNN", True, 1, "laplace")
    spec, sd, flow = _sweep_flow(34, combo, hidden=[192, 192])
    eng = flow.engine()
    assert eng.LD > eng.LDn
    B = eng.fused_min_rows
    x0, g_lp = sweep_input(spec, sd, B)
    ref = Reference(spec, sd, x0, g_lp)
    lp, gx = _grads_on_device(flow, x0, g_lp)
    fused = [p["arr"][m["op"]].kind == _ext.OP_COUPLING and not m.get("tiny")
             for p in eng._plans.values() if p.get("meta") and p["ws"]["zA"].shape[0] == B for m in p["meta"] if m["kind"] == "coupling"]
    assert fused and all(fused), "the training plan did not run its couplings on the fused kernel"
    ref.check_log_prob(lp)
    ref.check_input_grad(gx, combo, kink_rows=max(2, B // 1000))
    assert ref.check_param_grads(flow, combo, kink_frac=1e-3) >= 5
