"""Conditional image-shaped flows on the CPU: the mirror's CondConvNet2D / CondConvNet (reference networks.py:513-680)
against the REAL reference's fp64 outputs (tests/golden/cond/*.npz), the context forms the reference broadcasts, and the
flat engine's refusal of a vector CondConvNet."""
import pytest
import torch

from cond_image_cases import cond_case_names, default_double, load_cond_case, run_layers


def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max()).item()


@pytest.mark.parametrize("name", cond_case_names())
def test_cond_image_mirror_matches_reference_fp64(name):
    flow, a = load_cond_case(name, dtype=torch.float64)
    x, zin, ctx = a["x"].double(), a["zin"].double(), a["ctx"].double()
    with torch.no_grad(), default_double():
        assert _rel(flow.log_prob(x, ctx), a["log_prob64_ctx"]) <= 1e-10
        assert _rel(flow.log_prob(x), a["log_prob64_noctx"]) <= 1e-10          # the implicit zero context (flows.py:559-565)
        assert _rel(run_layers(flow, x, ctx, True), a["backward64_ctx"]) <= 1e-10
        assert _rel(run_layers(flow, x, torch.zeros(x.shape[0], 1, dtype=torch.float64), True), a["backward64_noctx"]) <= 1e-10
        assert _rel(run_layers(flow, zin, ctx, False), a["forward64_ctx"]) <= 1e-10
    # the fp32 mirror against the reference's own fp32 run
    f32, _ = load_cond_case(name)
    with torch.no_grad():
        assert _rel(f32.log_prob(a["x"], a["ctx"]), a["log_prob32_ctx"]) <= 1e-5
        assert _rel(f32.log_prob(a["x"]), a["log_prob32_noctx"]) <= 1e-5


@pytest.mark.parametrize("name", cond_case_names(with_grads=True))
def test_cond_image_mirror_parameters_and_gradients_key_for_key(name):
    flow, a = load_cond_case(name, dtype=torch.float64)
    named = dict(flow.named_parameters())
    gkeys = {k[2:] for k in a if k.startswith("g/")}
    assert gkeys <= set(named), sorted(gkeys - set(named))[:6]    # (parameters without a gradient in the reference: no entry)
    first = [m for n_, m in flow.named_modules() if n_.endswith("conditioner.nn.0")]
    C = flow.in_dims[0]
    assert first and all(m.in_channels == C + 1 for m in first)   # nn.0 is Conv2d(c_in + 1, c_hidden)
    with default_double():
        loss = -flow.log_prob(a["x"].double(), a["ctx"].double()).mean()
        loss.backward()
    assert abs(loss.item() - a["loss64"].item()) <= 1e-10 * abs(a["loss64"].item())
    for k, p in named.items():
        if k not in gkeys:
            assert p.grad is None or not p.grad.any(), k
            continue
        g = a["g/" + k].double()
        assert (p.grad - g).abs().max().item() <= 1e-6 * max(g.abs().max().item(), 1e-12), k


def test_cond_convnet2d_context_forms():
    from usflows_amd.networks import CondConvNet2D, CondConvNet
    torch.manual_seed(3)
    net = CondConvNet2D(4, 8, num_layers=1, padding="same").double()
    x = torch.rand(5, 4, 6, 6, dtype=torch.float64)
    c = torch.rand(5, dtype=torch.float64)
    plane = lambda v: v.reshape(-1, 1, 1, 1).expand(5, 1, 6, 6)          # noqa: E731
    ref = net.nn(torch.cat([x, plane(c)], 1))
    assert torch.equal(net(x, c), ref) and torch.equal(net(x, c.reshape(5, 1)), ref)
    assert torch.equal(net(x, 0.25), net.nn(torch.cat([x, torch.full((5, 1, 6, 6), 0.25, dtype=torch.float64)], 1)))
    assert torch.equal(net(x, torch.tensor(0.25, dtype=torch.float64)), net(x, 0.25))
    assert torch.equal(net(x), net.nn(torch.cat([x, torch.zeros(5, 1, 6, 6, dtype=torch.float64)], 1)))
    assert net(x).shape == x.shape                                       # c_out defaults to c_in
    with pytest.raises(TypeError):
        CondConvNet2D(16, 32, num_layers=1, rescale_hidden=1)           # as the reference's ConvNet2D (mnist_usflow_minimal.yaml:61)
    sp = CondConvNet([4, 6, 6], [8], c_out=4).double()
    assert torch.equal(sp(x, c), sp.nn(torch.cat([x, plane(c)], 1)))
    # a context that does not expand becomes a zero channel (networks.py:585-588)
    assert torch.equal(sp(x, torch.rand(3, 2, dtype=torch.float64)), sp.nn(torch.cat([x, torch.zeros(5, 1, 6, 6, dtype=torch.float64)], 1)))


def test_vector_cond_convnet_is_not_a_flat_engine_conditioner():
    from usflows_amd.engine import conditioner_supported
    from usflows_amd.networks import CondConvNet, ConvNet
    v = CondConvNet([8], [16, 16], gating=False, normalize_layers=False)
    assert not conditioner_supported(v)
    assert conditioner_supported(ConvNet([8], [16, 16], gating=False, normalize_layers=False))
    assert v.nn[0].in_features == 9
    x, c = torch.rand(4, 8), torch.rand(4, 1)
    assert torch.equal(v(x, c), v.nn(torch.cat([x, c], 1)))
