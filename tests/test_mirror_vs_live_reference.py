"""The host-side mirror (usflows_amd.flows / transforms) next to the REAL reference, method by method, on the same state
dict -- the caller-facing surface SURVEY.md 8b lists (sample shapes, export modes, per-layer log-dets and signs,
feasibility / jitter, simplify, log_prior, device plumbing).  The reference's side of every comparison is a recorded run
of the real reference (tests/golden/live_mirror.npz, tests/golden/make_golden_live.py); recording re-runs it live."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from golden_util import LiveReference, RECORD_LIVE, live_threads, write_recorded_live  # noqa: E402

FIXTURE = "live_mirror"


@pytest.fixture(scope="module", autouse=True)
def _write_recording():
    with live_threads():
        yield
    if RECORD_LIVE:
        write_recorded_live()


@pytest.fixture
def R(request):
    return LiveReference(FIXTURE, request.node.name)


def _reference():
    """(flows, transforms, networks, distributions) of the live reference: recording only"""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import ref_shim
    return ref_shim.install()


def _pair(R, hh=1, conj=True, D=10, K=3, prior_scale=None, soft=False):
    from usflows_amd.flows import USFlow
    from usflows_amd.networks import ConditionalDenseNN
    torch.manual_seed(3)
    args = dict(input_dim=D, context_dim=1, hidden_dims=[12, 12], out_dim=D, nonlinearity=torch.nn.LeakyReLU(0.01))
    prior = torch.distributions.Uniform(1e-20, 0.01) if soft else None
    ref = None
    if R.record:
        flows, _, networks, _ = _reference()
        ref = flows.USFlow(torch.distributions.Laplace(torch.zeros(D), torch.ones(D)), [D], K, networks.ConditionalDenseNN,
                           args, householder=hh, affine_conjugation=conj, prior_scale=prior_scale, soft_training=soft,
                           training_noise_prior=prior)
    mine = USFlow(torch.distributions.Laplace(torch.zeros(D), torch.ones(D)), [D], K, ConditionalDenseNN, dict(args),
                  householder=hh, affine_conjugation=conj, prior_scale=prior_scale, soft_training=soft,
                  training_noise_prior=prior)
    res = mine.load_state_dict(R.state_dict("state_dict", lambda: ref.state_dict()), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return ref, mine


def _val(v):
    return float(v.detach()) if torch.is_tensor(v) else float(v)


def _ref_sign(lr):
    try:
        return lr.sign() if callable(lr.sign) else lr.sign
    except TypeError:
        return None      # the reference's own sign() fails on blocks with a Householder factor (its `sign` is a
        #                  class attribute, transforms.py:760 vs :1455); the mirror returns the product


@pytest.mark.parametrize("hh,conj", [(0, False), (1, True), (2, True)])
def test_layer_protocol_side_by_side(R, hh, conj):
    ref, mine = _pair(R, hh, conj)
    assert R.names("layers", lambda: [type(l).__name__ for l in ref.layers]) == [type(l).__name__ for l in mine.layers]
    x = R.tensor("x", lambda: torch.rand(6, 10))
    with torch.no_grad():
        for i, lm in enumerate(mine.layers):
            lr = ref.layers[i] if ref is not None else None
            name = type(lm).__name__
            yr, ym = R.tensor(f"{i}/forward", lambda: lr.forward(x)), lm.forward(x)
            assert torch.allclose(yr, ym, rtol=1e-5, atol=1e-6), name
            assert torch.allclose(R.tensor(f"{i}/backward", lambda: lr.backward(x)), lm.backward(x), rtol=1e-4, atol=1e-5), name
            assert abs(R.float(f"{i}/ladj", lambda: _val(lr.log_abs_det_jacobian(x, yr))) - _val(lm.log_abs_det_jacobian(x, ym))) < 1e-5
            sr = R.float(f"{i}/sign", lambda: _ref_sign(lr))
            sm = lm.sign() if callable(lm.sign) else lm.sign
            assert sr is None or sr == _val(sm), name
            assert R.flag(f"{i}/is_feasible", lambda: lr.is_feasible()) == bool(lm.is_feasible())
            assert R.float(f"{i}/log_prior", lambda: _val(lr.log_prior())) == pytest.approx(_val(lm.log_prior()), abs=1e-6), name
        assert torch.allclose(R.tensor("log_prob", lambda: ref.log_prob(x)), mine.log_prob(x), rtol=1e-5)
        assert torch.allclose(R.tensor("backward", lambda: ref.backward(x)), mine.backward(x), rtol=1e-4, atol=1e-5)
        assert torch.allclose(R.tensor("_forward", lambda: ref._forward(x)), mine._forward(x), rtol=1e-4, atol=1e-5)


def test_log_prior_and_feasibility_side_by_side(R):
    ref, mine = _pair(R, hh=1, conj=True, prior_scale=0.7)
    assert R.float("log_prior", lambda: _val(ref.log_prior())) == pytest.approx(_val(mine.log_prior()), abs=1e-6)
    assert R.flag("is_feasible", lambda: ref.is_feasible()) and mine.is_feasible()
    flows = [f for f in (ref, mine) if f is not None]
    with torch.no_grad():
        for f in flows:
            f.layers[-2].block_transform.U_raw[2, 2] = 0.0
    # a zero pivot inside a BlockAffineTransform is invisible to Flow.is_feasible -- in the reference and here
    assert R.flag("is_feasible_zero_pivot", lambda: ref.is_feasible()) == mine.is_feasible()
    assert R.flag("block_is_feasible_zero_pivot", lambda: ref.layers[-2].block_transform.is_feasible()) == \
        bool(mine.layers[-2].block_transform.is_feasible()) is False
    with torch.no_grad():
        for f in flows:
            f.layers[-1].scale[0] = 0.0
    assert (not R.flag("is_feasible_zero_scale", lambda: ref.is_feasible())) and (not mine.is_feasible())


def test_export_modes_and_sample_shapes_side_by_side(R):
    ref, mine = _pair(R, hh=0, conj=False)
    x = R.tensor("x", lambda: torch.rand(5, 10))
    with torch.no_grad():
        for mode in ("log_prob", "forward", "backward"):
            if ref is not None:
                ref.export = mode
            mine.export = mode
            assert torch.allclose(R.tensor(f"export/{mode}", lambda: ref(x)), mine(x), rtol=1e-4, atol=1e-5), mode
        for shape in (None, [4], [2, 3]):
            assert R.shape(f"sample/{shape}", lambda: ref.sample(shape).shape) == tuple(mine.sample(shape).shape), shape
    if ref is not None:
        with pytest.raises(Exception):
            ref.export = "nonsense"
            ref(x)
    with pytest.raises(Exception):
        mine.export = "nonsense"
        mine(x)


def test_simplify_side_by_side(R):
    ref, mine = _pair(R, hh=1, conj=True)
    x = R.tensor("x", lambda: torch.rand(7, 10))
    with torch.no_grad():
        sr = ref.simplify() if ref is not None else None
        sm = mine.simplify()
        assert R.names("layers", lambda: [type(l).__name__ for l in sr.layers]) == [type(l).__name__ for l in sm.layers]
        assert torch.allclose(R.tensor("log_prob", lambda: sr.log_prob(x)), sm.log_prob(x), rtol=1e-4)
        assert torch.allclose(sm.log_prob(x), mine.log_prob(x), rtol=1e-4)


def test_soft_training_context_side_by_side(R):
    ref, mine = _pair(R, hh=0, conj=False, soft=True)
    x = R.tensor("x", lambda: torch.rand(5, 10))
    ctx = R.tensor("ctx", lambda: torch.rand(5, 1))
    with torch.no_grad():
        assert torch.allclose(R.tensor("log_prob", lambda: ref.log_prob(x)), mine.log_prob(x), rtol=1e-5)       # implicit zero context
        assert torch.allclose(R.tensor("log_prob_ctx", lambda: ref.log_prob(x, context=ctx)), mine.log_prob(x, context=ctx), rtol=1e-5)


# ---- distributions (distributions.py): the radial base and its parametrised norm distributions ----------------------
@pytest.mark.parametrize("p", [1.0, 2.0, float("inf")])
def test_radial_distribution_side_by_side(R, p):
    from usflows_amd import distributions as mdist
    D = 9
    loc = torch.linspace(-0.3, 0.4, D)
    ref = None
    if R.record:
        rdist = _reference()[3]
        ref = rdist.RadialDistribution(loc.clone(), rdist.LogNormal(torch.tensor([0.8]), torch.tensor([0.4])), p)
    mine = mdist.RadialDistribution(loc.clone(), mdist.LogNormal(torch.tensor([0.8]), torch.tensor([0.4])), p)
    sd = R.state_dict("state_dict", lambda: ref.state_dict())
    assert sorted(sd) == sorted(mine.state_dict())
    mine.load_state_dict(sd)
    x = torch.randn(11, D, generator=torch.Generator().manual_seed(2)) * 2
    r = torch.linspace(0.05, 9.0, 17)
    with torch.no_grad():
        assert torch.allclose(R.tensor("log_prob", lambda: ref.log_prob(x)), mine.log_prob(x), rtol=1e-5, atol=1e-5)
        assert torch.allclose(R.tensor("r_profile", lambda: ref.r_profile(r)), mine.r_profile(r), rtol=1e-5, atol=1e-5)
        assert torch.allclose(R.tensor("log_delta_volume", lambda: ref.log_delta_volume(p, r)), mine.log_delta_volume(p, r), rtol=1e-6)
        for thr in (-25.0, -18.0):
            a = R.tensor(f"udl/{thr}", lambda: ref.radial_udl_profile(threshold=torch.tensor(thr), r_max=40.0, n_samples=4000))
            b = mine.radial_udl_profile(threshold=torch.tensor(thr), r_max=40.0, n_samples=4000)
            assert a.shape == b.shape and torch.allclose(a, b, atol=1e-5), thr
            a = R.tensor(f"ldl/{thr}", lambda: ref.radial_ldl_profile(threshold=torch.tensor(thr), r_max=40.0, n_samples=4000))
            b = mine.radial_ldl_profile(threshold=torch.tensor(thr), r_max=40.0, n_samples=4000)
            assert a.shape == b.shape and torch.allclose(a, b, atol=1e-5), thr
        for shape in (None, [5], [2, 3]):
            assert R.shape(f"sample/{shape}", lambda: ref.sample(shape).shape) == tuple(mine.sample(shape).shape), shape
        assert R.float("unit_ball_log_prob", lambda: float(ref.unit_ball_distribution.log_prob(x[0]))) == pytest.approx(
            float(mine.unit_ball_distribution.log_prob(x[0])), rel=1e-6)


@pytest.mark.parametrize("cls", ["LogNormal", "Laplace", "Normal", "Gamma"])
def test_distribution_modules_side_by_side(R, cls):
    from usflows_amd import distributions as mdist
    a, b = torch.tensor([0.3, 1.1]), torch.tensor([0.6, 1.4])
    ref = getattr(_reference()[3], cls)(a.clone(), b.clone()) if R.record else None
    mine = getattr(mdist, cls)(a.clone(), b.clone())
    sd = R.state_dict("state_dict", lambda: ref.state_dict())
    assert sorted(sd) == sorted(mine.state_dict())
    mine.load_state_dict(sd)
    v = torch.tensor([[0.2, 0.9], [1.7, 2.5]])
    with torch.no_grad():
        assert torch.allclose(R.tensor("log_prob", lambda: ref.log_prob(v)), mine.log_prob(v), rtol=1e-5, atol=1e-6)
        assert R.shape("sample", lambda: ref.sample([4]).shape) == tuple(mine.sample([4]).shape)


# ---- conditioners (networks.py): same state-dict keys, same outputs with and without context ------------------------
def test_conditioners_side_by_side(R):
    from usflows_amd import networks as mnet
    rnet = _reference()[2] if R.record else None
    torch.manual_seed(11)
    act = torch.nn.LeakyReLU(0.01)
    makers = [
        lambda N: N.ConditionalDenseNN(input_dim=9, context_dim=1, hidden_dims=[14, 10], out_dim=9, nonlinearity=act),
        lambda N: N.ConvNet(in_dims=[9], c_hidden=[12, 8], nonlinearity=act, normalize_layers=False, gating=False),
        lambda N: N.ConvNet(in_dims=[9], c_hidden=[12, 8], nonlinearity=act),          # defaults: gated + layer-normalised
    ]
    pairs = [(mk(rnet) if rnet is not None else None, mk(mnet)) for mk in makers]
    x = R.tensor("x", lambda: torch.rand(6, 9))
    ctx = R.tensor("ctx", lambda: torch.rand(6, 1))
    for i, (ref, mine) in enumerate(pairs):
        name = type(mine).__name__
        sd = R.state_dict(f"{i}/state_dict", lambda: ref.state_dict())
        assert sorted(sd) == sorted(mine.state_dict()), name
        mine.load_state_dict(sd)
        with torch.no_grad():
            assert torch.allclose(R.tensor(f"{i}/out", lambda: ref(x)), mine(x), rtol=1e-5, atol=1e-6), name
            if isinstance(mine, mnet.ConditionalDenseNN):
                assert torch.allclose(R.tensor(f"{i}/out_ctx", lambda: ref(x, ctx)), mine(x, ctx), rtol=1e-5, atol=1e-6)


# ---- mixture families (distributions.py:674-707, 730-850) ------------------------------------------
def _mixtures():
    from usflows_amd import distributions as MD
    g = torch.Generator().manual_seed(11)
    k = 6
    cases = {
        "GammaMM": (lambda M: M.GammaMM(torch.rand(k, generator=g.manual_seed(1)) * 5 + 0.5,
                                        torch.rand(k, generator=g.manual_seed(2)) + 0.5,
                                        torch.randn(k, generator=g.manual_seed(3))), (40,)),
        "LogNormalMM": (lambda M: M.LogNormalMM(torch.randn(k, generator=g.manual_seed(4)),
                                                torch.rand(k, generator=g.manual_seed(5)) + 0.3,
                                                torch.randn(k, generator=g.manual_seed(6))), (40,)),
        "WeibullMM": (lambda M: M.WeibullMM(torch.rand(k, generator=g.manual_seed(7)) + 0.5,
                                            torch.rand(k, generator=g.manual_seed(8)) * 2 + 0.5,
                                            torch.randn(k, generator=g.manual_seed(9))), (40,)),
        "GMM": (lambda M: M.GMM(torch.randn(3, 4, generator=g.manual_seed(10)),
                                torch.stack([torch.eye(4) * (1 + i) for i in range(3)]),
                                torch.randn(3, generator=g.manual_seed(12))), (40, 4)),
    }
    return MD, cases


@pytest.mark.parametrize("name", ["GammaMM", "LogNormalMM", "WeibullMM", "GMM"])
def test_mixture_families_side_by_side(R, name):
    MD, cases = _mixtures()
    make, shape = cases[name]
    ref = make(_reference()[3]) if R.record else None
    mine = make(MD)
    assert R.names("parameters", lambda: [k for k, _ in ref.named_parameters()]) == [k for k, _ in mine.named_parameters()]
    res = mine.load_state_dict(R.state_dict("state_dict", lambda: ref.state_dict()), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert R.shape("event_shape", lambda: ref.event_shape) == tuple(mine.event_shape)
    assert R.shape("batch_shape", lambda: ref.batch_shape) == tuple(mine.batch_shape)
    x = torch.rand(shape, generator=torch.Generator().manual_seed(5)) * 3 + 0.05
    assert torch.allclose(R.tensor("log_prob", lambda: ref.log_prob(x)), mine.log_prob(x), rtol=1e-6, atol=1e-7)

    def ref_sample():
        torch.manual_seed(7)
        return ref.sample([9])
    sr = R.tensor("sample", ref_sample)
    torch.manual_seed(7)
    sm = mine.sample([9])
    assert torch.equal(sr, sm)
    # gradients reach every parameter the same way
    if ref is not None:
        (-ref.log_prob(x).mean()).backward()
    (-mine.log_prob(x).mean()).backward()
    for i, (n, pm) in enumerate(mine.named_parameters()):
        pr = dict(ref.named_parameters())[n] if ref is not None else None
        assert R.flag(f"grad/{n}/is_none", lambda: pr.grad is None) == (pm.grad is None), n
        if pm.grad is not None:
            assert torch.allclose(R.tensor(f"grad/{n}", lambda: pr.grad), pm.grad, rtol=1e-5, atol=1e-7), n


def test_radial_distribution_with_gammamm_norm_side_by_side(R):
    """the base distribution of the reference's live configs (gaussian_mixture.yaml:74-93): RadialDistribution(p=1) over a
    GammaMM norm distribution -- log_prob, sampling and the state-dict layout"""
    MD, _ = _mixtures()
    mk = lambda M: M.RadialDistribution(torch.zeros(6), M.GammaMM(torch.linspace(1.0, 4.0, 5), torch.ones(5), torch.ones(5) / 5),
                                        1.0)
    ref = mk(_reference()[3]) if R.record else None
    mine = mk(MD)
    assert set(R.names("state_dict_keys", lambda: list(ref.state_dict()))) == set(mine.state_dict())
    x = torch.randn(30, 6, generator=torch.Generator().manual_seed(2))
    assert torch.allclose(R.tensor("log_prob", lambda: ref.log_prob(x)), mine.log_prob(x), rtol=1e-6, atol=1e-6)
    # (RadialDistribution.sample needs norm samples of shape [n, 1], distributions.py:488-494: with a GammaMM, whose
    # samples are [n], the reference raises -- so does the mirror's host path; Flow.sample's device path reshapes the
    # radii itself and works, tests/test_flow_gpu.py)
    if ref is not None:
        with pytest.raises(RuntimeError):
            ref.sample([12])
    with pytest.raises(RuntimeError):
        mine.sample([12])


@pytest.mark.parametrize("masktype,gating,norm", [("checkerboard", True, True), ("channel", False, False)])
def test_image_shaped_usflow_side_by_side(R, masktype, gating, norm):
    """USFlow(in_dims=[C, H, W]): same layer list, masks (flows.py:494-536), state-dict keys and outputs as
    the live reference -- 1x1-conv BlockAffineTransform (transforms.py:904-962) and ConvNet2D (networks.py:405-510)"""
    from usflows_amd.flows import USFlow
    from usflows_amd.networks import ConvNet2D
    dims = [4, 5, 6]
    args = dict(c_in=4, c_hidden=6, num_layers=2, padding="same", normalize_layers=norm, gating=gating)
    mk = lambda F, N: F(torch.distributions.Laplace(torch.zeros(dims), torch.ones(dims)), dims, 2, N, dict(args),
                        householder=1, affine_conjugation=True, masktype=masktype)
    torch.manual_seed(5)
    ref = None
    if R.record:
        flows, _, networks, _ = _reference()
        ref = mk(flows.USFlow, networks.ConvNet2D)
    mine = mk(USFlow, ConvNet2D)
    sd = R.state_dict("state_dict", lambda: ref.state_dict())
    assert list(sd) == list(mine.state_dict())
    mine.load_state_dict(sd, strict=True)
    assert R.names("layers", lambda: [type(l).__name__ for l in ref.layers]) == [type(l).__name__ for l in mine.layers]
    for i, lm in enumerate(mine.layers):
        lr = ref.layers[i] if ref is not None else None
        if R.flag(f"{i}/has_mask", lambda: hasattr(lr, "mask")):
            assert torch.equal(R.tensor(f"{i}/mask", lambda: lr.mask), lm.mask)
    x = R.tensor("x", lambda: torch.rand(7, *dims))
    with torch.no_grad():
        assert torch.allclose(R.tensor("log_prob", lambda: ref.log_prob(x)), mine.log_prob(x), rtol=1e-6)
        assert torch.allclose(R.tensor("backward", lambda: ref.backward(x)), mine.backward(x), rtol=1e-5, atol=1e-6)
        assert torch.allclose(R.tensor("_forward", lambda: ref._forward(x)), mine._forward(x), rtol=1e-5, atol=1e-6)
        for i, lm in enumerate(mine.layers):
            lr = ref.layers[i] if ref is not None else None
            assert abs(R.float(f"{i}/ladj", lambda: _val(lr.log_abs_det_jacobian(x, x))) - _val(lm.log_abs_det_jacobian(x, x))) < 1e-5

        def ref_sample():
            torch.manual_seed(1)
            return ref.sample([3])
        sr = R.tensor("sample", ref_sample)
        torch.manual_seed(1)
        sm = mine.sample([3])
        assert sr.shape == sm.shape == (3, *dims) and torch.allclose(sr, sm, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("in_dims,c_hidden,kw", [
    ([4, 6, 6], [8, 8], {}), ([3, 10], [6, 9], dict(gating=True)), ([4, 5, 5], [8, 12], dict(gating=False)),
    ([2, 4, 4, 4], [6], dict(normalize_layers=False)), ([4, 6, 6], [8, 8], dict(padding=1, nonlinearity=torch.nn.LeakyReLU(0.1)))])
def test_convnet_spatial_path_side_by_side(R, in_dims, c_hidden, kw):
    """the SPATIAL branch of the reference's ConvNet (networks.py:312-371, 388-403: Conv1d / 2d / 3d, GatedConvND with and
    without the residual projection, LayerNormChannelsND): same module tree, same state-dict keys, same bits on the CPU"""
    from usflows_amd.networks import ConvNet
    torch.manual_seed(0)
    ref = _reference()[2].ConvNet(in_dims, c_hidden, **kw) if R.record else None
    mine = ConvNet(in_dims, c_hidden, **kw)
    sd = R.state_dict("state_dict", lambda: ref.state_dict())
    assert list(sd.keys()) == list(mine.state_dict().keys())
    mine.load_state_dict(sd, strict=True)
    x = R.tensor("x", lambda: torch.randn(5, *in_dims))
    assert torch.equal(R.tensor("out", lambda: ref(x)), mine(x))
    if len(in_dims) == 2:                                   # (L, B, C) inputs are accepted as (B, C, L)
        xl = R.tensor("xl", lambda: torch.randn(in_dims[1], 7, in_dims[0]))
        assert torch.equal(R.tensor("out_l", lambda: ref(xl)), mine(xl))
