"""Seeded radial sampling on the device: usf_radial_sample_norm_f32 (radii from the norm distribution and directions on the unit
Lp sphere in one launch) against the numpy emulator of its radius draw, row by row, and against the unfused direction kernel,
bit for bit; ``Flow.sample`` of flat and image-shaped flows with a radial base as a pure function of (seed, row)."""
import math

import numpy as np
import pytest
import torch

import emulator_radial_sample as emu
from radial_sample_cases import CASE_NAMES, M_DRAW, SEED, cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG_OFFSET = 2 ** 33 + 5
KIND_ID = {"lognormal": 0, "gamma": 1, "weibull": 2, "halfnormal": 3, "chi": 4}


def _ext():
    from usflows_amd import _ext as e
    e.load()
    return e


def _softplus64(s):
    return np.where(s > 20.0, s, np.log1p(np.exp(np.minimum(s, 20.0))))


def _inv_softplus32(v):
    """the stored fp32 parameter whose softplus is (about) v"""
    return np.where(v > 20.0, v, np.log(np.expm1(np.minimum(v, 20.0)))).astype(np.float32)


def _stored(name, variant):
    """(norm id, K, par_a, par_b, logits) as device tensors, and the constrained fp64 values the kernel derives from them"""
    ext = _ext()
    kind, a, b, l = cases()[name]
    soft_a = variant == "softplus" and kind in ("gamma", "weibull", "halfnormal")
    soft_b = variant == "softplus" and kind in ("lognormal", "gamma", "weibull")
    sa = _inv_softplus32(a) if soft_a else a.astype(np.float32)
    ca = _softplus64(sa.astype(np.float64)) if soft_a else sa.astype(np.float64)
    sb = cb = None
    if b is not None:
        sb = _inv_softplus32(b) if soft_b else b.astype(np.float32)
        cb = _softplus64(sb.astype(np.float64)) if soft_b else sb.astype(np.float64)
    norm = KIND_ID[kind] | (0 if variant == "softplus" else ext.NORM_RAW_PARAMS)
    t = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(DEV)
    return (norm, len(a), t(sa), t(sb), t(l)), (kind, ca, cb, l)


_REF = {}


def _emulated(name, variant, M, row_offset):
    key = (name, variant, M, row_offset)
    if key not in _REF:
        _, (kind, ca, cb, l) = _stored(name, variant)
        _REF[key] = emu.radii(kind, ca, cb, l, M=M, seed=SEED, offset=0, row_offset=row_offset)
    return _REF[key]


def _variants(name):
    return ["raw"] if cases()[name][0] == "chi" else ["raw", "softplus"]       # (USF_NORM_CHI: raw only)


# ---- the radii against the emulator ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,row_offset", [(M_DRAW, 0), (1027, BIG_OFFSET)])
@pytest.mark.parametrize("name,variant", [(n, v) for n in CASE_NAMES for v in _variants(n)])
def test_radii_match_the_emulator_row_by_row(name, variant, M, row_offset):
    ext = _ext()
    (norm, K, a, b, l), _ = _stored(name, variant)
    r = torch.zeros(M, device=DEV)
    ext.radial_sample_norm(None, 0, M, 0, 0, None, norm, K, a, b, l, r, SEED, 0, row_offset)
    h = M // 2
    r2 = torch.zeros(M, device=DEV)
    ext.radial_sample_norm(None, 0, h, 0, 0, None, norm, K, a, b, l, r2[:h], SEED, 0, row_offset)
    ext.radial_sample_norm(None, 0, M - h, 0, 0, None, norm, K, a, b, l, r2[h:], SEED, 0, row_offset + h)
    assert torch.equal(r, r2)                                   # the launch split does not matter, bit for bit
    got = r.cpu().numpy().astype(np.float64)
    ref = _emulated(name, variant, M, row_offset).astype(np.float64)
    rel = np.abs(got - ref) / ref
    print(f"{name}/{variant} M={M}: max rel {rel.max():.3e}")
    assert np.isfinite(got).all() and (got > 0).all()
    assert rel.max() < 2.5e-7, (int(rel.argmax()), got[rel.argmax()], ref[rel.argmax()])


# ---- fused against unfused ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,p_id", [(1.0, 2), (2.0, 3), (math.inf, 4)])
@pytest.mark.parametrize("D", [7, 64, 784])
@pytest.mark.parametrize("name", ["lognormal", "gamma_x20", "gamma_x64"])
def test_fused_draw_is_the_unfused_direction_kernel_on_its_own_radii(name, D, p, p_id):
    ext = _ext()
    (norm, K, a, b, l), _ = _stored(name, "softplus")
    assert K == {"lognormal": 1, "gamma_x20": 20, "gamma_x64": 64}[name]
    M, ldz = 1027, D + 3
    loc = torch.randn(D, generator=torch.Generator().manual_seed(D)).to(DEV)
    z = torch.full((M, ldz), 7.0, device=DEV)
    r = torch.zeros(M, device=DEV)
    ext.radial_sample_norm(z, ldz, M, D, p_id, loc, norm, K, a, b, l, r, SEED, 5, 77)
    z2 = torch.full((M, ldz), 7.0, device=DEV)
    ext.radial_sample(z2, ldz, M, D, p_id, loc, r, SEED, 5, 77)
    assert torch.equal(z, z2)
    assert (z[:, D:] == 7.0).all()                              # padding columns untouched
    r_only = torch.zeros(M, device=DEV)
    ext.radial_sample_norm(None, 0, M, 0, 0, None, norm, K, a, b, l, r_only, SEED, 5, 77)
    assert torch.equal(r, r_only)                               # the radii do not depend on the direction half
    # the Lp radius of every row is the radius drawn.  Measured on a draw around loc = 0 (same radii: they do not depend on
    # loc): the mixtures reach radii of 1e-3, where fl(loc + r u) around a loc of order 1 keeps no more than two digits of
    # r u -- a property of fp32 storage, not of the draw
    zero = torch.zeros(D, device=DEV)
    z0 = torch.full((M, ldz), 7.0, device=DEV)
    r0 = torch.zeros(M, device=DEV)
    ext.radial_sample_norm(z0, ldz, M, D, p_id, zero, norm, K, a, b, l, r0, SEED, 5, 77)
    assert torch.equal(r0, r)
    u = z0[:, :D].double().cpu()
    rr = r.double().cpu()
    nrm = u.abs().sum(1) if p == 1.0 else (u.pow(2).sum(1).sqrt() if p == 2.0 else u.abs().max(1).values)
    assert ((nrm - rr).abs() / rr).max().item() < 1e-5


# ---- error returns -----------------------------------------------------------------------------------------------------------------
def test_error_returns_launch_nothing():
    ext = _ext()
    (norm, K, a, b, l), _ = _stored("gamma_x64", "raw")
    r = torch.full((8,), -1.0, device=DEV)
    z = torch.full((8, 4), -1.0, device=DEV)
    loc = torch.zeros(4, device=DEV)
    a65, l65 = torch.ones(65, device=DEV), torch.zeros(65, device=DEV)
    with pytest.raises(RuntimeError, match="K = 65"):
        ext.radial_sample_norm(None, 0, 8, 0, 0, None, norm, 65, a65, a65, l65, r, 1, 0, 0)
    with pytest.raises(RuntimeError, match="null pointer"):
        ext.radial_sample_norm(None, 0, 8, 0, 0, None, norm, K, a, b, l, None, 1, 0, 0)
    with pytest.raises(RuntimeError, match="not an Lp-radial id"):
        ext.radial_sample_norm(z, 4, 8, 4, 1, loc, norm, K, a, b, l, r, 1, 0, 0)
    torch.cuda.synchronize()
    assert (r == -1.0).all() and (z == -1.0).all()


# ---- flat flows --------------------------------------------------------------------------------------------------------------------
def _lp_norm(u, p):
    u = u.flatten(1)
    return u.abs().sum(1) if p == 1.0 else (u.pow(2).sum(1).sqrt() if p == 2.0 else u.abs().max(1).values)


@pytest.fixture(scope="module", params=["synth_d16_k3_hh1_radial2", "synth_d16_k3_hh0_conj_radial1_gammamm", "synth_d16_k3_hh0_radialinf"])
def flat(request):
    from golden_util import load_case
    from model_util import build_flow
    from usflows_amd import radial
    spec, sd, _ = load_case(request.param)
    flow = build_flow(spec, sd, device=DEV)
    with torch.no_grad():
        x = flow.sample([2000], seed=11)
        z, r = radial.sample(flow.base_distribution, 2000, 11, want_r=True)
    return flow, x, z, r


def test_flat_sample_is_a_function_of_the_seed(flat):
    flow, x, z, r = flat
    with torch.no_grad():
        assert torch.equal(flow.sample([2000], seed=11), x)
        assert not torch.equal(flow.sample([2000], seed=12), x)
        assert torch.equal(x, flow._forward(z))
    assert x.shape == (2000, 16) and torch.isfinite(x).all()


def test_flat_latent_radii_are_the_drawn_ones(flat):
    flow, x, z, r = flat
    b = flow.base_distribution
    with torch.no_grad():
        zb = flow.backward(x)
    got = _lp_norm(zb - b.loc, float(b.p))
    assert (got - r).abs().max().item() < 2e-5 * max(1.0, r.max().item())


def test_flat_draw_splits_over_calls_and_ranks(flat):
    from usflows_amd.parallel import sample_sharded
    flow, x, z, r = flat
    tol = 2e-5 * max(1.0, x.abs().max().item())
    with torch.no_grad():
        two = torch.cat([flow.sample([1000], seed=11), flow.sample([1000], seed=11, row_offset=1000)])
        assert (two - x).abs().max().item() < tol
        for world in (1, 2, 4):
            parts = torch.cat([sample_sharded(flow, 2000, 11, rank, world) for rank in range(world)])
            assert parts.shape == x.shape and (parts - x).abs().max().item() < tol, world


# ---- image flows -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["imageradial_mnistlive_c16_7x7_k2_l3_lognormal", "imageradial_fashionlive_c16_7x7_k2_l3_gammamm"])
def image(request):
    from golden_util import load_image_radial_case
    flow, _, _, _ = load_image_radial_case(request.param, device=DEV)
    with torch.no_grad():
        x = flow.sample([64], seed=11)
    return flow, x


def test_image_sample_is_a_function_of_the_seed(image):
    from usflows_amd import radial
    flow, x = image
    b = flow.base_distribution
    with torch.no_grad():
        assert torch.equal(flow.sample([64], seed=11), x)
        assert not torch.equal(flow.sample([64], seed=12), x)
        z, r = radial.sample(b, 64, 11, want_r=True)
        zb = flow.backward(x)
        got = _lp_norm(zb - b.loc, float(b.p))
        assert (got - r).abs().max().item() < 2e-5 * max(1.0, r.max().item())
        c = flow.log_prob(x) - b.log_prob(zb)
    assert x.shape == (64, *b.loc.shape) and torch.isfinite(x).all()
    assert (c - c.mean()).abs().max().item() < 1e-4 * abs(c.mean().item())


# ---- the head: no use of the distribution object, no host read-back ---------------------------------------------------------------------
def _count_norm_samples(flow, monkeypatch):
    nd = flow.base_distribution.norm_distribution
    calls = []
    real = nd.sample
    monkeypatch.setattr(nd, "sample", lambda *a_, **k_: (calls.append(1), real(*a_, **k_))[1], raising=False)
    return calls


def test_served_flows_do_not_touch_the_distribution_object(flat, image, monkeypatch):
    from usflows_amd import radial
    for flow, n in ((flat[0], 2000), (image[0], 64)):
        calls = _count_norm_samples(flow, monkeypatch)
        with torch.no_grad():
            flow.sample([n], seed=3)
            flow.sample([n])                                    # (seed=None: a seed from torch's generator, the same head)
        assert calls == []
        # the head itself: no host read-back at all
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            z, r = radial.sample(flow.base_distribution, n, 3, want_r=True)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert z.shape[0] == n and r.shape == (n,)


def test_unserved_norm_distribution_keeps_the_old_route(monkeypatch):
    """a 65-component GammaMM has no device form (K <= 64): radii from its own sample(), directions from usf_radial_sample_f32"""
    from golden_util import load_case
    from model_util import build_flow
    from usflows_amd import distributions as D, radial
    spec, sd, _ = load_case("synth_d16_k3_hh0_conj_radial1_gammamm")
    flow = build_flow(spec, sd, device=DEV)
    g = torch.Generator().manual_seed(0)
    nd = D.GammaMM(2 + 6 * torch.rand(65, generator=g), 0.5 + torch.rand(65, generator=g), torch.ones(65) / 65).to(DEV)
    flow.base_distribution.norm_distribution = nd
    assert radial.norm_spec(nd, torch.device(DEV)) is None and radial.sample(flow.base_distribution, 8, 1) is None
    assert radial.sample_radii(nd, 8, 1) is None
    calls = _count_norm_samples(flow, monkeypatch)
    with torch.no_grad():
        x = flow.sample([500], seed=11)
        r = _lp_norm(flow.backward(x) - flow.base_distribution.loc, 1.0)
    assert calls == [1]
    assert x.shape == (500, 16) and torch.isfinite(x).all()
    # 65 Gamma components with shapes in [2, 8] and rates in [.5, 1.5]: mean radius between 2 / 1.5 and 8 / .5
    assert 1.0 < r.mean().item() < 16.0 and (r > 0).all()


def test_sample_radii_are_the_radii_of_sample(flat):
    from usflows_amd import radial
    flow = flat[0]
    r = radial.sample_radii(flow.base_distribution.norm_distribution, 2000, 11)
    assert r is not None and torch.equal(r, flat[3])
