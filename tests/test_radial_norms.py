"""The radius distributions of the reference's norm-distribution study under ``RadialDistribution`` on the device path:
Weibull (``WeibullMM``, torch ``Weibull``), ``HalfNormal``, the reference's ``Chi``, ``Chi2`` and ``Exponential``
(experiments/mnist/mnist_digits_minimal_radial_*.yaml; distributions.py:55-115, 835-850) -- the component kinds
``USF_NORM_WEIBULL`` / ``HALFNORMAL`` / ``CHI`` of ``usf_radial_logprob_f32`` / ``usf_radial_logprob_grad_f32`` and the host
mapping ``radial.norm_spec`` against fp64 statements of the densities (tests/radial_norms_cases.py) and against golden
vectors of the REAL reference (tests/golden/radial_norms/*.npz, made by tests/golden/make_golden_radial_norms.py)."""
import copy
import math
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_util import grads_close
from radial_norms_cases import (fit_case_names, grad_case_names, load_case, load_chi_grid, load_fit, log_dv64, norm_logp64,
                                ref_radial_logprob)

DEV = "cuda:0"
KINDS = ("weibull", "halfnormal", "exponential", "chi2")          # (+ "chi": a plain distribution only)


def _close(got, want, tol=1e-5, what=""):
    want = want.double().cpu()
    got = got.double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    s = max(want.abs().max().item(), 1e-30)
    err = (got - want).abs().max().item()
    assert err <= tol * s, f"{what}: max abs err {err:.3e} vs scale {s:.3e} (rel {err / s:.2e})"


def _rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).abs() / b.double().cpu().abs().clamp_min(1e-30)).max().item()


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_fp64_statements_equal_torch_and_the_chi_fixture_cpu():
    """the test's own fp64 formulas (what the kernels are held against) are torch's log_prob and the reference's Chi: 1e-12"""
    g = torch.Generator().manual_seed(1)
    r = (0.05 + 6 * torch.rand(200, generator=g, dtype=torch.float64))
    for lam, k in ((1.3, 0.7), (2.0, 1.0), (0.9, 4.5)):
        lam, k = torch.tensor(lam, dtype=torch.float64), torch.tensor(k, dtype=torch.float64)
        assert _rel(norm_logp64("weibull", r, lam, k), torch.distributions.Weibull(lam, k).log_prob(r)) < 1e-12
    for s in (0.4, 2.5):
        s = torch.tensor(s, dtype=torch.float64)
        assert _rel(norm_logp64("halfnormal", r, s, None), torch.distributions.HalfNormal(s).log_prob(r)) < 1e-12
        assert _rel(norm_logp64("exponential", r, s, None), torch.distributions.Exponential(s).log_prob(r)) < 1e-12
    for df in (1.0, 3.5, 40.0):
        df = torch.tensor(df, dtype=torch.float64)
        assert _rel(norm_logp64("chi2", r, df, None), torch.distributions.Chi2(df).log_prob(r)) < 1e-12
    for df, scale, rr, lp, _cdf, _h in load_chi_grid():
        got = norm_logp64("chi", rr, torch.tensor(df, dtype=torch.float64), torch.tensor(scale, dtype=torch.float64))
        assert _rel(got, lp) < 1e-12, (df, scale)


def test_chi_mirror_matches_the_reference_fixture_cpu():
    from usflows_amd import distributions as D
    torch.set_default_dtype(torch.float64)
    try:
        for df, scale, rr, lp, cdf, h in load_chi_grid():
            d = D.Chi(torch.Tensor([df]), scale)
            assert _rel(d.log_prob(rr), lp) < 1e-12 and _rel(d.entropy(), h) < 1e-12, (df, scale)
            assert (d.cdf(rr) - cdf).abs().max().item() < 1e-12, (df, scale)
    finally:
        torch.set_default_dtype(torch.float32)
    d = D.Chi(torch.Tensor([5.0]), 0.5)             # fp32, as the study file builds it
    assert d.batch_shape == (1,) and d.event_shape == ()
    s = d.sample((7, 3))
    assert s.shape == (7, 3, 1) and (s > 0).all() and torch.isfinite(s).all()
    assert d.sample().shape == (1,)
    x = torch.tensor([0.3, 1.0, 2.2])
    assert _rel(d.log_prob(x), norm_logp64("chi", x.double(), torch.tensor(5.0, dtype=torch.float64),
                                            torch.tensor(0.5, dtype=torch.float64))) < 1e-5


def _mm(cls, names, K, positive=True):
    from usflows_amd import distributions as D
    c = torch.distributions.constraints
    return D.MixtureModel(cls, names, {n: (c.positive if positive else c.real) for n in names}, *[torch.ones(K) + i for i in range(len(names))],
                          mixture_weights=torch.zeros(K))


def test_norm_spec_maps_the_study_distributions_cpu():
    """kind, K and the tensors the kernels read, per served object.  ``radial.norm_spec`` serves these radii for a GPU device
    only; the mapping behind it, ``radial.study_norm_spec``, takes any device: the device / dtype checks are on "cpu" here
    (on the device: test_norm_spec_on_the_device)"""
    from usflows_amd import _ext, radial, distributions as D
    td = torch.distributions
    RAW = _ext.NORM_RAW_PARAMS
    spec_of = radial.study_norm_spec
    assert radial.norm_spec(D.WeibullMM(torch.ones(3), 2 * torch.ones(3), torch.zeros(3)), "cpu") is None      # (no kernel on a host device)
    nd = D.WeibullMM(torch.ones(3), 2 * torch.ones(3), torch.zeros(3))
    sp = spec_of(nd, "cpu")
    assert sp[:2] == (_ext.NORM_WEIBULL, 3) and sp[2] is nd.unconstrained_params[0] and sp[3] is nd.unconstrained_params[1] \
        and sp[4] is nd.mixture_logits
    nd = _mm(td.Weibull, ["scale", "concentration"], 5, positive=False)
    assert spec_of(nd, "cpu")[:2] == (_ext.NORM_WEIBULL | RAW, 5)
    nd = _mm(td.HalfNormal, ["scale"], 4)
    sp = spec_of(nd, "cpu")
    assert sp[:2] == (_ext.NORM_HALFNORMAL, 4) and sp[2] is nd.unconstrained_params[0] and sp[3] is None and sp[4] is nd.mixture_logits
    assert spec_of(_mm(td.HalfNormal, ["scale"], 4, positive=False), "cpu")[0] == _ext.NORM_HALFNORMAL | RAW
    # the two Gammas: Exponential(rate) = Gamma(1, rate), Chi2(df) = Gamma(df / 2, 1/2), the constrained value formed on the host
    nd = _mm(td.Exponential, ["rate"], 2)
    sp = spec_of(nd, "cpu")
    assert sp[:2] == (_ext.NORM_GAMMA | RAW, 2) and torch.equal(sp[2], torch.ones(2))
    assert torch.equal(sp[3], F.softplus(nd.unconstrained_params[0])) and sp[3].requires_grad
    nd = _mm(td.Chi2, ["df"], 2, positive=False)
    sp = spec_of(nd, "cpu")
    assert sp[:2] == (_ext.NORM_GAMMA | RAW, 2) and torch.equal(sp[2], 0.5 * nd.unconstrained_params[0]) \
        and torch.equal(sp[3], torch.full((2,), 0.5))
    # plain objects, one-element parameters
    w = td.Weibull(1.0 * 37.5, 1.5)                    # (as the study file writes it: Python floats)
    sp = spec_of(w, "cpu")
    assert sp[:2] == (_ext.NORM_WEIBULL | RAW, 1) and float(sp[2]) == 37.5 and float(sp[3]) == 1.5 and sp[4] is None
    sp = spec_of(td.HalfNormal(torch.tensor([3.0])), "cpu")
    assert sp[:2] == (_ext.NORM_HALFNORMAL | RAW, 1) and float(sp[2]) == 3.0 and sp[3] is None
    sp = spec_of(td.Exponential(0.25), "cpu")
    assert sp[:2] == (_ext.NORM_GAMMA | RAW, 1) and float(sp[2]) == 1.0 and float(sp[3]) == 0.25
    df = torch.tensor([6.0], requires_grad=True)
    sp = spec_of(td.Chi2(df), "cpu")
    assert sp[:2] == (_ext.NORM_GAMMA | RAW, 1) and float(sp[2].detach()) == 3.0 and float(sp[3]) == 0.5 and sp[2].requires_grad
    sp = spec_of(D.Chi(torch.Tensor([2.0]), 1.5), "cpu")
    assert sp[:2] == (_ext.NORM_CHI | RAW, 1) and float(sp[2]) == 2.0 and float(sp[3]) == 1.5 and sp[4] is None
    # not served: a 2-D parameter array, 65 components, more than one element, a parameter that needs a gradient elsewhere
    assert spec_of(D.WeibullMM(torch.ones(3, 2), torch.ones(3, 2), torch.zeros(3, 2)), "cpu") is None
    assert spec_of(D.WeibullMM(torch.ones(65), torch.ones(65), torch.zeros(65)), "cpu") is None
    assert spec_of(D.WeibullMM(torch.ones(64), torch.ones(64), torch.zeros(64)), "cpu")[1] == 64
    assert spec_of(td.Weibull(torch.ones(2), torch.ones(2)), "cpu") is None
    assert spec_of(td.HalfNormal(torch.ones(1, 1)), "cpu") is None
    for ask in (spec_of, radial.norm_spec):
        assert ask(nd, "cuda:0") is None                                  # (a module on the host, asked for the device)
        assert ask(td.Chi2(df), "cuda:0") is None                         # (needs a gradient on the host)
        assert ask(td.HalfNormal(torch.tensor([3.0], requires_grad=True)), "cuda:0") is None
    assert radial.norm_spec(D.GMM(torch.zeros(3, 2), torch.eye(2).expand(3, 2, 2).clone(), torch.zeros(3)), "cuda:0") is None
    assert spec_of(td.Weibull(torch.ones(1, dtype=torch.float64, requires_grad=True), torch.ones(1, dtype=torch.float64)), "cpu") is None


@pytest.mark.parametrize("name", grad_case_names())
def test_mirror_reproduces_the_gradient_fixtures_cpu(name):
    """the mirror's torch formulation on the CPU (the reference's own ops) against the real reference's fp32 run"""
    flow, a, _g, _spec = load_case(name)
    with torch.no_grad():
        assert _rel(flow.log_prob(a["x"]), a["log_prob32"]) < 2e-6
        assert (flow.backward(a["x"]) - a["backward32"]).abs().max().item() < 2e-5 * a["backward32"].abs().max().item()


# ---- GPU: the kernels against fp64 autograd of the statements -------------------------------------------------------------------
def _inv_softplus64(c):
    return torch.where(c > 30.0, c, torch.log(torch.expm1(c)))


def _draw(kind, K, m, g):
    """constrained parameters near the radii (median m), fp64: a [K], b [K] | None"""
    u = lambda: torch.rand(K, generator=g, dtype=torch.float64)       # noqa: E731
    if kind == "weibull":
        return m * (0.7 + 0.6 * u()), 1.0 + 4.0 * u()
    if kind in ("halfnormal", "chi2"):
        return m * (0.7 + 0.6 * u()), None
    if kind == "exponential":
        return (0.5 + u()) / m, None
    nu = 4.0 + 60.0 * u()
    return nu, m / nu.sqrt()


def _norm_object(kind, variant, K, a, b, logits):
    """(the norm distribution on the device, its leaves [a, b | None, logits | None], stored fp32 values the same way,
    softplus?) -- variant "raw": the plain distribution object over one-element leaves; "mm": MixtureModel / WeibullMM"""
    from usflows_amd import distributions as D
    td = torch.distributions
    if variant == "raw":
        la = a.float().to(DEV).requires_grad_(True)
        if kind == "weibull":
            lb = b.float().to(DEV).requires_grad_(True)
            return td.Weibull(scale=la, concentration=lb), [la, lb, None], False
        if kind == "chi":
            s = float(np.float32(b.item()))                  # (the constant scale: a Python float, read as fp32)
            return D.Chi(la, s), [la, torch.tensor([s]), None], False
        cls = {"halfnormal": td.HalfNormal, "exponential": td.Exponential, "chi2": td.Chi2}[kind]
        return cls(la), [la, None, None], False
    cls, names = {"weibull": (td.Weibull, ["scale", "concentration"]), "halfnormal": (td.HalfNormal, ["scale"]),
                  "exponential": (td.Exponential, ["rate"]), "chi2": (td.Chi2, ["df"])}[kind]
    if kind == "weibull" and K == 3:
        nd = D.WeibullMM(torch.ones(K), torch.ones(K), torch.zeros(K))
    else:
        nd = D.MixtureModel(cls, names, {n: td.constraints.positive for n in names}, *[torch.ones(K) for _ in names],
                            mixture_weights=torch.zeros(K))
    # (MixtureModel's own inv_softplus overflows in fp32 beyond 88: the stored values are written directly)
    with torch.no_grad():
        nd.unconstrained_params[0].copy_(_inv_softplus64(a).float())
        if b is not None:
            nd.unconstrained_params[1].copy_(_inv_softplus64(b).float())
        nd.mixture_logits.copy_(logits)
    nd = nd.to(DEV)
    return nd, [nd.unconstrained_params[0], nd.unconstrained_params[1] if b is not None else None, nd.mixture_logits], True


@pytest.mark.gpu
def test_norm_spec_on_the_device():
    """``radial.norm_spec`` itself, for the device: the stored tensors of a WeibullMM as they are; a host-resident parameter
    (the study files' Python floats) through ONE cached fp32 device copy, renewed when the host tensor changes"""
    from usflows_amd import _ext, radial, distributions as D
    dev = torch.device(DEV)
    nd = D.WeibullMM(torch.ones(3), 2 * torch.ones(3), torch.zeros(3)).to(DEV)
    sp = radial.norm_spec(nd, dev)
    assert sp[:2] == (_ext.NORM_WEIBULL, 3) and sp[2] is nd.unconstrained_params[0] and sp[3] is nd.unconstrained_params[1] \
        and sp[4] is nd.mixture_logits
    assert radial.norm_spec(D.WeibullMM(torch.ones(65), torch.ones(65), torch.zeros(65)).to(DEV), dev) is None
    w = torch.distributions.Weibull(1.0 * 37.5, 1.5)
    sp = radial.norm_spec(w, dev)
    assert sp[:2] == (_ext.NORM_WEIBULL | _ext.NORM_RAW_PARAMS, 1) and sp[2].device == dev and sp[2].dtype == torch.float32
    assert sp[2].item() == 37.5 and sp[3].item() == 1.5
    again = radial.norm_spec(w, dev)
    assert again[2] is sp[2] and again[3] is sp[3], "the host parameters were copied twice"
    w.scale.mul_(2.0)                                  # (_version moves on)
    assert radial.norm_spec(w, dev)[2].item() == 75.0
    sp = radial.norm_spec(D.Chi(torch.Tensor([2.0]), 1.5), dev)
    assert sp[:2] == (_ext.NORM_CHI | _ext.NORM_RAW_PARAMS, 1) and sp[2].item() == 2.0 and sp[3].item() == 1.5
    assert radial.norm_spec(torch.distributions.HalfNormal(torch.tensor([3.0], requires_grad=True)), dev) is None


EVENTS = [((7,), 1.0), ((33,), 2.0), ((3, 5, 2), math.inf), ((16, 7, 7), 1.0), ((7,), math.inf), ((33,), 1.0), ((3, 5, 2), 2.0),
          ((16, 7, 7), 2.0), ((16, 7, 7), math.inf)]
KERNEL_CASES = []                    # (kind, variant, K, event shape, p)
for _i, _kind in enumerate(KINDS):
    for _j, (_variant, _K) in enumerate((("raw", 1), ("mm", 1), ("mm", 3), ("mm", 64))):
        KERNEL_CASES.append((_kind, _variant, _K) + EVENTS[(3 * _i + 2 * _j) % len(EVENTS)])
KERNEL_CASES += [("chi", "raw", 1) + EVENTS[0], ("chi", "raw", 1) + EVENTS[1], ("chi", "raw", 1) + EVENTS[8]]


@pytest.mark.gpu
@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: f"{c[0]}-{c[1]}{c[2]}-{'x'.join(map(str, c[3]))}-p{c[4]}")
@pytest.mark.parametrize("B", [1, 5, 300])
def test_radial_norm_kernels_vs_fp64(case, B):
    """forward and backward kernels, reached through ``radial.log_prob`` on the distribution OBJECT (so the host mapping is
    part of what is checked), against fp64 autograd of the statements: log-density, d/dz, d/dloc, d/d(stored parameters),
    d/d(mixture logits); bit-reproducible.  Input recipe and tolerances of test_image_radial.py::test_radial_kernels_vs_fp64."""
    from usflows_amd import _ext, radial, distributions as D
    kind, variant, K, ev, p = case
    Dn = math.prod(ev)
    g = torch.Generator().manual_seed(1000 * Dn + 10 * K + B + 7 * len(kind))
    scale = {1.0: 500.0 / Dn, 2.0: 500.0 / Dn ** 0.5, math.inf: 150.0}[p]
    z = (torch.randn(B, *ev, generator=g) * scale * 1.25)
    loc = 0.1 * scale * torch.randn(*ev, generator=g)
    from radial_norms_cases import radius64
    m = radius64(z.double(), loc.double(), p).median().item()
    a, b = _draw(kind, K, m, g)
    logits = torch.randn(K, generator=g)
    glp = torch.randn(B, generator=g)
    want_kind = {"weibull": _ext.NORM_WEIBULL, "halfnormal": _ext.NORM_HALFNORMAL, "chi": _ext.NORM_CHI}.get(kind, _ext.NORM_GAMMA)
    calls = []
    real_f, real_b = _ext.radial_logprob, _ext.radial_logprob_grad

    def run():
        # (the object is built per run: a Chi2 over a leaf df holds the graph of df / 2, which one backward frees)
        nd, leaves, sp_on = _norm_object(kind, variant, K, a, b, logits)
        base = D.RadialDistribution(loc=loc, norm_distribution=nd, p=p, device=DEV)
        spec = radial.radial_spec(base, torch.device(DEV))
        assert spec is not None and spec["K"] == K and (spec["norm"] & 0xff) == want_kind
        zd = z.to(DEV).requires_grad_(True)
        _ext.radial_logprob = lambda *a_, **k_: (calls.append("f"), real_f(*a_, **k_))[1]
        _ext.radial_logprob_grad = lambda *a_, **k_: (calls.append("b"), real_b(*a_, **k_))[1]
        try:
            lp = radial.log_prob(base, zd)
            assert lp is not None
            lp.backward(glp.to(DEV))
        finally:
            _ext.radial_logprob, _ext.radial_logprob_grad = real_f, real_b
        return ([lp.detach(), zd.grad, base.loc.grad.clone()]
                + [None if (t is None or not t.requires_grad) else t.grad.clone() for t in leaves]), leaves, sp_on

    got, leaves, sp_on = run()
    assert calls == ["f", "b"], calls
    z6, l6 = z.double().requires_grad_(True), loc.double().requires_grad_(True)
    st = [None if t is None else t.detach().double().cpu().requires_grad_(True) for t in leaves]
    lp6, _r6 = ref_radial_logprob(z6, l6, p, kind, st[0], st[1], st[2] if variant == "mm" else None, sp_on)
    lp6.backward(glp.double())
    _close(got[0], lp6.detach(), 2e-6, "logp")
    _close(got[1], z6.grad, 2e-5, "dz")
    _close(got[2], l6.grad, 2e-5, "dloc")
    for gq, rq, what in ((got[3], st[0], "da"), (got[4], st[1], "db"), (got[5], st[2], "dlogits")):
        if gq is None:
            continue
        s = max(rq.grad.abs().max().item(), 1e-3 * glp.abs().sum().item())
        assert (gq.double().cpu() - rq.grad).abs().max().item() <= 2e-4 * s, (what, gq, rq.grad)
    assert got[3] is not None and (variant == "raw" or got[5] is not None)
    again, _, _ = run()
    for u, v in zip(got, again):
        assert (u is None and v is None) or torch.equal(u, v), "not bit-reproducible"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["weibull", "halfnormal", "chi"])
def test_radial_norm_kernel_given_radii_logdet_and_sums(kind):
    """the entry points themselves: the fp64 device log-det scalar and the data-parallel sums, then the radii-given mode (flat
    training path) with its gradients -- as test_radial_kernel_raw_parameters_given_radii_and_sums does for the old kinds"""
    from usflows_amd import _ext, radial
    g = torch.Generator().manual_seed(5)
    B, Dn = 77, 784
    z = torch.randn(B, Dn, generator=g) * 0.8
    loc = torch.zeros(Dn)
    K = 1 if kind == "chi" else 3
    a, b = _draw(kind, K, 500.0, g)
    a, b = a.float(), (None if b is None else b.float())
    logits = None if K == 1 else torch.randn(K, generator=g)
    norm = {"weibull": _ext.NORM_WEIBULL, "halfnormal": _ext.NORM_HALFNORMAL, "chi": _ext.NORM_CHI}[kind] | _ext.NORM_RAW_PARAMS
    lp6, r6 = ref_radial_logprob(z.double(), loc.double(), 1.0, kind, a.double(), None if b is None else b.double(),
                                 None if logits is None else logits.double(), False)
    dv = lambda t: None if t is None else t.to(DEV)       # noqa: E731
    out = torch.empty(B, device=DEV)
    r = torch.empty(B, device=DEV)
    sums = torch.zeros(2, dtype=torch.float64, device=DEV)
    ld = torch.tensor([-12.5], dtype=torch.float64, device=DEV)
    _ext.radial_logprob(z.to(DEV), Dn, B, Dn, _ext.BASE_LPNORM1, loc.to(DEV), norm, K, dv(a), dv(b), dv(logits),
                        radial.log_dv_const(1.0, Dn), 0.25, out, r_out=r, sum_out=sums, logdet_dev=ld)
    _close(out, lp6 - 12.25, 2e-6, "logp + logdet")
    _close(r, r6, 1e-6, "r")
    assert abs(sums[0].item() - out.double().sum().item()) < 1e-6 * abs(sums[0].item()) and sums[1].item() == B
    rr = r.clone().requires_grad_(True)
    ps = [None if t is None else t.to(DEV).requires_grad_(True) for t in (a, b, logits)]
    lp = radial.RadialFinish.apply(rr, ps[0], ps[1], ps[2], _ext.BASE_LPNORM1, norm, K, Dn, radial.log_dv_const(1.0, Dn))
    lp.sum().backward()
    r64 = r.double().cpu().requires_grad_(True)
    p64 = [None if t is None else t.double().requires_grad_(True) for t in (a, b, logits)]
    comp = norm_logp64(kind, r64.unsqueeze(-1), p64[0], p64[1])
    if logits is not None:
        comp = comp + torch.log_softmax(p64[2], -1)
    ref = torch.logsumexp(comp, -1) - log_dv64(1.0, Dn, r64)
    ref.sum().backward()
    _close(lp.detach(), ref.detach(), 1e-6, "finish")
    _close(rr.grad, r64.grad, 1e-5, "d/dr")
    for t, t64, what in zip(ps, p64, ("d/da", "d/db", "d/dlogits")):
        if t is not None:
            _close(t.grad, t64.grad, 1e-4, what)


@pytest.mark.gpu
def test_every_component_at_minus_infinity_gives_minus_infinity():
    """a Weibull far in its tail (k = 50, r / lambda = 1e7): each component's log-density is -inf; the row is -inf as
    torch.logsumexp gives it, not NaN -- next to a row where the density is finite"""
    from usflows_amd import _ext, radial
    lam = torch.tensor([1.0, 2.0], device=DEV)
    k = torch.tensor([50.0, 50.0], device=DEV)
    logits = torch.tensor([0.3, -0.2], device=DEV)
    r = torch.tensor([1e7, 1.5, 2e7], device=DEV)
    out = torch.full((3,), 7.0, device=DEV)
    _ext.radial_logprob(None, 0, 3, 5, _ext.BASE_LPNORM2, None, _ext.NORM_WEIBULL | _ext.NORM_RAW_PARAMS, 2, lam, k, logits,
                        radial.log_dv_const(2.0, 5), 0.0, out, r_out=r)
    out = out.cpu()
    assert out[0].item() == -math.inf and out[2].item() == -math.inf, out
    r6 = r.double().cpu()
    comp = norm_logp64("weibull", r6.unsqueeze(-1), lam.double().cpu(), k.double().cpu()) + torch.log_softmax(logits.double().cpu(), -1)
    ref = torch.logsumexp(comp, -1) - log_dv64(2.0, 5, r6)
    assert ref[0].item() == -math.inf and abs(out[1].item() - ref[1].item()) <= 2e-6 * abs(ref[1].item())


# ---- GPU: whole flows against the real reference --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", grad_case_names())
def test_flows_over_the_study_bases_match_the_real_reference_on_the_device(name, monkeypatch):
    """log_prob, backward, _forward and the gradients of Flow.fit's loss w.r.t. layer AND base parameters, at the tolerances of
    test_live_configuration_on_the_device_matches_the_real_reference; the base density and its gradient come from the radial
    kernels (call record), without a host synchronisation once the caches are filled"""
    from usflows_amd import _ext
    flow, a, g_ref, spec = load_case(name, device=DEV)
    x = a["x"].to(DEV)
    calls, gcalls = [], []
    real, real_g = _ext.radial_logprob, _ext.radial_logprob_grad
    monkeypatch.setattr(_ext, "radial_logprob", lambda *a_, **k_: (calls.append(1), real(*a_, **k_))[1])
    monkeypatch.setattr(_ext, "radial_logprob_grad", lambda *a_, **k_: (gcalls.append(1), real_g(*a_, **k_))[1])
    with torch.no_grad():
        flow.log_prob(x)                               # (first sighting: caches fill, the host parameters are copied once)
    assert len(calls) == 1, "the base density did not run on usf_radial_logprob_f32"
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            lp = flow.log_prob(x)
            assert len(calls) == 2, "the base density did not run on usf_radial_logprob_f32"
            lp3 = flow.log_prob(x)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(lp, lp3)
    if len(spec["in_dims"]) == 3:
        plan = flow.__dict__["_loop_lists"][(tuple(x.shape), str(x.device))][1]
        assert plan is not None and len(calls) == 2, "the op list of the image flow is not pure"
    _close(lp, a["log_prob64"], 1e-5, "log_prob vs fp64 reference")
    _close(lp, a["log_prob32"], 1e-5, "log_prob vs fp32 reference")
    assert _rel(lp, a["log_prob64"]) <= 1e-5, "log_prob row-wise (the project's parity bound)"
    with torch.no_grad():
        _close(flow.backward(x), a["backward64"], 1e-5, "backward")
        _close(flow._forward(a["zin"].to(DEV)), a["forward64"], 1e-5, "_forward")
    n_f = len(calls)
    lpg = flow.log_prob(x)
    assert len(calls) == n_f + 1, "the training pass's base density did not run on usf_radial_logprob_f32"
    _close(lpg.detach(), a["log_prob64"], 1e-5, "log_prob under autograd")
    loss = -lpg.mean() - flow.log_prior()
    loss.backward()
    assert len(gcalls) == 1, "the base density's gradient did not come from usf_radial_logprob_grad_f32"
    assert abs(float(loss.detach()) - float(a["loss64"])) < 1e-5 * abs(float(a["loss64"]))
    named = dict(flow.named_parameters())
    assert "base_distribution.loc" in g_ref and set(g_ref) <= set(named)
    grads_close(named, g_ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name", fit_case_names())
def test_weibullmm_fit_on_device_matches_reference_run(name, monkeypatch):
    """Flow.fit with SophiaG at the live hyper-parameters over a WeibullMM radius reproduces the reference's own 6 steps, eagerly
    and with the step captured and replayed: graph_replays == steps - 3 and no capture warning (tolerances of
    test_live_configuration_fit_on_device_matches_reference_run)"""
    from usflows_amd import _ext
    for graph in ("0", "1"):
        monkeypatch.setenv("USFLOWS_AMD_TRAIN_GRAPH", graph)
        flow, data, losses_ref, sd_ref = load_fit(name, device=DEV)
        calls = []
        real = _ext.radial_logprob_grad
        monkeypatch.setattr(_ext, "radial_logprob_grad", lambda *a_, **k_: (calls.append(1), real(*a_, **k_))[1])
        ds = torch.utils.data.TensorDataset(data, torch.zeros(data.shape[0]))
        np.random.seed(5)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            losses = flow.fit(ds, optim_params=dict(lr=1e-3, weight_decay=0.0), batch_size=32, shuffle=True, device=torch.device(DEV),
                              epochs=2)
        monkeypatch.setattr(_ext, "radial_logprob_grad", real)
        assert not [w for w in caught if "capture" in str(w.message)], [str(w.message) for w in caught]
        assert len(calls) > 0, "the base density's gradient did not come from usf_radial_logprob_grad_f32"
        st = flow.__dict__.get("_train_graph_state")
        if graph == "1":
            assert st is not None and st["graph"] is not None and st["replays"] == 6 - 3, (st and st["replays"])
        for l, r in zip(losses, losses_ref):
            assert abs(float(l) - r) < 2e-4 * abs(r), (graph, losses, losses_ref)
        sd = flow.state_dict()
        for k, v in sd_ref.items():
            s = max(v.abs().max().item(), 1e-3)
            d = (sd[k].cpu().double() - v.double()).abs()
            assert d.max().item() <= 2.1e-3 + 2e-3 * s, (graph, k, d.max().item())
            assert (d > 1e-4 * s + 1e-6).double().mean().item() < 0.02, (graph, k, "more than 2 % of the entries took another sign")


@pytest.mark.gpu
@pytest.mark.parametrize("B", [0, 1, 3])
def test_weibullmm_empty_and_tiny_batches(B):
    """an empty batch (empty log_prob; zero gradients for the base's parameters), one and three rows -- against the mirror on
    the CPU, as test_live_configuration_empty_and_tiny_batches"""
    name = "grads_image_c16_7x7_k2_weibullmm3_p1"
    flow, a, _, spec = load_case(name)
    cpu = copy.deepcopy(flow)
    flow = flow.to(DEV)
    x = a["x"][:B]
    with torch.no_grad():
        lp = flow.log_prob(x.to(DEV))
    assert lp.shape == (B,)
    if B:
        with torch.no_grad():
            _close(lp, cpu.log_prob(x), 2e-6, "log_prob")
    lpg = flow.log_prob(x.to(DEV))
    lpg.sum().backward()
    named, named_c = dict(flow.named_parameters()), dict(cpu.named_parameters())
    if B:
        lpc = cpu.log_prob(x)
        lpc.sum().backward()
    for k in ("base_distribution.loc", "base_distribution.norm_distribution.unconstrained_params.0",
              "base_distribution.norm_distribution.unconstrained_params.1", "base_distribution.norm_distribution.mixture_logits"):
        g = named[k].grad
        assert g is not None and torch.isfinite(g).all(), k
        if B == 0:
            assert not g.any(), k
        else:
            gc = named_c[k].grad
            s = max(gc.abs().max().item(), 1e-6)
            assert (g.cpu() - gc).abs().max().item() <= 2e-4 * s + 1e-6 * lpc.abs().sum().item() / max(B, 1), k
