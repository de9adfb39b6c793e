"""``RadialDistribution.log_prob`` on the device, forward and backward (the base distribution of every live
image configuration of the reference: experiments/mnist/mnist.yaml:79-92 ``LogNormal(6, .35)``,
experiments/fashion/fashionclasses_veriflow.yaml:79-93 ``GammaMM`` x 20, experiments/cifar/cifar.yaml).

Reference arithmetic (src/usflows/distributions.py:501-549)::

    r    = (x - loc).norm(p, dim=event_dims)
    logp = norm_distribution.log_prob(r.unsqueeze(-1)).squeeze(-1) - log_delta_volume(p, r)

The torch formulation is ~25 small launches plus the construction of a fresh, argument-validating distribution object per
call (``DistributionModule.distribution``, distributions.py:127-139) whose validation reads a flag back to the host: no
stream capture, one host round trip per training step.  Here the whole density is ``usf_radial_logprob_f32`` (radius
reduction over the flattened event + the norm distribution's mixture density + the volume term, one launch) and its
gradient ``usf_radial_logprob_grad_f32`` (d/dz, d/dloc, d/d(norm parameters), d/d(mixture logits)): no host
synchronisation, capturable, for flat AND image-shaped events.

Served norm distributions (``norm_spec``): the ``LogNormal`` / ``Gamma`` modules with one-element parameters, ``GammaMM`` and
``MixtureModel`` over ``torch.distributions.LogNormal`` (``LogNormalMM``) with up to 64 components along one axis, and plain
``torch.distributions.LogNormal`` / ``Gamma`` objects with one-element parameters on the device; the radii of the reference's
norm-distribution study (experiments/mnist/mnist_digits_minimal_radial_*.yaml): ``WeibullMM`` and ``MixtureModel`` over torch
``Weibull`` / ``Exponential`` / ``HalfNormal`` / ``Chi2``, and plain ``Weibull`` / ``Exponential`` / ``HalfNormal`` / ``Chi2`` /
``Chi`` objects with one-element parameters (``Exponential(rate)`` is ``Gamma(1, rate)``, ``Chi2(df)`` is ``Gamma(df / 2, 1/2)``:
both run as the Gamma kind; the study's radii are served for a GPU device only, ``study_norm_spec`` is their mapping for
any device).  Anything else keeps the distribution object's op chain.
"""
from __future__ import annotations

import math
import weakref
from typing import Optional

import torch
from torch.nn.functional import softplus

from . import _ext
from . import distributions as D_


def p_id_of(p: float) -> Optional[int]:
    return {1.0: _ext.BASE_LPNORM1, 2.0: _ext.BASE_LPNORM2, float("inf"): _ext.BASE_LPNORMINF}.get(float(p))


def log_dv_const(p: float, d: int) -> float:
    """the r-independent part of ``RadialDistribution.log_delta_volume`` (distributions.py:513-549), in fp64 on the host:
    log dV_p(r) = log_dv_const + (d - 1) log r"""
    if p == 1:
        return math.log(2) * d - math.lgamma(d)                      # sum_{i<d} log i = log (d-1)!
    if p == 2:
        return math.log(d) + (d / 2) * math.log(math.pi) - math.lgamma(d / 2 + 1)
    if p == math.inf:
        return math.log(d) + d * math.log(2)
    raise ValueError(f"p={p} not implemented. Use p=1,2, or infinity")


def _dev_f32(t, device) -> bool:
    return torch.is_tensor(t) and t.dtype == torch.float32 and t.device == device and t.is_contiguous()


_consts = {}         # (device, K, value) -> fp32 [K] tensor filled with value
_host_copies = {}    # (data_ptr, _version, device) -> (weak reference to the host tensor, its fp32 device copy)


def _const(device, K, value):
    """a constant parameter of a component kind (the concentration 1 of an Exponential, the rate 1/2 of a Chi2)"""
    key = (str(device), int(K), float(value))
    t = _consts.get(key)
    if t is None:
        t = _consts[key] = torch.full((int(K),), float(value), dtype=torch.float32, device=device)
    return t


def _servable(t, device) -> bool:
    """whether ``_served`` has a device form of this parameter of one of the study's norm distributions"""
    if isinstance(t, (int, float)) and not isinstance(t, bool):
        return True
    if not torch.is_tensor(t) or t.numel() != 1:
        return False
    return _dev_f32(t, device) or (t.device.type == "cpu" and device.type != "cpu" and not t.requires_grad and t.is_floating_point())


def _served(t, device):
    """a one-element parameter as the kernels can read it: an fp32 device tensor as it is; a Python number as a cached
    constant; a HOST-resident tensor without grad (the study files pass Python floats and host tensors, which torch keeps on
    the host) through one cached fp32 device copy, keyed on (data_ptr, _version)"""
    if not torch.is_tensor(t):
        return _const(device, 1, float(t))
    if _dev_f32(t, device):
        return t
    key = (t.data_ptr(), t._version, str(device))
    hit = _host_copies.get(key)
    if hit is not None and hit[0]() is t:
        return hit[1]
    if len(_host_copies) >= 256:
        _host_copies.clear()
    c = t.detach().to(device=device, dtype=torch.float32).contiguous()
    _host_copies[key] = (weakref.ref(t), c)
    return c


def _positive(nd, name) -> bool:
    """whether MixtureModel stores this parameter through softplus (distributions.py:762)"""
    c = nd.param_constraints.get(name)
    return isinstance(c, type(torch.distributions.constraints.positive)) and getattr(c, "lower_bound", None) == 0.0


def _study_mixture_spec(nd, device):
    """MixtureModel over torch Weibull / Exponential / HalfNormal / Chi2 components (WeibullMM included)"""
    cls, names = nd.component_distribution_class, list(nd.param_names)
    ps, l = list(nd.unconstrained_params), nd.mixture_logits
    K = ps[0].numel()
    if not (all(q.dim() == 1 and q.shape == l.shape for q in ps) and 1 <= K <= _ext.RADIAL_MAX_K
            and all(_dev_f32(t, device) for t in ps + [l])):
        return None
    pos = [_positive(nd, n) for n in names]
    raw = 0 if pos[0] else _ext.NORM_RAW_PARAMS
    if cls is torch.distributions.Weibull and names == ["scale", "concentration"]:
        if pos[0] != pos[1]:
            return None
        return _ext.NORM_WEIBULL | raw, K, ps[0], ps[1], l
    if cls is torch.distributions.HalfNormal and names == ["scale"]:
        return _ext.NORM_HALFNORMAL | raw, K, ps[0], None, l
    # the two Gammas: the constrained parameter is formed here (one or two tensor ops, differentiable), the kernel takes it raw
    if cls is torch.distributions.Exponential and names == ["rate"]:
        return _ext.NORM_GAMMA | _ext.NORM_RAW_PARAMS, K, _const(device, K, 1.0), softplus(ps[0]) if pos[0] else ps[0], l
    if cls is torch.distributions.Chi2 and names == ["df"]:
        return _ext.NORM_GAMMA | _ext.NORM_RAW_PARAMS, K, 0.5 * (softplus(ps[0]) if pos[0] else ps[0]), _const(device, K, 0.5), l
    return None


def _study_plain_spec(nd, device):
    """plain torch Weibull / Exponential / HalfNormal / Chi2 objects and the mirror's Chi, one-element parameters"""
    if type(nd) is D_.Chi:
        kind, a, b = _ext.NORM_CHI, nd.df, nd.scale
    elif len(nd.batch_shape) > 1:
        return None
    elif type(nd) is torch.distributions.Weibull:
        kind, a, b = _ext.NORM_WEIBULL, nd.scale, nd.concentration
    elif type(nd) is torch.distributions.HalfNormal:
        kind, a, b = _ext.NORM_HALFNORMAL, nd.scale, None
    elif type(nd) is torch.distributions.Exponential:
        kind, a, b = _ext.NORM_GAMMA, 1.0, nd.rate
    else:                                       # Chi2(df) IS torch's Gamma(df / 2, 1/2): concentration carries the link to df
        kind, a, b = _ext.NORM_GAMMA, nd.concentration, nd.rate
    if not _servable(a, device) or not (b is None or _servable(b, device)):
        return None
    return kind | _ext.NORM_RAW_PARAMS, 1, _served(a, device), None if b is None else _served(b, device), None


_STUDY_COMPONENTS = (torch.distributions.Weibull, torch.distributions.Exponential, torch.distributions.HalfNormal,
                     torch.distributions.Chi2)


def norm_spec(nd, device):
    """(norm id, K, par_a, par_b | None, logits | None) -- the STORED tensors of the norm distribution, as the kernels read
    them -- or None when this norm distribution has no device form"""
    device = torch.device(device)
    if isinstance(nd, D_.LogNormal) and type(nd) is D_.LogNormal:
        a, b = nd.loc, nd.scale_unconstrained
        if a.numel() == 1 and b.numel() == 1 and _dev_f32(a, device) and _dev_f32(b, device):
            return _ext.NORM_LOGNORMAL, 1, a, b, None
        return None
    if isinstance(nd, D_.Gamma) and type(nd) is D_.Gamma:
        a, b = nd.concentration_unconstrained, nd.rate_unconstrained
        if a.numel() == 1 and b.numel() == 1 and _dev_f32(a, device) and _dev_f32(b, device):
            return _ext.NORM_GAMMA, 1, a, b, None
        return None
    if isinstance(nd, D_.GammaMM) and type(nd) is D_.GammaMM:
        a, b, l = nd.concentration_unconstrained, nd.rate_unconstrained, nd.mixture_logits
        K = a.numel()
        if a.dim() == 1 and b.shape == a.shape and l.shape == a.shape and 1 <= K <= _ext.RADIAL_MAX_K \
                and all(_dev_f32(t, device) for t in (a, b, l)):
            return _ext.NORM_GAMMA, K, a, b, l
        return None
    if isinstance(nd, D_.MixtureModel) and nd.component_distribution_class is torch.distributions.LogNormal \
            and list(nd.param_names) == ["loc", "scale"]:
        a, b = nd.unconstrained_params[0], nd.unconstrained_params[1]
        l = nd.mixture_logits
        K = a.numel()
        c = nd.param_constraints.get("scale")
        positive = isinstance(c, type(torch.distributions.constraints.positive)) and getattr(c, "lower_bound", None) == 0.0
        if a.dim() == 1 and b.shape == a.shape and l.shape == a.shape and 1 <= K <= _ext.RADIAL_MAX_K \
                and all(_dev_f32(t, device) for t in (a, b, l)):
            return _ext.NORM_LOGNORMAL | (0 if positive else _ext.NORM_RAW_PARAMS), K, a, b, l
        return None
    if type(nd) is torch.distributions.LogNormal:
        a, b = nd.loc, nd.scale
        if a.numel() == 1 and b.numel() == 1 and len(nd.batch_shape) <= 1 and _dev_f32(a, device) and _dev_f32(b, device):
            return _ext.NORM_LOGNORMAL | _ext.NORM_RAW_PARAMS, 1, a, b, None
        return None
    if type(nd) is torch.distributions.Gamma:
        a, b = nd.concentration, nd.rate
        if a.numel() == 1 and b.numel() == 1 and len(nd.batch_shape) <= 1 and _dev_f32(a, device) and _dev_f32(b, device):
            return _ext.NORM_GAMMA | _ext.NORM_RAW_PARAMS, 1, a, b, None
        return None
    # the study's radii are served where the kernels run: asked about a host device (the CPU formulation, which has no
    # kernel behind it) they have no device form
    return study_norm_spec(nd, device) if device.type == "cuda" else None


def study_norm_spec(nd, device):
    """``norm_spec`` of the radius distributions of the norm-distribution study -- WeibullMM / MixtureModel over torch
    Weibull, Exponential, HalfNormal, Chi2; those plain objects; Chi -- for tensors on ``device``, whatever its type (the
    mapping itself needs no GPU); None for everything else"""
    device = torch.device(device)
    if isinstance(nd, D_.MixtureModel) and nd.component_distribution_class in _STUDY_COMPONENTS:
        return _study_mixture_spec(nd, device)
    if type(nd) in _STUDY_COMPONENTS or type(nd) is D_.Chi:
        return _study_plain_spec(nd, device)
    return None


def radial_spec(base, device):
    """everything the kernels need of a ``RadialDistribution``: dict(p_id, D, loc, norm, K, a, b, logits, logdv) or None"""
    if not isinstance(base, D_.RadialDistribution) or base.n_batch_dims != 0:
        return None
    p_id = p_id_of(base.p)
    if p_id is None or not _dev_f32(base.loc, torch.device(device)):
        return None
    ns = norm_spec(base.norm_distribution, device)
    if ns is None:
        return None
    d = int(base.loc.numel())
    return dict(p_id=p_id, D=d, loc=base.loc, norm=ns[0], K=ns[1], a=ns[2], b=ns[3], logits=ns[4],
                logdv=log_dv_const(base.p, d))


class RadialLogProb(torch.autograd.Function):
    """logp [B] of rows z [B, *event] under the radial density; gradients of z, loc, the norm parameters and the logits"""

    @staticmethod
    def forward(ctx, z, loc, par_a, par_b, logits, p_id, norm, K, logdv):
        B = z.shape[0]
        d = loc.numel()
        zf = z.detach().reshape(B, d).contiguous()
        locf = loc.detach().reshape(-1)
        out = torch.empty(B, dtype=torch.float32, device=z.device)
        r = torch.empty(B, dtype=torch.float32, device=z.device)
        a, b = par_a.detach(), (None if par_b is None else par_b.detach())        # (a one-parameter kind has no par_b)
        lg = None if logits is None else logits.detach()
        if B > 0:
            _ext.radial_logprob(zf, d, B, d, p_id, locf, norm, K, a, b, lg, logdv, 0.0, out, r_out=r)
        ctx.save_for_backward(zf, r, locf, a, b, lg)
        ctx.cfg = (p_id, norm, K, tuple(z.shape), tuple(loc.shape), tuple(par_a.shape), None if par_b is None else tuple(par_b.shape),
                   None if logits is None else tuple(logits.shape))
        return out

    @staticmethod
    def backward(ctx, g_lp):
        zf, r, locf, a, b, lg = ctx.saved_tensors
        p_id, norm, K, zshape, lshape, ashape, bshape, gshape = ctx.cfg
        B, d = zf.shape
        need = ctx.needs_input_grad
        dev = zf.device
        g = torch.empty_like(zf)
        d_loc = torch.empty(d, dtype=torch.float32, device=dev) if need[1] else None
        d_a = torch.empty(K, dtype=torch.float32, device=dev) if need[2] else None
        d_b = torch.empty(K, dtype=torch.float32, device=dev) if (b is not None and need[3]) else None
        d_l = torch.empty(K, dtype=torch.float32, device=dev) if (lg is not None and need[4]) else None
        _ext.radial_logprob_grad(zf, d, r, g_lp.contiguous(), B, d, p_id, locf, norm, K, a, b, lg, g, d, d_loc=d_loc, d_a=d_a,
                                 d_b=d_b, d_logits=d_l)
        return (g.reshape(zshape) if need[0] else None,
                None if d_loc is None else d_loc.reshape(lshape),
                None if d_a is None else d_a.reshape(ashape),
                None if d_b is None else d_b.reshape(bshape),
                None if d_l is None else d_l.reshape(gshape), None, None, None, None)


class RadialFinish(torch.autograd.Function):
    """logp [B] from GIVEN radii r [B] (the flat training path's tail kernel reduces them): the finishing formula
    norm_dist.log_prob(r) - log dV_p(r) and its gradients at r, the norm parameters and the logits"""

    @staticmethod
    def forward(ctx, r, par_a, par_b, logits, p_id, norm, K, d, logdv):
        B = r.shape[0]
        rc = r.detach().contiguous()
        out = torch.empty(B, dtype=torch.float32, device=r.device)
        a, b = par_a.detach(), (None if par_b is None else par_b.detach())
        lg = None if logits is None else logits.detach()
        if B > 0:
            _ext.radial_logprob(None, 0, B, d, p_id, None, norm, K, a, b, lg, logdv, 0.0, out, r_out=rc)
        ctx.save_for_backward(rc, a, b, lg)
        ctx.cfg = (p_id, norm, K, d, tuple(par_a.shape), None if par_b is None else tuple(par_b.shape),
                   None if logits is None else tuple(logits.shape))
        return out

    @staticmethod
    def backward(ctx, g_lp):
        rc, a, b, lg = ctx.saved_tensors
        p_id, norm, K, d, ashape, bshape, gshape = ctx.cfg
        B = rc.shape[0]
        need = ctx.needs_input_grad
        dev = rc.device
        g = torch.empty(B, dtype=torch.float32, device=dev)
        d_a = torch.empty(K, dtype=torch.float32, device=dev) if need[1] else None
        d_b = torch.empty(K, dtype=torch.float32, device=dev) if (b is not None and need[2]) else None
        d_l = torch.empty(K, dtype=torch.float32, device=dev) if (lg is not None and need[3]) else None
        _ext.radial_logprob_grad(None, 0, rc, g_lp.contiguous(), B, d, p_id, None, norm, K, a, b, lg, g, 0, d_a=d_a, d_b=d_b,
                                 d_logits=d_l)
        return (g if need[0] else None,
                None if d_a is None else d_a.reshape(ashape),
                None if d_b is None else d_b.reshape(bshape),
                None if d_l is None else d_l.reshape(gshape), None, None, None, None, None)


def log_prob(base, z: torch.Tensor, logdet_dev: Optional[torch.Tensor] = None, sum_out: Optional[torch.Tensor] = None,
             ldz: Optional[int] = None):
    """``base.log_prob(z)`` (+ the fp64 device scalar ``logdet_dev``) on the kernels, or None when this base / input has no
    device form.  Differentiable when autograd is on and anything involved requires a gradient.  ``ldz``: z is a raw
    [B, ldz] fp32 buffer whose first D columns are the event (the flat engine's latent buffer); inference only."""
    if not (torch.is_tensor(z) and z.is_cuda and z.dtype == torch.float32 and z.dim() >= 2):
        return None
    sp = radial_spec(base, z.device)
    if sp is None:
        return None
    d = sp["D"]
    if ldz is None and (math.prod(z.shape[1:]) != d or tuple(z.shape[1:]) != tuple(base.loc.shape)):
        return None
    _ext.load()
    train = torch.is_grad_enabled() and (z.requires_grad or any(
        torch.is_tensor(t) and t.requires_grad for t in (sp["loc"], sp["a"], sp["b"], sp["logits"])))
    if train:
        if ldz is not None or logdet_dev is not None or sum_out is not None:
            return None
        return RadialLogProb.apply(z, sp["loc"], sp["a"], sp["b"], sp["logits"], sp["p_id"], sp["norm"], sp["K"], sp["logdv"])
    B = z.shape[0]
    out = torch.empty(B, dtype=torch.float32, device=z.device)
    if B == 0:
        return out
    if ldz is None:
        zf, ldz = z.reshape(B, d), d
        if not zf.is_contiguous():
            zf = zf.contiguous()
    else:
        zf = z
    lg = sp["logits"]
    _ext.radial_logprob(zf, ldz, B, d, sp["p_id"], sp["loc"].detach().reshape(-1), sp["norm"], sp["K"], sp["a"].detach(),
                        None if sp["b"] is None else sp["b"].detach(), None if lg is None else lg.detach(), sp["logdv"], 0.0, out,
                        sum_out=sum_out,
                        logdet_dev=logdet_dev)
    return out


def log_prob_from_radius(base, r: torch.Tensor):
    """the finishing formula on given radii (differentiable), or None when the norm distribution has no device form"""
    if not (torch.is_tensor(r) and r.is_cuda and r.dtype == torch.float32 and r.dim() == 1):
        return None
    sp = radial_spec(base, r.device)
    if sp is None:
        return None
    _ext.load()
    return RadialFinish.apply(r, sp["a"], sp["b"], sp["logits"], sp["p_id"], sp["norm"], sp["K"], sp["D"], sp["logdv"])


# ---- sampling: radii and directions in one launch (usf_radial_sample_norm_f32) -------------------------------------------------
def sample(base, n: int, seed: int, offset: int = 0, row_offset: int = 0, want_r: bool = False):
    """``n`` rows z [n, D] ~ ``base`` (a ``RadialDistribution`` on a GPU; D = the flattened event) from ONE launch: row i is a
    pure function of (seed, offset, i + row_offset, the parameters) -- the same rows for any split of a draw over calls or
    ranks, no host read-back, no use of torch's generator.  ``want_r``: (z, r [n]), the radii drawn.  None when
    ``radial_spec`` has no device form of this base (the caller keeps the distribution object's own ``sample``)."""
    loc = getattr(base, "loc", None)
    if not (torch.is_tensor(loc) and loc.is_cuda):
        return None
    with torch.no_grad():
        sp = radial_spec(base, loc.device)
        if sp is None:
            return None
        _ext.load()
        n, d = int(n), sp["D"]
        z = torch.empty(n, d, dtype=torch.float32, device=loc.device)
        r = torch.empty(n, dtype=torch.float32, device=loc.device) if want_r else None
        if n > 0:
            b, lg = sp["b"], sp["logits"]
            _ext.radial_sample_norm(z, d, n, d, sp["p_id"], loc.detach().reshape(-1), sp["norm"], sp["K"], sp["a"].detach(),
                                    None if b is None else b.detach(), None if lg is None else lg.detach(), r, int(seed), int(offset),
                                    int(row_offset))
    return (z, r) if want_r else z


def _norm_device(nd):
    """the device a norm distribution's parameters live on (None: it holds no tensor)"""
    if isinstance(nd, torch.nn.Module):
        for t in list(nd.parameters()) + list(nd.buffers()):
            return t.device
    for t in vars(nd).values():
        if torch.is_tensor(t):
            return t.device
    return None


def sample_radii(norm_distribution, n: int, seed: int, offset: int = 0, row_offset: int = 0, device=None):
    """``n`` radii r [n] ~ ``norm_distribution`` from the same launch without a direction (z == NULL): exactly the radii
    ``sample`` draws for these arguments.  ``device``: where the parameters live (default: taken from them).  None when
    ``norm_spec`` has no device form of this distribution."""
    device = torch.device(device) if device is not None else _norm_device(norm_distribution)
    if device is None or device.type != "cuda":
        return None
    with torch.no_grad():
        ns = norm_spec(norm_distribution, device)
        if ns is None:
            return None
        _ext.load()
        norm, K, a, b, lg = ns
        r = torch.empty(int(n), dtype=torch.float32, device=device)
        if n > 0:
            _ext.radial_sample_norm(None, 0, int(n), 0, 0, None, norm, K, a.detach(), None if b is None else b.detach(),
                                    None if lg is None else lg.detach(), r, int(seed), int(offset), int(row_offset))
    return r
