"""Golden vectors of flows over a ``RadialDistribution`` whose radius ("norm") distribution comes from the reference's
norm-distribution study -- Weibull, half-normal, chi, chi-square, exponential -- from the REAL reference (this container only).

    python tests/golden/make_golden_radial_norms.py     # writes tests/golden/radial_norms/<case>.npz

The study files (experiments/mnist/mnist_digits_minimal_radial_{weilbul,exponential,chi,chi2,radialdists}.yaml) put
``torch.distributions.Weibull`` / ``Exponential`` / ``Chi2`` / ``HalfNormal`` and the reference's own ``Chi``
(distributions.py:55-115) under ``RadialDistribution``, their parameters written as Python floats or host tensors;
``WeibullMM`` (distributions.py:835-850) is the trainable mixture.  Cases:

* image ``[16,7,7]``, 2 blocks, the live conditioner (make_golden_image_radial.py), ``WeibullMM`` x 3, p = 1
* flat D = 7, 3 blocks, ``Weibull(scale, 1.5)`` as the study file writes it, p = 2
* flat D = 16, 3 blocks, ``HalfNormal``, p = inf;  flat D = 16, 3 blocks, ``Chi``, p = 2
* flat D = 7, 3 blocks, ``Chi2``, p = 1;  flat D = 7, 3 blocks, ``Exponential``, p = 1

The flat flows are the live flat configuration's (make_golden_gaussian_mixture.py: DenseNN [32, 32] + ReLU, lu_transform 1,
householder 0, affine_conjugation, prior_scale 1.0) as drawn under the case's seed with its conditioned LU factors; the radius
distribution's parameters are set from the median latent radius of the case's inputs (a base far from the latents gives a
density of -1e6 that tests nothing) and stored in the spec.  Per case: inputs, ``log_prob`` / ``backward`` / ``_forward`` in
fp32 and fp64, and the fp64 gradients of ``Flow.fit``'s loss ``-log_prob(x).mean() - log_prior()`` w.r.t. EVERY parameter,
base included.  One fit case (image, ``WeibullMM``): 2 epochs x 96 rows, batch 32, SophiaG at the live hyper-parameters, as
``imageradialfit_*``.  One ``chi_grid`` file: ``Chi(df, scale)``'s ``log_prob`` / ``cdf`` / ``entropy`` on a grid, fp64.
Data only."""
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ref_shim  # noqa: E402

flows, transforms, networks, distributions = ref_shim.install()
from pyro.nn import DenseNN  # noqa: E402  (the shim's restatement)
from image_synth import synth_image_params_  # noqa: E402

OUT = os.path.join(HERE, "radial_norms")
LIVE_COND = dict(c_hidden=32, num_layers=3, padding="same", kernel_size=3, normalize_layers=True, gating=True)
LR, NP_SEED, N_ROWS, BATCH, EPOCHS = 1e-3, 5, 96, 32, 2


def make_norm(norm):
    """the radius distribution from its spec entry, constructor call for constructor call (Python floats stay floats)"""
    kind = norm["kind"]
    if kind == "weibullmm":
        return distributions.WeibullMM(scale=torch.tensor(norm["scale"]), concentration=torch.tensor(norm["concentration"]),
                                       mixture_weights=torch.tensor(norm["mixture_weights"]), device="cpu")
    if kind == "weibull":
        return torch.distributions.weibull.Weibull(concentration=norm["concentration"], scale=1.0 * norm["scale"])
    if kind == "halfnormal":
        return torch.distributions.HalfNormal(scale=norm["scale"])
    if kind == "chi":
        return distributions.Chi(df=torch.Tensor([norm["df"]]), scale=norm["scale"])       # (df as the study file writes it)
    if kind == "chi2":
        return torch.distributions.chi2.Chi2(df=torch.Tensor([norm["df"]]))
    if kind == "exponential":
        return torch.distributions.Exponential(rate=norm["rate"])
    raise KeyError(kind)


def build(spec, norm):
    dims = list(spec["in_dims"])
    torch.manual_seed(spec["seed"])
    base = distributions.RadialDistribution(device="cpu", p=float(spec["p"]), loc=torch.zeros(dims), norm_distribution=make_norm(norm))
    if len(dims) == 3:
        flow = flows.USFlow(base, dims, spec["coupling_blocks"], networks.ConvNet2D, dict(LIVE_COND, c_in=dims[0]), prior_scale=1.0,
                            lu_transform=1, householder=0, affine_conjugation=True, nonlinearity=torch.nn.ReLU())
        synth_image_params_(flow, spec["seed"])
    else:
        D = dims[0]
        flow = flows.USFlow(base_distribution=base, in_dims=[D], coupling_blocks=spec["coupling_blocks"], conditioner_cls=DenseNN,
                            conditioner_args=dict(input_dim=D, hidden_dims=[32, 32], param_dims=[D]), soft_training=False,
                            training_noise_prior=torch.distributions.Uniform(1e-20, 0.01), prior_scale=1.0, lu_transform=1,
                            householder=0, affine_conjugation=True, nonlinearity=torch.nn.ReLU())
        # the default initialisation is badly conditioned through the chain of affine layers (latent radii of thousands): the
        # conditioning transform of make_golden_gaussian_mixture.py on the LU factors, everything else as drawn
        g = torch.Generator().manual_seed(spec["seed"])
        alpha = 0.1
        with torch.no_grad():
            for name, q in flow.named_parameters():
                if name.endswith("L_raw"):
                    q.copy_(torch.eye(D) + alpha * q.tril(-1))
                elif name.endswith("U_raw"):
                    sign = torch.where(q.diagonal() < 0, -1.0, 1.0)
                    q.copy_(alpha * q.triu(1) + torch.diag(sign * (0.75 + 0.5 * torch.rand(D, generator=g))))
    if spec.get("loc_noise"):
        with torch.no_grad():
            flow.base_distribution.loc.copy_(spec["loc_noise"] * torch.randn(flow.base_distribution.loc.shape,
                                                                            generator=torch.Generator().manual_seed(spec["seed"])))
    return flow


def inputs(spec, n):
    g = torch.Generator().manual_seed(1000 + spec["seed"])
    dims = spec["in_dims"]
    if len(dims) == 3:
        return torch.rand(n, *dims, generator=g), 0.5 * torch.randn(n, *dims, generator=g)
    comp = (torch.rand(n, generator=g) < 0.5).float()[:, None] * 2 - 1
    return comp * torch.ones(dims[0]) + 0.5 * torch.randn(n, dims[0], generator=g), 0.7 * torch.randn(n, dims[0], generator=g)


def median_radius(spec, x):
    """median ||backward(x) - loc||_p of the case's inputs (the layers do not depend on the base)"""
    flow = build(spec, dict(kind="halfnormal", scale=1.0))
    with torch.no_grad():
        z = (flow.backward(x) - flow.base_distribution.loc).flatten(1)
    return float(z.norm(p=float(spec["p"]), dim=1).median())


def norm_for(kind, m, seed, dim):
    """parameters near the latent radii, rounded so that the JSON spec reproduces them exactly"""
    m = round(m, 3)
    if kind == "weibullmm":
        # (MixtureModel stores positive parameters through utils.inv_softplus = log(exp(x) - 1), which overflows in fp32 beyond
        # x = 88: the scales stay below that, whatever the latent radii are)
        g = torch.Generator().manual_seed(seed)
        return dict(kind=kind, scale=[round(min(m, 85.0) * (0.65 + 0.175 * i), 3) for i in range(3)],
                    concentration=[round(v, 3) for v in (1.0 + torch.rand(3, generator=g)).tolist()],
                    mixture_weights=[round(v, 3) for v in torch.randn(3, generator=g).tolist()])
    if kind == "weibull":
        return dict(kind=kind, scale=m, concentration=1.5)
    if kind == "halfnormal":
        return dict(kind=kind, scale=m)
    if kind == "chi":
        return dict(kind=kind, df=float(dim), scale=round(m / math.sqrt(dim), 3))
    if kind == "chi2":
        return dict(kind=kind, df=m)
    if kind == "exponential":
        return dict(kind=kind, rate=round(1.0 / m, 4))
    raise KeyError(kind)


def to64(flow):
    f64 = flow.double()
    for l in f64.layers:
        if isinstance(l, transforms.MaskedCoupling):
            l.mask = l.mask.double()
    return f64


def run_case(name, in_dims, K, kind, seed, p, n=12, loc_noise=0.05):
    if len(sys.argv) > 1 and name not in sys.argv[1:]:
        return
    spec = dict(in_dims=list(in_dims), coupling_blocks=K, seed=seed, p=("inf" if p == math.inf else p), loc_noise=loc_noise,
                cond_args=LIVE_COND, prior_scale=1.0)
    x, zin = inputs(spec, n)
    spec["norm"] = norm = norm_for(kind, median_radius(spec, x), seed, math.prod(in_dims))
    flow = build(spec, norm)
    sd = {k: v.detach().clone() for k, v in flow.state_dict().items()
          if len(in_dims) == 1 or k.startswith("base_distribution.")}          # (image layers: regenerated from the seed)
    out = {}
    with torch.no_grad():
        out["log_prob32"], out["backward32"], out["forward32"] = flow.log_prob(x), flow.backward(x), flow._forward(zin)
    torch.set_default_dtype(torch.float64)
    try:
        # (the plain distributions are rebuilt under the fp64 default so that their float parameters are fp64 tensors)
        f64 = to64(build(spec, norm)) if len(in_dims) == 1 else to64(flow)
        if len(in_dims) == 1:
            f64.load_state_dict({k: v.double() for k, v in sd.items()})
        with torch.no_grad():
            out["log_prob64"], out["backward64"], out["forward64"] = f64.log_prob(x.double()), f64.backward(x.double()), f64._forward(zin.double())
        for q in f64.parameters():
            q.grad = None
        lp = f64.log_prob(x.double())
        prior = f64.log_prior()
        loss = -lp.mean() - prior
        loss.backward()
        out["loss64"] = loss.detach()
        out["log_prior64"] = torch.as_tensor(float(prior), dtype=torch.float64)
        grads = {k: q.grad.detach().clone() for k, q in f64.named_parameters() if q.grad is not None}
    finally:
        torch.set_default_dtype(torch.float32)
    arrays = {"x": x.numpy(), "zin": zin.numpy()}
    arrays.update({k: v.detach().numpy() for k, v in out.items()})
    arrays.update({"sd/" + k: v.float().numpy() for k, v in sd.items()})
    arrays.update({"g/" + k: v.numpy() for k, v in grads.items()})
    arrays["spec"] = np.array(json.dumps(spec))
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    rel = (out["log_prob32"].double() - out["log_prob64"]).abs() / out["log_prob64"].abs()
    r = (out["backward64"] - f64.base_distribution.loc.detach()).flatten(1).norm(p=float(p), dim=1)
    print(f"{name:40s} logp[0]={out['log_prob64'][0].item():+.6e} ref32-vs-64 {rel.max().item():.2e} r in [{r.min().item():.4g}, "
          f"{r.max().item():.4g}] {json.dumps(norm)} {len(grads)} grads {os.path.getsize(path) / 1024:.0f} KB")


def fit_case(name, in_dims, K, kind, seed):
    if len(sys.argv) > 1 and name not in sys.argv[1:]:
        return
    spec = dict(in_dims=list(in_dims), coupling_blocks=K, seed=seed, p=1.0, loc_noise=0.0, cond_args=LIVE_COND, prior_scale=1.0)
    data = torch.rand(N_ROWS, *in_dims, generator=torch.Generator().manual_seed(77))
    spec["norm"] = norm = norm_for(kind, median_radius(spec, data), seed, math.prod(in_dims))
    flow = build(spec, norm)
    bsd = {k: v.detach().clone() for k, v in flow.state_dict().items() if k.startswith("base_distribution.")}
    ds = torch.utils.data.TensorDataset(data, torch.zeros(N_ROWS))
    np.random.seed(NP_SEED)
    losses = flow.fit(ds, optim_params=dict(lr=LR, weight_decay=0.0), batch_size=BATCH, shuffle=True, device=torch.device("cpu"),
                      epochs=EPOCHS)
    arrays = {"losses": np.array(losses, dtype=np.float64), "data": data.numpy(), "spec": np.array(json.dumps(spec))}
    arrays.update({"sd0/" + k: v.numpy() for k, v in bsd.items()})
    for k, v in flow.state_dict().items():
        arrays["sd/" + k] = v.detach().numpy()
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"{name:40s} epoch losses {losses}  {os.path.getsize(path) / 1024:.0f} KB")


def chi_grid(name="chi_grid"):
    """the reference's Chi on a grid, fp64 (its constants are built under the fp64 default dtype)"""
    if len(sys.argv) > 1 and name not in sys.argv[1:]:
        return
    torch.set_default_dtype(torch.float64)
    try:
        arrays = {}
        cases = [(1.0, 1.0), (3.0, 0.5), (7.5, 2.0), (16.0, 1.3), (64.0, 0.07)]
        arrays["df"] = np.array([c[0] for c in cases])
        arrays["scale"] = np.array([c[1] for c in cases])
        for i, (df, scale) in enumerate(cases):
            d = distributions.Chi(torch.Tensor([df]), scale)
            r = scale * math.sqrt(df) * torch.linspace(0.05, 3.0, 40)
            arrays[f"r/{i}"] = r.numpy()
            arrays[f"log_prob/{i}"] = d.log_prob(r).numpy()
            arrays[f"cdf/{i}"] = d.cdf(r).numpy()
            arrays[f"entropy/{i}"] = d.entropy().numpy()
    finally:
        torch.set_default_dtype(torch.float32)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"{name:40s} {os.path.getsize(path) / 1024:.0f} KB")


def main():
    os.makedirs(OUT, exist_ok=True)
    run_case("grads_image_c16_7x7_k2_weibullmm3_p1", (16, 7, 7), 2, "weibullmm", 71, 1.0, n=10)
    run_case("grads_flat_d7_k3_weibull_p2", (7,), 3, "weibull", 72, 2.0)
    run_case("grads_flat_d16_k3_halfnormal_pinf", (16,), 3, "halfnormal", 73, math.inf)
    run_case("grads_flat_d16_k3_chi_p2", (16,), 3, "chi", 74, 2.0)
    run_case("grads_flat_d7_k3_chi2_p1", (7,), 3, "chi2", 75, 1.0)
    run_case("grads_flat_d7_k3_exponential_p1", (7,), 3, "exponential", 76, 1.0)
    fit_case("fit_image_c16_7x7_k2_weibullmm3", (16, 7, 7), 2, "weibullmm", 77)
    chi_grid()


if __name__ == "__main__":
    main()
