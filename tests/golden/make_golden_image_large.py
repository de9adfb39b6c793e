"""Golden vectors of image-shaped flows whose feature maps have MORE than 256 pixels -- the reference's dataset classes without
space-to-depth (explib/datasets.py: ``space_to_depth_factor: int = 1``; MNIST [1, 28, 28], CIFAR [3, 32, 32]) -- from the REAL
reference (this container only).

    python tests/golden/make_golden_image_large.py     # rewrites tests/golden/image_large/*.npz

Cases, parameters from tests/image_synth.py (a pure function of the seed and the module tree, which the mirror shares key for
key: no state dict is stored):
  (a) imagelarge_mnist_c1_28x28    [1, 28, 28]: ConvNet2D(c_in=1, c_hidden=32, num_layers=2, kernel_size=3, padding="same", gating,
                                   layer norm), 2 blocks, Householder 1, conjugation, Laplace base (make_golden_conv5.run_plain's recipe);
  (b) imagelarge_cifar_c3_32x32    [3, 32, 32]: the same conditioner at c_in=3 in the live configurations' flow (lu_transform 1,
                                   conjugation, prior_scale 1.0) over RadialDistribution(p=1, LogNormal(6, .35), image-shaped loc),
                                   2 rows, 1 block -- with 2 blocks the reference's own fp32-against-fp64 gap is 1.06e-6, above
                                   the 1e-6 the rule below allows (make_golden_image_radial's recipe);
  (c) imagelarge_cond_c2_17x17     [2, 17, 17]: CondConvNet2D(c_hidden=16, num_layers=1), soft-training context, with a per-row
                                   context and with the implicit zero context (make_golden_cond_image.run_case).
Stored per case: the inputs, log_prob in fp32 and fp64, the layer loop's backward and forward in fp64.  main() prints the
reference's own fp32-against-fp64 gap of log_prob per case; the tests hold the device to 1e-5 of the fp64 run, so a case whose
own gap exceeds 1e-6 would get a milder synth scale or one block fewer, never a wider bound.  Data only."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "image_large")
sys.path.insert(0, HERE)

import make_golden_cond_image as mgc  # noqa: E402  (imports the reference through ref_shim; its main() is not run)

flows, transforms, networks, distributions = mgc.flows, mgc.transforms, mgc.networks, mgc.distributions


def cond_args(c_in):
    return dict(c_in=c_in, c_hidden=32, num_layers=2, kernel_size=3, padding="same", normalize_layers=True, gating=True)


def _save(name, arrays, spec, lp32, lp64):
    arrays = {k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in arrays.items()}
    arrays["spec"] = np.array(json.dumps(spec))
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    rel = ((lp32.double() - lp64).abs() / lp64.abs()).max().item()
    print(f"{name:32s} logp[0]={lp64[0].item():+.6e} ref32-vs-64 {rel:.2e} {'ok' if rel <= 1e-6 else 'TOO LARGE'}  "
          f"{os.path.getsize(path) / 1024:.0f} KB")


def _double_masks(f64):
    for l in f64.layers:
        if isinstance(l, transforms.MaskedCoupling):
            l.mask = l.mask.double()
    return f64


def run_laplace(name, dims, seed, n=4):
    """(a): the unconditional flow over a Laplace base"""
    from image_synth import synth_image_params_
    spec = dict(in_dims=list(dims), coupling_blocks=2, cond_cls="ConvNet2D", cond_args=cond_args(dims[0]), householder=1,
                affine_conjugation=True, seed=seed, base="laplace")
    torch.manual_seed(seed)
    flow = flows.USFlow(torch.distributions.Laplace(torch.zeros(dims), torch.ones(dims)), list(dims), 2, networks.ConvNet2D,
                        dict(spec["cond_args"]), householder=1, affine_conjugation=True)
    synth_image_params_(flow, seed)
    g = torch.Generator().manual_seed(2000 + seed)
    x = torch.rand(n, *dims, generator=g)
    zin = torch.distributions.Laplace(0.0, 1.0).icdf(torch.rand(n, *dims, generator=g) * 0.998 + 0.001)
    out = {"x": x, "zin": zin}
    with torch.no_grad():
        out["log_prob32"] = flow.log_prob(x)
    torch.set_default_dtype(torch.float64)
    try:
        f64 = _double_masks(flow.double())
        f64.base_distribution = distributions.Independent(
            torch.distributions.Laplace(torch.zeros(dims).double(), torch.ones(dims).double()), len(dims))
        with torch.no_grad():
            out["log_prob64"] = f64.log_prob(x.double())
            out["backward64"], out["forward64"] = f64.backward(x.double()), f64._forward(zin.double())
    finally:
        torch.set_default_dtype(torch.float32)
    _save(name, out, spec, out["log_prob32"], out["log_prob64"])


def run_radial(name, dims, seed, K, n=2):
    """(b): the live configurations' flow and base (make_golden_image_radial.build), the conditioner two layers deep"""
    from image_synth import synth_image_params_
    spec = dict(in_dims=list(dims), coupling_blocks=K, base="lognormal", seed=seed, p=1.0, cond_args=cond_args(dims[0]), prior_scale=1.0)
    torch.manual_seed(seed)
    nd = distributions.LogNormal(loc=torch.ones([1]) * 6, scale=torch.ones([1]) * .35, device="cpu")
    base = distributions.RadialDistribution(device="cpu", p=1.0, loc=torch.zeros(list(dims)), norm_distribution=nd)
    flow = flows.USFlow(base, list(dims), K, networks.ConvNet2D, dict(spec["cond_args"]), prior_scale=1.0, lu_transform=1, householder=0,
                        affine_conjugation=True, nonlinearity=torch.nn.ReLU())
    synth_image_params_(flow, seed)
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.rand(n, *dims, generator=g)
    zin = 0.5 * torch.randn(n, *dims, generator=g)       # (the reference's radial sample() raises for an image-shaped loc)
    out = {"x": x, "zin": zin}
    with torch.no_grad():
        out["log_prob32"] = flow.log_prob(x)
    torch.set_default_dtype(torch.float64)
    try:
        f64 = _double_masks(flow.double())
        with torch.no_grad():
            out["log_prob64"] = f64.log_prob(x.double())
            out["backward64"], out["forward64"] = f64.backward(x.double()), f64._forward(zin.double())
    finally:
        torch.set_default_dtype(torch.float32)
    _save(name, out, spec, out["log_prob32"], out["log_prob64"])


def main():
    run_laplace("imagelarge_mnist_c1_28x28", (1, 28, 28), 61)
    # (with 2 blocks the reference's own fp32 run of this case is 1.06e-6 from its fp64 run: one block fewer, 1 block)
    run_radial("imagelarge_cifar_c3_32x32", (3, 32, 32), 62, K=1)
    mgc.OUT = OUT
    mgc.run_case("imagelarge_cond_c2_17x17", (2, 17, 17), 2, "CondConvNet2D",
                 dict(c_in=2, c_hidden=16, num_layers=1, padding="same", kernel_size=3, normalize_layers=False, gating=False), 63,
                 store_grads=False)


if __name__ == "__main__":
    main()
