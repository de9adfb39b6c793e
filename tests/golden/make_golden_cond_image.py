"""Golden vectors of CONDITIONAL image-shaped flows from the REAL reference (this container only): ``USFlow`` with the
``CondConvNet2D`` / spatial ``CondConvNet`` conditioners (networks.py:513-680), soft-trained (flows.py:551-566), the
per-row context appended as one more input channel.

    python tests/golden/make_golden_cond_image.py     # rewrites tests/golden/cond/*.npz

Cases: (a) the model of experiments/mnist/mnist_usflow_minimal.yaml:41-82 -- CondConvNet2D, c_hidden 32, one plain layer,
householder 1, conjugated (its ``rescale_hidden: 1`` is dropped: the reference's ConvNet2D does not accept it); (b) the live
MNIST conditioner (gated, layer norm, 3 layers) as CondConvNet2D at K = 2; (c) a spatial CondConvNet at [16, 7, 7]; (d) one
CIFAR-shaped [48, 8, 8] case.  Laplace base.  Parameters: tests/image_synth.py (a pure function of the seed and the module
tree, which the mirror shares key for key), so no state dict is stored.  Stored (fp32 and fp64 runs): log_prob, the layer
loop's backward and forward with a non-zero per-row context (``*_ctx``) and with the implicit zero context (``*_noctx``), and
every parameter's gradient of -mean(log_prob(x, ctx)) from the fp64 run (rounded to fp32; not for the CIFAR case: the
files stay under 500 KB).  Data only.  (The files live in a sub-directory: the fixture globs of tests/golden_util.py do not
pick them up.)"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "cond")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden_image as mgi  # noqa: E402  (imports the reference through ref_shim; main() is not run)

flows, transforms, networks, distributions = mgi.flows, mgi.transforms, mgi.networks, mgi.distributions


def build(spec):
    torch.manual_seed(spec["seed"])
    in_dims = spec["in_dims"]
    base = torch.distributions.Laplace(torch.zeros(in_dims), torch.ones(in_dims))
    cls = getattr(networks, spec["cond_cls"])
    flow = flows.USFlow(base, list(in_dims), spec["coupling_blocks"], cls, dict(spec["cond_args"]), householder=spec["householder"],
                        affine_conjugation=spec["affine_conjugation"], soft_training=True)
    from image_synth import synth_image_params_
    synth_image_params_(flow, spec["seed"])
    return flow


def run_layers(flow, x, context, inverse):
    for layer in (reversed(flow.layers) if inverse else flow.layers):
        x = layer.backward(x, context) if inverse else layer.forward(x, context)
    return x


def run_case(name, in_dims, K, cond_cls, cond_args, seed, hh=1, conj=True, n=4, store_grads=True):
    if len(sys.argv) > 1 and name not in sys.argv[1:]:
        return
    spec = dict(in_dims=list(in_dims), coupling_blocks=K, cond_cls=cond_cls, cond_args=cond_args, householder=hh,
                affine_conjugation=conj, seed=seed)
    flow = build(spec)
    g = torch.Generator().manual_seed(2000 + seed)
    x = torch.rand(n, *in_dims, generator=g)
    zin = torch.distributions.Laplace(0.0, 1.0).icdf(torch.rand(n, *in_dims, generator=g) * 0.998 + 0.001)
    ctx = 2.0 * torch.rand(n, 1, generator=g)                  # SoftFlow's conditioning scale: noise * 2 / high in [0, 2]
    out = {}
    with torch.no_grad():
        out["log_prob32_ctx"], out["log_prob32_noctx"] = flow.log_prob(x, ctx), flow.log_prob(x)
    torch.set_default_dtype(torch.float64)
    try:
        f64 = flow.double()
        for l in f64.layers:
            if isinstance(l, transforms.MaskedCoupling):
                l.mask = l.mask.double()
        f64.base_distribution = distributions.Independent(
            torch.distributions.Laplace(torch.zeros(in_dims).double(), torch.ones(in_dims).double()), len(in_dims))
        xd, zd, cd = x.double(), zin.double(), ctx.double()
        with torch.no_grad():
            out["log_prob64_ctx"], out["log_prob64_noctx"] = f64.log_prob(xd, cd), f64.log_prob(xd)
            out["backward64_ctx"], out["forward64_ctx"] = run_layers(f64, xd, cd, True), run_layers(f64, zd, cd, False)
            out["backward64_noctx"] = run_layers(f64, xd, torch.zeros(n, 1), True)
        for q in f64.parameters():
            q.grad = None
        loss = -f64.log_prob(xd, cd).mean()
        loss.backward()
        out["loss64"] = loss.detach()
        grads = {k: q.grad.detach().clone() for k, q in f64.named_parameters() if q.grad is not None}
    finally:
        torch.set_default_dtype(torch.float32)
    arrays = {"x": x.numpy(), "zin": zin.numpy(), "ctx": ctx.numpy()}
    arrays.update({k: v.detach().numpy() for k, v in out.items()})
    if store_grads:
        arrays.update({"g/" + k: v.float().numpy() for k, v in grads.items()})
    arrays["spec"] = np.array(json.dumps(spec))
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    rel = (out["log_prob32_ctx"].double() - out["log_prob64_ctx"]).abs() / out["log_prob64_ctx"].abs()
    dctx = (out["log_prob64_ctx"] - out["log_prob64_noctx"]).abs().max().item()
    print(f"{name:40s} logp[0]={out['log_prob64_ctx'][0].item():+.6e} ref32-vs-64 {rel.max().item():.2e} "
          f"|ctx effect| {dctx:.3g}  {len(grads)} grads  {os.path.getsize(path) / 1024:.0f} KB")


def main():
    # (a) mnist_usflow_minimal.yaml:41-82 (padding 1, no gating, no layer norm)
    run_case("condimage_minimal_c16_7x7_k1_plain_hh1_conj", (16, 7, 7), 1, "CondConvNet2D",
             dict(c_in=16, c_hidden=32, num_layers=1, padding=1, normalize_layers=False, gating=False), 41)
    # (b) the live MNIST conditioner (tests/explib/mnist.yaml:44-77) as CondConvNet2D
    run_case("condimage_mnistcfg_c16_7x7_k2_gated_ln_hh1_conj", (16, 7, 7), 2, "CondConvNet2D",
             dict(c_in=16, c_hidden=32, num_layers=3, padding="same", kernel_size=3, normalize_layers=True, gating=True), 42)
    # (c) the spatial CondConvNet (networks.py:513-592)
    run_case("condimage_convnet_c16_7x7_k2_gated_ln_hh0", (16, 7, 7), 2, "CondConvNet",
             dict(in_dims=[16, 7, 7], c_hidden=[32, 32], c_out=16, kernel_size=3, normalize_layers=True, gating=True), 43,
             hh=0, conj=False)
    # (d) CIFAR-shaped (experiments/cifar/cifar.yaml:56-77 with 2 coupling blocks)
    run_case("condimage_cifarcfg_c48_8x8_k2_gated_ln_hh1_conj", (48, 8, 8), 2, "CondConvNet2D",
             dict(c_in=48, c_hidden=32, num_layers=3, padding="same", kernel_size=3, normalize_layers=True, gating=True), 44,
             n=3, store_grads=False)


if __name__ == "__main__":
    main()
