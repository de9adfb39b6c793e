"""Golden vectors of image-shaped flows whose conditioners use 5 x 5 convolutions, from the REAL reference (this container
only) -- the models experiments/mnist/mnist_usflow_hyperopt.yaml draws at ``kernel_size: 5``.

    python tests/golden/make_golden_conv5.py     # rewrites tests/golden/conv5/conv5_*.npz

Cases, all at [16, 7, 7] with 2 coupling blocks, Laplace base, parameters from tests/image_synth.py (a pure function of the seed
and the module tree, which the mirror shares key for key: no state dict is stored):
  (a) conv5_cond_c32   CondConvNet2D(c_in=16, c_hidden=32, num_layers=2, kernel_size=5, padding="same", gating, layer norm),
                       Householder 1, conjugation, soft-training context -- the inner convolutions' weights fit the LDS in part;
  (b) conv5_cond_c64   the same with c_hidden=64: every inner convolution streams its weights;
  (c) conv5_plain_c8   an unconditional ConvNet2D, c_hidden=8.
Stored per case, as tests/golden/make_golden_cond_image.py stores them (its ``run_case`` makes (a) and (b)): log_prob in fp32 and
fp64, the layer loop's backward and forward in fp64, with a per-row context and with the implicit zero context, the fp64 loss,
and EVERY parameter's gradient of -mean(log_prob) from the reference's fp64 run, rounded to fp32 as that generator rounds them.
The gradients live beside the case in ``<case>_grads<i>.npz``, split so that no file exceeds 400 KB (a 64 -> 64 channel 5 x 5
weight alone is 400 KB as fp32; the largest fixture in tests/golden/cond/ is 445 KB).

The ``fit`` run (conv5_fit_plain_c16.npz): the recipe of make_golden_image_wide.fit_run (SGD, 96 rows drawn from seed 77, batch 32,
shuffle under numpy seed 5, 2 epochs, fp32 on the CPU as the reference runs it) on the UNCONDITIONAL flow of (c) at c_hidden=16.
Not on (a): a soft-trained flow draws its noise and context from torch's generator inside ``fit``, and the CPU generator's
draws are not the device generator's, so no device run can follow the reference's CPU run of (a) step by step (the conditional
3 x 3 flows' fit test compares with torch autograd on the same GPU for the same reason).  The rows are regenerated from the seed,
the file holds the epoch losses, the learning rate and the final state dict.  Learning rate: the first of 1e-3, 1e-4, 1e-5 at which
the reference determines the run -- its fp32 run within a tenth of the test's bounds of its own fp64 run (losses 2e-5, parameters
2e-4 of the tensor's largest entry, updates 2e-3 of the update's largest entry), the rule of make_golden_image_wide.py; main()
measures and prints the figures.  Data only."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "conv5")
sys.path.insert(0, HERE)

import make_golden_cond_image as mgc  # noqa: E402  (imports the reference through ref_shim; its main() is not run)

flows, transforms, networks, distributions = mgc.flows, mgc.transforms, mgc.networks, mgc.distributions
DIMS = (16, 7, 7)


def cond_args(c_hidden):
    return dict(c_in=16, c_hidden=c_hidden, num_layers=2, kernel_size=5, padding="same", normalize_layers=True, gating=True)


def run_plain(name, c_hidden, seed, n=4):
    """the unconditional case: ConvNet2D, no soft training"""
    from image_synth import synth_image_params_
    spec = dict(in_dims=list(DIMS), coupling_blocks=2, cond_cls="ConvNet2D", cond_args=cond_args(c_hidden), householder=1,
                affine_conjugation=True, seed=seed)
    torch.manual_seed(seed)
    flow = flows.USFlow(torch.distributions.Laplace(torch.zeros(DIMS), torch.ones(DIMS)), list(DIMS), 2, networks.ConvNet2D,
                        dict(spec["cond_args"]), householder=1, affine_conjugation=True)
    synth_image_params_(flow, seed)
    g = torch.Generator().manual_seed(2000 + seed)
    x = torch.rand(n, *DIMS, generator=g)
    zin = torch.distributions.Laplace(0.0, 1.0).icdf(torch.rand(n, *DIMS, generator=g) * 0.998 + 0.001)
    out = {}
    with torch.no_grad():
        out["log_prob32"] = flow.log_prob(x)
    torch.set_default_dtype(torch.float64)
    try:
        f64 = flow.double()
        for l in f64.layers:
            if isinstance(l, transforms.MaskedCoupling):
                l.mask = l.mask.double()
        f64.base_distribution = distributions.Independent(
            torch.distributions.Laplace(torch.zeros(DIMS).double(), torch.ones(DIMS).double()), len(DIMS))
        with torch.no_grad():
            out["log_prob64"] = f64.log_prob(x.double())
            out["backward64"], out["forward64"] = f64.backward(x.double()), f64._forward(zin.double())
            out["loss64"] = -out["log_prob64"].mean()
    finally:
        torch.set_default_dtype(torch.float32)
    arrays = {"x": x.numpy(), "zin": zin.numpy(), "spec": np.array(json.dumps(spec))}
    arrays.update({k: v.detach().numpy() for k, v in out.items()})
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    rel = ((out["log_prob32"].double() - out["log_prob64"]).abs() / out["log_prob64"].abs()).max().item()
    print(f"{name:40s} logp[0]={out['log_prob64'][0].item():+.6e} ref32-vs-64 {rel:.2e}  {os.path.getsize(path) / 1024:.0f} KB")


GRAD_FILE_BYTES = 400 * 1024
FIT_NAME, FIT_HIDDEN, FIT_SEED, FIT_ROWS, FIT_DATA_SEED, NP_SEED = "conv5_fit_plain_c16", 16, 54, 96, 77, 5


def plain_grads64(name, c_hidden, seed):
    """the fp64 gradients of the unconditional case into its file as g/<parameter> (run_case stores them for the conditional ones)"""
    from image_synth import synth_image_params_
    path = os.path.join(OUT, name + ".npz")
    z = dict(np.load(path))
    torch.manual_seed(seed)
    flow = flows.USFlow(torch.distributions.Laplace(torch.zeros(DIMS), torch.ones(DIMS)), list(DIMS), 2, networks.ConvNet2D,
                        cond_args(c_hidden), householder=1, affine_conjugation=True)
    synth_image_params_(flow, seed)
    torch.set_default_dtype(torch.float64)
    try:
        f64 = _double(flow)
        lp = f64.log_prob(torch.from_numpy(z["x"]).double())
        assert float((lp.detach() - torch.from_numpy(z["log_prob64"])).abs().max()) < 1e-9
        (-lp.mean()).backward()
        for k, q in f64.named_parameters():
            if q.grad is not None:
                z["g/" + k] = q.grad.detach().float().numpy()
    finally:
        torch.set_default_dtype(torch.float32)
    np.savez_compressed(path, **z)


def _double(flow):
    f64 = flow.double()
    for l in f64.layers:
        if isinstance(l, transforms.MaskedCoupling):
            l.mask = l.mask.double()
    f64.base_distribution = distributions.Independent(
        torch.distributions.Laplace(torch.zeros(DIMS).double(), torch.ones(DIMS).double()), len(DIMS))
    return f64


def split_grads(name):
    """move the g/<parameter> arrays of a case into <case>_grads<i>.npz files of at most GRAD_FILE_BYTES of fp32 each"""
    path = os.path.join(OUT, name + ".npz")
    z = dict(np.load(path))
    grads = {k: z.pop(k) for k in list(z) if k.startswith("g/")}
    np.savez_compressed(path, **z)
    chunks, cur, size = [], {}, 0
    for k, v in grads.items():
        if cur and size + v.nbytes > GRAD_FILE_BYTES:
            chunks.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += v.nbytes
    chunks.append(cur)
    for i, c in enumerate(chunks):
        np.savez_compressed(os.path.join(OUT, f"{name}_grads{i}.npz"), **c)
    sizes = [os.path.getsize(os.path.join(OUT, f"{name}_grads{i}.npz")) // 1024 for i in range(len(chunks))]
    print(f"{name}: {len(grads)} gradients in {len(chunks)} files of {sizes} KB")


def fit_run(lr, double):
    from image_synth import synth_image_params_
    torch.manual_seed(FIT_SEED)
    flow = flows.USFlow(torch.distributions.Laplace(torch.zeros(DIMS), torch.ones(DIMS)), list(DIMS), 2, networks.ConvNet2D,
                        cond_args(FIT_HIDDEN), householder=1, affine_conjugation=True)
    synth_image_params_(flow, FIT_SEED)
    sd0 = {k: v.detach().double().clone() for k, v in flow.state_dict().items()}
    data = torch.rand(FIT_ROWS, *DIMS, generator=torch.Generator().manual_seed(FIT_DATA_SEED))
    rows = data
    try:
        if double:
            torch.set_default_dtype(torch.float64)
            flow = _double(flow)
            rows = data.double()
        ds = torch.utils.data.TensorDataset(rows, torch.zeros(FIT_ROWS))
        np.random.seed(NP_SEED)
        losses = flow.fit(ds, optim=torch.optim.SGD, optim_params=dict(lr=lr), batch_size=32, shuffle=True, device=torch.device("cpu"),
                          epochs=2)
    finally:
        torch.set_default_dtype(torch.float32)
    return [float(v) for v in losses], {k: v.detach().clone() for k, v in flow.state_dict().items()}, sd0


def fit_fixture():
    for lr in (1e-3, 1e-4, 1e-5):
        l32, sd32, sd0 = fit_run(lr, False)
        l64, sd64, _ = fit_run(lr, True)
        el = max(abs(a - b) / abs(b) for a, b in zip(l32, l64))
        ep = eu = 0.0
        for k, v in sd64.items():
            if not v.is_floating_point():
                continue
            d = float((sd32[k].double() - v.double()).abs().max())
            ep = max(ep, d / max(float(v.abs().max()), 1e-3))
            up = float((v.double() - sd0[k]).abs().max())
            if up > 0:
                eu = max(eu, d / up)
        ok = el <= 2e-5 and ep <= 2e-4 and eu <= 2e-3
        print(f"fit lr {lr:g}: reference fp32 vs fp64: losses {el:.1e}, parameters {ep:.1e}, updates {eu:.1e} -> {'kept' if ok else 'next'}")
        if ok:
            break
    else:
        raise SystemExit("the reference determines the run at none of the learning rates")
    spec = dict(in_dims=list(DIMS), coupling_blocks=2, cond_cls="ConvNet2D", cond_args=cond_args(FIT_HIDDEN), householder=1,
                affine_conjugation=True, seed=FIT_SEED, rows=FIT_ROWS, data_seed=FIT_DATA_SEED, np_seed=NP_SEED)
    arrays = {"losses": np.array(l32, dtype=np.float64), "lr": np.array(lr), "spec": np.array(json.dumps(spec))}
    arrays.update({"sd/" + k: v.numpy() for k, v in sd32.items()})
    path = os.path.join(OUT, FIT_NAME + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"fit: epoch losses {l32}  {os.path.getsize(path) / 1024:.0f} KB")


def main():
    mgc.OUT = OUT
    mgc.run_case("conv5_cond_c32", DIMS, 2, "CondConvNet2D", cond_args(32), 51)
    mgc.run_case("conv5_cond_c64", DIMS, 2, "CondConvNet2D", cond_args(64), 52)
    run_plain("conv5_plain_c8", 8, 53)
    plain_grads64("conv5_plain_c8", 8, 53)
    for name in ("conv5_cond_c32", "conv5_cond_c64", "conv5_plain_c8"):
        split_grads(name)
    fit_fixture()


if __name__ == "__main__":
    main()
