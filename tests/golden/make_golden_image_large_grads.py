"""Golden fp64 gradients and a golden ``Flow.fit`` run of image-shaped flows whose feature maps have MORE than 256 pixels, from
the REAL reference (this container only), for tests/test_image_large_training_gpu.py.

    python tests/golden/make_golden_image_large_grads.py     # rewrites tests/golden/image_large_train/*.npz

The flows are cases (a) and (b) of make_golden_image_large.py, built by its recipes with the parameters of tests/image_synth.py
(a pure function of the seed and the module tree: no state dict is stored for the gradient cases):
  (a) imagelargegrads_mnist_c1_28x28   [1, 28, 28], Laplace base, 2 blocks, c_hidden 32, 2 gated layers with layer norm,
                                       Householder 1, conjugation; 4 rows;
  (b) imagelargegrads_cifar_c3_32x32   [3, 32, 32], radial LogNormal base (p = 1), lu_transform 1, conjugation, 1 block; 2 rows.
Stored per case: x, the fp64 log_prob, the fp64 loss -mean(log_prob) and every parameter's fp64 gradient as g/<name> (recipe of
make_golden_image_grads.grads / make_golden_image_wide.py).  The inputs are drawn from the first generator seed (the large
generator's, + 100 j) for which no ReLU input of the fp64 run lies within KINK_MARGIN = 2e-6 (relative to the tensor's largest
entry) of zero; the seed is recorded in the spec.

For case (a) also a 2-epoch SGD run of the reference's ``Flow.fit`` (64 rows, batch 32, numpy seed 5): the data, the epoch losses,
the final state dict and the learning rate.  As in make_golden_image_wide.py, main() first measures the reference's own
fp32-against-fp64 gap of that run -- losses, parameters (over the tensor's largest entry), each tensor's total update (over the
update's largest entry) -- for five candidate parameter seeds and takes the first learning rate of FIT_LRS, starting from that
generator's 1e-5, at which every candidate stays within FIT_GAP; it refuses to write a fit fixture otherwise.  FIT_GAP is that
generator's: a tenth of the test's bounds for the losses (2e-4) and the parameters (2e-3), 2e-3 for the updates (test: 1e-2).
No rate brings the updates of all five candidates under 1e-3: the gap of the last layer's ``scale`` (updates of 5e-5 of values
of size one) falls with the rate, 2.6e-3 at 1e-5 and 1.2e-3 at 3e-5, while from 5e-5 on the run of one candidate (261) amplifies
rounding (1.4e-2).  A tensor's update counts where the fp64 run moves it by more than 2^-24 of its largest entry: the Householder
vectors of a ONE-channel affine block have a gradient that is zero analytically (the reflection of a 1-vector is -1 whatever
the vector) and move by 1e-16, noise of either precision; the names of the tensors that count are stored (``update_keys``).
The chosen rate and the measured gaps are recorded in the fixture.
Data only."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "image_large_train")
sys.path.insert(0, HERE)

import make_golden_image_large as mgl  # noqa: E402  (imports the reference through ref_shim; its main() is not run)
from make_golden_image_radial import relu_margin  # noqa: E402

flows, networks, distributions = mgl.flows, mgl.networks, mgl.distributions
KINK_MARGIN = 2e-6
N_ROWS, BATCH, EPOCHS, NP_SEED, DATA_SEED = 64, 32, 2, 5, 77
FIT_LRS = (1e-5, 3e-5, 1e-4, 3e-4)
FIT_CANDIDATES = (61, 161, 261, 361, 461)          # parameter seeds; the fixture is the first one's, case (a)'s own
FIT_GAP = (2e-5, 2e-4, 2e-3)                       # losses, parameters, updates: make_golden_image_wide.py's thresholds
U = 2.0 ** -24


def build_laplace(dims, seed):
    from image_synth import synth_image_params_
    spec = dict(in_dims=list(dims), coupling_blocks=2, cond_cls="ConvNet2D", cond_args=mgl.cond_args(dims[0]), householder=1,
                affine_conjugation=True, seed=seed, base="laplace")
    torch.manual_seed(seed)
    flow = flows.USFlow(torch.distributions.Laplace(torch.zeros(dims), torch.ones(dims)), list(dims), 2, networks.ConvNet2D,
                        dict(spec["cond_args"]), householder=1, affine_conjugation=True)
    synth_image_params_(flow, seed)
    return flow, spec


def build_radial(dims, seed, K):
    from image_synth import synth_image_params_
    spec = dict(in_dims=list(dims), coupling_blocks=K, base="lognormal", seed=seed, p=1.0, cond_args=mgl.cond_args(dims[0]), prior_scale=1.0)
    torch.manual_seed(seed)
    nd = distributions.LogNormal(loc=torch.ones([1]) * 6, scale=torch.ones([1]) * .35, device="cpu")
    base = distributions.RadialDistribution(device="cpu", p=1.0, loc=torch.zeros(list(dims)), norm_distribution=nd)
    flow = flows.USFlow(base, list(dims), K, networks.ConvNet2D, dict(spec["cond_args"]), prior_scale=1.0, lu_transform=1, householder=0,
                        affine_conjugation=True, nonlinearity=torch.nn.ReLU())
    synth_image_params_(flow, seed)
    return flow, spec


def to_double(flow, dims, laplace):
    """the flow in fp64 (call under torch.set_default_dtype(torch.float64)), as make_golden_image_large does it"""
    f64 = mgl._double_masks(flow.double())
    if laplace:
        f64.base_distribution = distributions.Independent(
            torch.distributions.Laplace(torch.zeros(dims).double(), torch.ones(dims).double()), len(dims))
    return f64


def grads_case(name, build, dims, x_seed0, n, laplace):
    flow, spec = build()
    torch.set_default_dtype(torch.float64)
    try:
        f64 = to_double(flow, dims, laplace)
        s = x_seed0
        while True:
            x = torch.rand(n, *dims, generator=torch.Generator().manual_seed(s), dtype=torch.float32)
            m = relu_margin(f64, x.double())
            if m >= KINK_MARGIN:
                break
            print(f"{name}: input seed {s}: smallest relative |ReLU input| {m:.2e} < {KINK_MARGIN:.0e}; next seed")
            s += 100
        lp = f64.log_prob(x.double())
        loss = -lp.mean()
        loss.backward()
        out = {"x": x.numpy(), "log_prob64": lp.detach().numpy(), "loss": np.array(float(loss))}
        for k, p in f64.named_parameters():
            if p.grad is not None:
                out["g/" + k] = p.grad.detach().numpy()
    finally:
        torch.set_default_dtype(torch.float32)
    with torch.no_grad():
        flow32, _ = build()
        rel = ((flow32.log_prob(x).double() - torch.from_numpy(out["log_prob64"])).abs() / np.abs(out["log_prob64"]).max()).max().item()
    spec.update(x_seed=s, kink_margin=m, rows=n)
    out["spec"] = np.array(json.dumps(spec))
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    if size > 1000 * 1000:                       # (a committed file stays under 1 MB: the gradients as fp32 casts of the fp64 values)
        for k in list(out):
            if k.startswith("g/"):
                out[k] = out[k].astype(np.float32)
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
    print(f"{name}: input seed {s}, margin {m:.2e}, loss {float(out['loss']):+.6e}, {sum(k.startswith('g/') for k in out)} gradients, "
          f"reference fp32 vs fp64 log_prob {rel:.2e}, {size / 1024:.0f} KB")


def fit_run(dims, seed, lr, double):
    """the reference's 2-epoch SGD run of case (a)'s flow with the parameters of `seed`, in fp32 as it runs or in fp64"""
    flow, _ = build_laplace(dims, seed)
    sd0 = {k: v.detach().double().clone() for k, v in flow.state_dict().items()}
    data = torch.rand(N_ROWS, *dims, generator=torch.Generator().manual_seed(DATA_SEED))
    rows = data
    try:
        if double:
            torch.set_default_dtype(torch.float64)
            flow = to_double(flow, dims, True)
            rows = data.double()
        ds = torch.utils.data.TensorDataset(rows, torch.zeros(N_ROWS))
        np.random.seed(NP_SEED)
        losses = flow.fit(ds, optim=torch.optim.SGD, optim_params=dict(lr=lr), batch_size=BATCH, shuffle=True, device=torch.device("cpu"),
                          epochs=EPOCHS)
    finally:
        torch.set_default_dtype(torch.float32)
    return data, [float(v) for v in losses], {k: v.detach().clone() for k, v in flow.state_dict().items()}, sd0


def fit_self_error(dims, seed, lr):
    """(loss, parameter, update) deviation of the reference's fp32 fit run from its own fp64 run, in the units of the test's bounds"""
    _, l32, sd32, sd0 = fit_run(dims, seed, lr, False)
    _, l64, sd64, _ = fit_run(dims, seed, lr, True)
    el = max(abs(a - b) / abs(b) for a, b in zip(l32, l64))
    ep = eu = 0.0
    for k, v in sd64.items():
        if not v.is_floating_point():
            continue
        d = float((sd32[k].double() - v.double()).abs().max())
        ep = max(ep, d / max(float(v.abs().max()), 1e-3))
        up = float((v.double() - sd0[k]).abs().max())
        if up > U * float(v.abs().max()):           # (an update fp32 cannot hold is no update: see the module docstring)
            eu = max(eu, d / up)
    return el, ep, eu


def main():
    dims_a, dims_b = (1, 28, 28), (3, 32, 32)
    grads_case("imagelargegrads_mnist_c1_28x28", lambda: build_laplace(dims_a, 61), dims_a, 2000 + 61, 4, True)
    grads_case("imagelargegrads_cifar_c3_32x32", lambda: build_radial(dims_b, 62, 1), dims_b, 1000 + 62, 2, False)
    chosen, gaps = None, {}
    for lr in FIT_LRS:
        worst = [0.0, 0.0, 0.0]
        for s in FIT_CANDIDATES:
            e = fit_self_error(dims_a, s, lr)
            print(f"fit lr {lr:g}, candidate seed {s}: reference fp32 vs fp64: losses {e[0]:.1e}, parameters {e[1]:.1e}, updates {e[2]:.1e}")
            worst = [max(a, b) for a, b in zip(worst, e)]
        gaps[lr] = worst
        if all(w <= t for w, t in zip(worst, FIT_GAP)):
            chosen = lr
            break
    assert chosen is not None, f"the reference determines this run at no learning rate of {FIT_LRS}: {gaps}"
    data, losses, sd, sd0 = fit_run(dims_a, FIT_CANDIDATES[0], chosen, False)
    _, _, sd64, _ = fit_run(dims_a, FIT_CANDIDATES[0], chosen, True)
    # the tensors whose update counts (the fp64 run moves them by more than 2^-24 of their largest entry): by name, for the test
    counted = [k for k, v in sd64.items() if v.is_floating_point()
               and float((v.double() - sd0[k]).abs().max()) > U * float(v.abs().max())]
    arrays = {"losses": np.array(losses, dtype=np.float64), "data": data.numpy(), "lr": np.array(chosen),
              "self_gap": np.array(gaps[chosen], dtype=np.float64), "seed": np.array(FIT_CANDIDATES[0]),
              "update_keys": np.array(json.dumps(counted))}
    for k, v in sd.items():
        arrays["sd/" + k] = v.numpy()
    path = os.path.join(OUT, "imagelargefit_mnist_c1_28x28.npz")
    np.savez_compressed(path, **arrays)
    print(f"fit: lr {chosen:g}, epoch losses {losses}, worst gaps over the candidates {gaps[chosen]}, {os.path.getsize(path) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
