"""Golden values, gradients and a golden ``Flow.fit`` run of IMAGE-SHAPED flows with feature maps of 65 .. 256 pixels from the REAL
reference (this container only), for tests/test_image_wide_training_gpu.py.  Written to tests/golden/wide/ -- a directory of
its own, so that the globs of golden_util (image_*.npz, imagegrads_*.npz) do not pick them up.

The forward values come from make_golden_image.run_case, the fp64 gradients and the 2-epoch SGD run from the recipes of
make_golden_image_grads.py (96 rows, batch 32, numpy seed 5).  The inputs are drawn from the first seed for which no ReLU input
of the fp64 run lies within KINK_MARGIN (relative to the tensor's largest entry, the rule of make_golden_image_radial.py) of
zero; the seed is recorded in the spec.  A case holds ~1e5 .. 4e5 ReLU inputs, so a margin of 1e-4 leaves dozens of them inside
the band for every seed; 2e-6 -- that generator's own margin, an order above fp32 rounding -- is reachable.

The fit run uses the recipe of make_golden_image_grads.fit (SGD, 96 rows, batch 32, numpy seed 5, 2 epochs) at FIT_LR = 1e-5,
not that file's 1e-3.  At 1e-3 this 784-dimensional flow of 196-pixel maps sits at the edge of SGD's stability (for some draws the
loss rises, 1211 -> 1501) and the run amplifies rounding a thousandfold in its six steps: the reference's fp32 run then ends up
to 1.6e-2 (relative to a tensor's largest entry) from its own fp64 run, and two runs of one GPU build differ by 3.6e-3, because
torch's own backward of the C = 4 affine blocks is not reproducible to the last bits.  Such a run pins nothing.  At 1e-5 the
reference determines the run for EVERY kink-clean candidate seed (FIT_CANDIDATES; fp32 against fp64: losses <= 7e-8, parameters
<= 3.6e-5 of the largest entry, each tensor's total update <= 1.6e-3 of its largest entry), so the case keeps the first
kink-clean seed like the others.  main() measures and prints these figures again and refuses to write a fixture that exceeds a
tenth of the test's bounds for any candidate."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_image as mgi  # noqa: E402
import make_golden_image_grads as mgg  # noqa: E402
from make_golden_image_radial import relu_margin  # noqa: E402

KINK_MARGIN = 2e-6
GATED_LN = dict(padding="same", kernel_size=3, normalize_layers=True, gating=True)
CASES = [
    # name, in_dims, K, cond_args, seed, householder, conjugation, masktype, rows
    ("wide/image_a_c4_14x14_k2_gated_ln_hh1_conj", (4, 14, 14), 2, dict(c_in=4, c_hidden=16, num_layers=1, **GATED_LN), 61, 1, True,
     "checkerboard", 6),
    ("wide/image_b_c12_16x16_k2_plain_channelmask", (12, 16, 16), 2,
     dict(c_in=12, c_hidden=16, num_layers=2, padding="same", kernel_size=3, normalize_layers=False, gating=False), 62, 0, False,
     "channel", 5),
    ("wide/image_c_c16_9x9_k2_gated_ln_hh1_conj", (16, 9, 9), 2, dict(c_in=16, c_hidden=32, num_layers=1, **GATED_LN), 63, 1, True,
     "checkerboard", 7),
]
FIT_CASE = CASES[0][0]
FIT_LR = 1e-5
FIT_CANDIDATES = (461, 661, 961, 1061, 1361)      # the first five seeds 61 + 100 j of case (a) with a clean ReLU margin


def margin64(name, x_seed):
    """relu_margin of the stored case's fp64 flow on its stored x"""
    flow, spec, a = mgg.build(name)
    torch.set_default_dtype(torch.float64)
    try:
        f64 = flow.double()
        for l in f64.layers:
            if isinstance(l, mgi.transforms.MaskedCoupling):
                l.mask = l.mask.double()
        dims = spec["in_dims"]
        f64.base_distribution = mgi.distributions.Independent(
            torch.distributions.Laplace(torch.zeros(dims).double(), torch.ones(dims).double()), len(dims))
        return relu_margin(f64, torch.from_numpy(a["x"]).double())
    finally:
        torch.set_default_dtype(torch.float32)


def fit_run(name, double):
    """the 2-epoch SGD run of make_golden_image_grads.fit on the stored case, in fp32 as the reference runs it or in fp64"""
    flow, spec, a = mgg.build(name)
    dims = spec["in_dims"]
    data = torch.rand(mgg.N_ROWS, *dims, generator=torch.Generator().manual_seed(77))
    rows = data
    try:
        if double:
            torch.set_default_dtype(torch.float64)
            flow = flow.double()
            for l in flow.layers:
                if isinstance(l, mgi.transforms.MaskedCoupling):
                    l.mask = l.mask.double()
            flow.base_distribution = mgi.distributions.Independent(
                torch.distributions.Laplace(torch.zeros(dims).double(), torch.ones(dims).double()), len(dims))
            rows = data.double()
        ds = torch.utils.data.TensorDataset(rows, torch.zeros(mgg.N_ROWS))
        np.random.seed(mgg.NP_SEED)
        losses = flow.fit(ds, optim=torch.optim.SGD, optim_params=dict(lr=FIT_LR), batch_size=mgg.BATCH, shuffle=True,
                          device=torch.device("cpu"), epochs=mgg.EPOCHS)
    finally:
        torch.set_default_dtype(torch.float32)
    return data, [float(v) for v in losses], {k: v.detach().clone() for k, v in flow.state_dict().items()}


def fit_self_error(name):
    """(loss, parameter, update) deviation of the reference's fp32 fit run from its own fp64 run, in the units of the test's
    bounds: relative loss, parameters over the tensor's largest entry, parameters over the largest entry of the tensor's update"""
    sd0 = {k: v.detach().double() for k, v in mgg.build(name)[0].state_dict().items()}
    _, l32, sd32 = fit_run(name, False)
    _, l64, sd64 = fit_run(name, True)
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
    return el, ep, eu


def main():
    os.makedirs(os.path.join(HERE, "wide"), exist_ok=True)
    for name, dims, K, cond, seed, hh, conj, mask, n in CASES:
        s = seed
        while True:
            mgi.run_case(name, dims, K, cond, s, hh=hh, conj=conj, masktype=mask, n=n)
            m = margin64(name, s)
            if m >= KINK_MARGIN:
                break
            print(f"{name}: seed {s}: smallest relative |ReLU input| {m:.2e} < {KINK_MARGIN:.0e}; next seed")
            s += 100
        path = os.path.join(HERE, name + ".npz")
        z = dict(np.load(path))
        spec = json.loads(str(z["spec"]))
        spec.update(seed=s, kink_margin=m)
        for k in ("zin", "backward32", "forward32", "backward64", "forward64", "log_prob32", "total_ladj64"):
            z.pop(k, None)      # the training test reads x, log_prob64 and the state dict only
        z["spec"] = np.array(json.dumps(spec))
        # the fp64 gradients (recipe of make_golden_image_grads.grads), stored in the same file as g/<parameter>
        flow, _, a = mgg.build(name)
        torch.set_default_dtype(torch.float64)
        try:
            f64 = flow.double()
            for l in f64.layers:
                if isinstance(l, mgi.transforms.MaskedCoupling):
                    l.mask = l.mask.double()
            f64.base_distribution = mgi.distributions.Independent(
                torch.distributions.Laplace(torch.zeros(dims).double(), torch.ones(dims).double()), len(dims))
            lp = f64.log_prob(torch.from_numpy(a["x"]).double())
            assert float((lp.detach() - torch.from_numpy(a["log_prob64"])).abs().max()) < 1e-9
            (-lp.mean()).backward()
            z["loss"] = np.array(float(-lp.mean()))
            for k, p in f64.named_parameters():
                if p.grad is not None:
                    z["g/" + k] = p.grad.detach().numpy()
        finally:
            torch.set_default_dtype(torch.float32)
        np.savez_compressed(path, **z)
        print(f"{name}: seed {s}, margin {m:.2e}, loss {float(z['loss']):+.6e}, {os.path.getsize(path) / 1024:.0f} KB")
    # the 2-epoch SGD run of case (a): first that the reference determines it for every candidate seed (the stored case is
    # rewritten per candidate and restored from its own seed, the first candidate, afterwards)
    name, dims, K, cond, seed, hh, conj, mask, n = CASES[0]
    keep = open(os.path.join(HERE, name + ".npz"), "rb").read()
    assert json.loads(str(np.load(os.path.join(HERE, name + ".npz"))["spec"]))["seed"] == FIT_CANDIDATES[0]
    for s in FIT_CANDIDATES:
        mgi.run_case(name, dims, K, cond, s, hh=hh, conj=conj, masktype=mask, n=n)
        assert margin64(name, s) >= KINK_MARGIN
        el, ep, eu = fit_self_error(name)
        print(f"fit candidate seed {s}: reference fp32 vs fp64: losses {el:.1e}, parameters {ep:.1e}, updates {eu:.1e}")
        assert el <= 2e-5 and ep <= 2e-4 and eu <= 2e-3, "the reference does not determine this run"
    open(os.path.join(HERE, name + ".npz"), "wb").write(keep)
    data, losses, sd = fit_run(FIT_CASE, False)
    arrays = {"losses": np.array(losses, dtype=np.float64), "data": data.numpy(), "lr": np.array(FIT_LR)}
    for k, v in sd.items():
        arrays["sd/" + k] = v.numpy()
    path = os.path.join(HERE, "wide", "fit_a_c4_14x14_k2_gated_ln_hh1_conj.npz")
    np.savez_compressed(path, **arrays)
    print(f"fit: epoch losses {losses}  {os.path.getsize(path) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
