"""The vector-context cases (ConditionalDenseNN with context_dim > 1) shared by tests/golden/make_golden_vector_ctx.py, which
records the real reference's results into tests/golden/vctx/*.npz, and by the tests that read them.  Inputs, latents and
contexts are functions of the case's seed (``inputs``): the 1100-row cases store no rows, only results, and keep their
fp64 gradients in a second file."""
import json
import os

import numpy as np
import torch

from oracle import usflows_oracle as orc

VCTX_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vctx")

# name -> (spec arguments, context_dim, rows, seed, context kind, keep every row and the gradients in the case's one file?)
CASES = {
    # tiny-layer kernel, odd halves (4 / 3)
    "d7_k3": (dict(dim=7, coupling_blocks=3, hidden_dims=[16, 16], householder=0, base="laplace"), 3, 37, 11, "uniform", True),
    # class-conditional: one-hot labels
    "d16_k3": (dict(dim=16, coupling_blocks=3, hidden_dims=[32], householder=1, affine_conjugation=True, base="normal"),
               10, 64, 12, "onehot", True),
    # above the tiny kernel's 256 rows; padded halves 17 / 16
    "d33_k2": (dict(dim=33, coupling_blocks=2, hidden_dims=[40, 24], lu_transform=2, householder=1, base="laplace"),
               5, 300, 13, "uniform", True),
    # bf16x3 kernel: hidden width in (128, 256], >= 1024 rows, no multiple of the 128-row tile
    "d64_k2_c10": (dict(dim=64, coupling_blocks=2, hidden_dims=[160, 160], householder=1, base="laplace"), 10, 1100, 14, "onehot", False),
    "d64_k2_c32": (dict(dim=64, coupling_blocks=2, hidden_dims=[160, 160], householder=1, base="laplace"), 32, 1100, 15, "uniform", False),
}
SMALL = [n for n in CASES if CASES[n][5]]
ROWS_KEPT = 8          # head / middle / tail rows of backward64 / forward64 kept by the cases that store no rows


def spec_of(name):
    kw, C = CASES[name][0], CASES[name][1]
    # (soft_training: the reference's USFlow.log_prob hands a context on only then, flows.py:559-567; the caller passes it)
    return orc.FlowSpec(**kw, soft_training=True, extra={"context_dim": C})


def inputs(name):
    """(x [n, D] in [0, 1), latents zin [n, D] ~ Laplace, context [n, C]) of a case, from its seed"""
    kw, C, n, seed, kind, _ = CASES[name]
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.rand(n, kw["dim"], generator=g)
    zin = torch.distributions.Laplace(0.0, 1.0).icdf(torch.rand(n, kw["dim"], generator=g) * 0.998 + 0.001)
    if kind == "onehot":
        ctx = torch.nn.functional.one_hot(torch.randint(0, C, (n,), generator=g), C).float()
    else:
        ctx = torch.rand(n, C, generator=g) * 2 - 0.5
    return x, zin, ctx


def kept_rows(n):
    """the rows of backward64 / forward64 a 1100-row case keeps"""
    k = ROWS_KEPT
    return torch.cat([torch.arange(k), torch.arange(n // 2, n // 2 + k), torch.arange(n - k, n)])


def state_dict_of(name):
    """the case's parameters: the documented synthetic generator with the context layer sized [h0, C]"""
    from usflows_amd.synth import synth_state_dict
    return synth_state_dict(spec_of(name), seed=CASES[name][3])


def load(name):
    """(spec, state dict, arrays: log_prob32 / log_prob64 / backward64 / forward64 / ref_gap, {parameter: fp64 gradient})"""
    z = np.load(os.path.join(VCTX_DIR, name + ".npz"), allow_pickle=False)
    d = json.loads(str(z["spec"]))
    assert d == json.loads(spec_json(name)), "fixture was made for another spec"
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    arrays = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith(("sd/", "g/")) and k != "spec"}
    gz = z if CASES[name][5] else np.load(os.path.join(VCTX_DIR, name + "_grads.npz"), allow_pickle=False)   # (1100 rows: own file)
    grads = {k[2:]: torch.from_numpy(gz[k]) for k in gz.files if k.startswith("g/")}
    return spec_of(name), sd, arrays, grads


def spec_json(name):
    kw, C, n, seed = CASES[name][:4]
    return json.dumps(dict(kw, context_dim=C, rows=n, seed=seed), sort_keys=True)


def build(name, sd=None, device="cpu"):
    from usflows_amd.synth import build_usflow
    return build_usflow(spec_of(name), sd if sd is not None else state_dict_of(name), device=device)


# context rows WIDER than every hidden layer and than the rows themselves (Cp = round_up(C, 4) > max(hidden, LD)): the shapes at
# which the context layer's gradient image must be sized by Cp.  (dim, hidden, C, rows): 37 rows = the queued small-batch gradient
# jobs, 300 rows = the direct weight-gradient launches.  No fixture: checked against autograd through the fp64 oracle.
WIDE = [(8, [16], 32, 37), (8, [16], 32, 300), (8, [8], 10, 37)]


def wide_case(dim, hidden, C, rows):
    """(spec, state dict, x, context, {parameter: fp64 gradient of -log_prob(x, context).mean() through the oracle}, log_prob64)"""
    from usflows_amd.synth import synth_state_dict
    spec = orc.FlowSpec(dim=dim, coupling_blocks=2, hidden_dims=hidden, householder=1, soft_training=True, extra={"context_dim": C})
    sd = synth_state_dict(spec, seed=40 + C)
    g = torch.Generator().manual_seed(rows + C)
    x, ctx = torch.rand(rows, dim, generator=g), torch.rand(rows, C, generator=g) * 2 - 0.5
    sd64 = {k: (v.double().clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
    lp = orc.flow_log_prob(sd64, spec, x.double(), ctx.double())
    (-lp.mean()).backward()
    grads = {k: v.grad for k, v in sd64.items() if torch.is_tensor(v) and v.is_floating_point() and v.grad is not None}
    return spec, sd, x, ctx, grads, lp.detach()
