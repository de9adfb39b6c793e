"""Conditional image-shaped flows of the real reference (tests/golden/cond/*.npz, made by
tests/golden/make_golden_cond_image.py): the mirror ``USFlow`` with ``CondConvNet2D`` / ``CondConvNet`` built as there, its
parameters regenerated from the seed (tests/image_synth.py), soft-trained."""
import glob
import json
import os

import numpy as np
import torch

COND_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cond")


def cond_case_names(with_grads=False):
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(COND_DIR, "condimage_*.npz")))
    if with_grads:
        names = [n for n in names if any(k.startswith("g/") for k in np.load(os.path.join(COND_DIR, n + ".npz")).files)]
    return names


def load_cond_case(name, device="cpu", dtype=torch.float32):
    """(mirror USFlow, arrays) of a conditional image case; dtype float64: the CPU mirror in double precision"""
    from image_synth import synth_image_params_
    from usflows_amd import networks
    from usflows_amd.flows import USFlow
    z = np.load(os.path.join(COND_DIR, name + ".npz"), allow_pickle=False)
    d = json.loads(str(z["spec"]))
    dims = d["in_dims"]
    torch.manual_seed(d["seed"])
    base = torch.distributions.Laplace(torch.zeros(dims, dtype=dtype, device=device), torch.ones(dims, dtype=dtype, device=device))
    flow = USFlow(base, dims, d["coupling_blocks"], getattr(networks, d["cond_cls"]), dict(d["cond_args"]),
                  householder=d["householder"], affine_conjugation=d["affine_conjugation"], soft_training=True)
    synth_image_params_(flow, d["seed"])
    if dtype == torch.float64:
        flow = flow.double()
        for l in flow.layers:
            if hasattr(l, "mask") and torch.is_tensor(l.mask):
                l.mask = l.mask.double()
    if device != "cpu":
        flow = flow.to(device)
    arrays = {k: torch.from_numpy(z[k]) for k in z.files if k != "spec"}
    return flow, arrays


class default_double:
    """torch.set_default_dtype(float64) inside (the reference's fp64 runs, tests/golden/make_golden_cond_image.py, do the same:
    the affine layers build their identity matrices in the default dtype)"""

    def __enter__(self):
        torch.set_default_dtype(torch.float64)

    def __exit__(self, *exc):
        torch.set_default_dtype(torch.float32)
        return False


def run_layers(flow, x, context, inverse):
    for layer in (reversed(flow.layers) if inverse else flow.layers):
        x = layer.backward(x, context) if inverse else layer.forward(x, context)
    return x
