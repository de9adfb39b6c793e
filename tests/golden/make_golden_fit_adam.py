"""Golden run of the REAL reference's ``Flow.fit`` with ``torch.optim.Adam`` (this container only), the optimiser most of
its experiment files name -- in fp32 AND in fp64, so that a test can hold the device run to the reference's own rounding
error instead of to a guessed tolerance.

    python tests/golden/make_golden_fit_adam.py        # writes tests/golden/fitadam/fitadam_<case>.npz

(a directory of their own: the per-case loops of the suite take every .npz directly under tests/golden for a model case)

Two epochs over 96 rows (batch 32, shuffle=True under a fixed numpy seed: 6 steps) of Adam(lr=1e-3, weight_decay=0.1) from
the stored state dict of a small golden case, the second case with gradient_clip=1.0; stored: the data, the per-epoch
losses and every parameter after the 6 steps, of both runs.  Data only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as mg  # noqa: E402
from golden_util import load_case  # noqa: E402

# (case, gradient_clip)
CASES = [("synth_d7_k3_hh0_laplace", None), ("synth_d16_k3_hh1_radial2", 1.0)]
OPTIM = dict(lr=1e-3, weight_decay=0.1)
NP_SEED, N_ROWS, BATCH, EPOCHS = 5, 96, 32, 2


def run(name, clip, dtype):
    spec, sd, _ = load_case(name)
    seed = int(np.load(os.path.join(HERE, name + ".npz"))["seed"])
    flow = mg.build_reference(spec, seed)
    res = flow.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys
    data = torch.rand(N_ROWS, spec.dim, generator=torch.Generator().manual_seed(77))
    torch.set_default_dtype(dtype)
    try:
        if dtype == torch.float64:
            # (make_golden.py's recipe: the reference's constructors build torch.FloatTensor values, so it is built in fp32
            # and converted; its matrices are created with the default dtype, which an fp64 run has to switch as well)
            flow = mg.to_double(flow, spec)
            data = data.double()
        ds = torch.utils.data.TensorDataset(data, torch.zeros(N_ROWS))
        np.random.seed(NP_SEED)
        losses = flow.fit(ds, optim=torch.optim.Adam, optim_params=dict(OPTIM), batch_size=BATCH, shuffle=True,
                          gradient_clip=clip, device=torch.device("cpu"), epochs=EPOCHS)
        params = {k: v.detach().clone() for k, v in flow.state_dict().items()}
        assert all(v.dtype == dtype for v in params.values() if v.is_floating_point())
        with torch.no_grad():
            assert flow.log_prob(data[:4]).dtype == dtype
    finally:
        torch.set_default_dtype(torch.float32)
    return data, losses, params


def main():
    for name, clip in CASES:
        if len(sys.argv) > 1 and name not in sys.argv[1:]:
            continue
        data, l32, p32 = run(name, clip, torch.float32)
        _, l64, p64 = run(name, clip, torch.float64)
        arrays = {"data": data.numpy(), "gradient_clip": np.array(-1.0 if clip is None else clip),
                  "losses32": np.array(l32, dtype=np.float64), "losses64": np.array(l64, dtype=np.float64)}
        for k in p32:
            arrays["sd32/" + k] = p32[k].numpy()
            arrays["sd64/" + k] = p64[k].numpy()
        os.makedirs(os.path.join(HERE, "fitadam"), exist_ok=True)
        path = os.path.join(HERE, "fitadam", "fitadam_" + name + ".npz")
        np.savez_compressed(path, **arrays)
        worst = max((p32[k].double() - p64[k].double()).abs().max().item() for k in p32 if p32[k].is_floating_point())
        print(f"{name:32s} clip {clip}  losses fp32 {l32}  fp64 {l64}  max |fp32 - fp64| over parameters {worst:.2e}  "
              f"{os.path.getsize(path) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
