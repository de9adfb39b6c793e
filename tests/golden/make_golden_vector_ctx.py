"""Golden vectors for flows whose ConditionalDenseNN takes a VECTOR context (context_dim > 1), from the REAL reference (this
container only; imported through ref_shim as make_golden_grads.py does).

    python tests/golden/make_golden_vector_ctx.py [case ...]      # writes tests/golden/vctx/<case>.npz

Per case (tests/vctx_cases.py): the reference ``USFlow`` with ``ConditionalDenseNN(context_dim=C)`` is loaded with the
synthetic state dict, and its fp32 and fp64 results are stored -- ``log_prob(x, context)``, ``backward``, ``_forward`` of the
latents, the fp64 gradient of the training loss of ``Flow.fit`` (flows.py:196-199: ``-log_prob(x, context).mean()``) with
respect to every parameter, and the reference's own fp32-vs-fp64 gap on log_prob.  Inputs are regenerated from the seed; the
1100-row cases keep the full log_prob and head / middle / tail rows of the transforms, and their fp64 gradients go to a second
file (<case>_grads.npz) to keep each file under the size limit of a committed one.  Data only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as mg  # noqa: E402  (imports the reference through ref_shim; main() is not run)
import vctx_cases as vc  # noqa: E402

RTOL = 1e-5       # the bound tests/test_flow_gpu.py::test_golden_parity applies: the reference's own fp32 run must stay inside it


def build_reference(spec, C, seed):
    torch.manual_seed(seed)
    act = torch.nn.LeakyReLU(spec.negative_slope) if spec.negative_slope != 0 else torch.nn.ReLU()
    args = dict(input_dim=spec.dim, context_dim=C, hidden_dims=list(spec.hidden_dims), out_dim=spec.dim, nonlinearity=act)
    prior = torch.distributions.Uniform(1e-20, 0.01) if spec.soft_training else None
    return mg.flows.USFlow(mg.make_base(spec), [spec.dim], spec.coupling_blocks, mg.networks.ConditionalDenseNN, args,
                           soft_training=spec.soft_training, training_noise_prior=prior, affine_conjugation=spec.affine_conjugation, lu_transform=spec.lu_transform,
                           householder=spec.householder)


def main():
    os.makedirs(vc.VCTX_DIR, exist_ok=True)
    for name, (kw, C, n, seed, kind, store) in vc.CASES.items():
        if len(sys.argv) > 1 and name not in sys.argv[1:]:
            continue
        spec = vc.spec_of(name)
        sd = vc.state_dict_of(name)
        flow = build_reference(spec, C, seed)
        res = flow.load_state_dict(sd, strict=False)
        assert not res.unexpected_keys and all(k.startswith("base_distribution.") for k in res.missing_keys), res
        full_sd = {k: v.detach().clone() for k, v in flow.state_dict().items()}
        x, zin, ctx = vc.inputs(name)
        out = {}
        with torch.no_grad():
            out["log_prob32"] = flow.log_prob(x, context=ctx)
        torch.set_default_dtype(torch.float64)        # (the reference builds eye() / zeros() at the default dtype)
        try:
            flow64 = mg.to_double(flow, spec)
            x64, z64, c64 = x.double(), zin.double(), ctx.double()
            for p in flow64.parameters():
                p.grad = None
            lp = flow64.log_prob(x64, context=c64)
            (-lp.mean()).backward()
            out["log_prob64"] = lp.detach()
            grads = {k: p.grad.detach() for k, p in flow64.named_parameters() if p.grad is not None}
            with torch.no_grad():
                y = x64                                   # (layer by layer with the context, as make_golden.py's context case)
                for l in reversed(flow64.layers):
                    y = l.backward(y, context=c64)
                out["backward64"] = y
                y = z64
                for l in flow64.layers:
                    y = l.forward(y, context=c64)
                out["forward64"] = y
        finally:
            torch.set_default_dtype(torch.float32)
        gap = ((out["log_prob32"].double() - out["log_prob64"]).abs() / out["log_prob64"].abs()).max().item()
        assert gap < RTOL, f"{name}: the reference's own fp32 log_prob is {gap:.2e} from its fp64 one: change the seed or the scale"
        arrays = {"spec": np.array(vc.spec_json(name)), "ref_gap": np.array(gap), "loss64": np.array(float(-lp.detach().mean()))}
        rows = slice(None) if store else vc.kept_rows(n)
        arrays["log_prob32"], arrays["log_prob64"] = out["log_prob32"].numpy(), out["log_prob64"].numpy()
        arrays["backward64"], arrays["forward64"] = out["backward64"][rows].numpy(), out["forward64"][rows].numpy()
        # the state dict as the reference holds it after loading, and the fp64 gradients: in a file of their own for the
        # 1100-row cases (<case>_grads.npz), whose parameters and gradients together would pass the size limit of a committed file
        for k, v in full_sd.items():
            arrays["sd/" + k] = v.numpy()
        garrays = {"g/" + k: v.numpy() for k, v in grads.items()}
        path = os.path.join(vc.VCTX_DIR, name + ".npz")
        if store:
            arrays.update(garrays)
        else:
            gpath = os.path.join(vc.VCTX_DIR, name + "_grads.npz")
            np.savez_compressed(gpath, **garrays)
            print(f"{name}_grads: {os.path.getsize(gpath) / 1024:.0f} KB")
        np.savez_compressed(path, **arrays)
        print(f"{name:12s} C={C:2d} rows={n:4d} loss {arrays['loss64']:+.6e} ref32-vs-64 {gap:.2e} max|z| "
              f"{out['backward64'].abs().max().item():.3g}  {len(grads)} gradients  {os.path.getsize(path) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
