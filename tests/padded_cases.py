"""Flows at padded feature dims (test infrastructure shared by tests/test_training_emulated.py and tests/test_training_gpu.py).

The engine keeps two row layouts: the segment layout (both mask segments, each padded to 4 columns: ``FlowEngine.LD``) and the
natural one (``LDn = round_up(D, 4)``).  Where the two differ (D = 2, 3, 10, 34, 100, ...) a buffer written in one layout and
read back in the other goes wrong without a shape error, so the training path is held to the fp64 oracle at such dims.

Tolerances follow the oracle's own fp32 run: a device result may be off by 3x what the oracle's fp32 restatement of the same
operation is off from its fp64 one (a deep default-initialised flow amplifies fp32 rounding on its own)."""
import copy

import torch

from oracle import usflows_oracle as orc

# every D mod 4, odd and even segment sizes, LD > LDn (2, 3, 34, 100) and LD == LDn (5, 6, 9, 13)
SWEEP_DIMS = [2, 3, 5, 6, 9, 13, 34, 100]
SWEEP_CONDS = ["ConditionalDenseNN", "DenseNN"]
SWEEP_AFFINE = [(False, 0), (True, 1)]          # (affine_conjugation, householder)
SWEEP_BASES = ["laplace", "radial"]

# golden cases at padded dims: the reference's live flat configuration (D = 2, 10, 100) and two small flows at D = 2
PADDED_GOLDEN = ["init_d2_k4_hh0_laplace", "init_d2_k3_densenn_conj", "init_d10_k10_gmlive", "init_d100_k10_gmlive"]


def sweep_spec(D, cond, conj, hh, base, seed=11):
    """(spec, state dict) of a 3-block flow with [32, 32] conditioners at feature dim D"""
    spec = orc.FlowSpec(D, 3, [32, 32], householder=hh, affine_conjugation=conj, conditioner=cond, base=base, radial_p=1.0)
    if base == "laplace":
        g = torch.Generator().manual_seed(seed + D)
        spec.base_loc = 0.1 * torch.randn(D, generator=g)
        spec.base_scale = 0.5 + torch.rand(D, generator=g)
    sd = orc.synth_state_dict(spec, seed=seed + D)
    if "base_distribution.loc" in sd:
        spec.base_loc = sd["base_distribution.loc"]
    return spec, sd


def sweep_ids():
    return [(D, c, conj, hh, b) for D in SWEEP_DIMS for c in SWEEP_CONDS for conj, hh in SWEEP_AFFINE for b in SWEEP_BASES]


def _kink_margin(spec, sd, x):
    """per row: the smallest |pre-activation| / (largest of its layer) of any conditioner unit in the fp64 oracle's log_prob"""
    sd64 = orc.to_dtype(sd, torch.float64)
    margin = torch.full((x.shape[0],), float("inf"), dtype=torch.float64)
    act = orc._act

    def probe(h, slope):
        margin.copy_(torch.minimum(margin, h.abs().amin(dim=1) / h.abs().max().clamp_min(1e-300)))
        return act(h, slope)
    orc._act = probe
    try:
        orc.flow_log_prob(sd64, spec, x.double(), None)
    finally:
        orc._act = act
    return margin


def sweep_input(spec, sd, B, seed=5, margin=1e-5):
    """B rows in [-1, 1)^D and weights g_lp.  A row that puts a conditioner unit within `margin` of the LeakyReLU kink is drawn
    again: fp32 rounding takes the other branch there than the fp64 oracle, and the row's gradient moves by O(1) of one unit's
    contribution -- a measure-zero event, not what these tests look for"""
    D = spec.dim
    g = torch.Generator().manual_seed(seed + 7 * D + B)
    x, w = torch.rand(B, D, generator=g) * 2 - 1, torch.randn(B, generator=g)
    for _ in range(20):
        bad = _kink_margin(spec, sd, x) < margin
        if not bad.any():
            return x, w
        x[bad] = torch.rand(int(bad.sum()), D, generator=g) * 2 - 1
    raise AssertionError("could not draw rows away from the conditioners' kinks")


def oracle_run(spec, sd, x, g_lp, dtype):
    """log_prob [B], d/dx [B, D] and {parameter: gradient} of sum_m g_lp[m] log_prob(x)[m], by autograd through the oracle
    in `dtype` (radial bases: a trainable loc, as in the flow)"""
    sdd = {k: (v.to(dtype).clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
    spec = copy.copy(spec)
    if spec.base == "radial" and "base_distribution.loc" in sdd:
        spec.base_loc = sdd["base_distribution.loc"]
    else:
        for nm in ("base_loc", "base_scale"):
            v = getattr(spec, nm)
            if torch.is_tensor(v):
                setattr(spec, nm, v.to(dtype))
    xd = x.detach().to(dtype).clone().requires_grad_(True)
    lp = orc.flow_log_prob(sdd, spec, xd, None)
    (lp * g_lp.to(dtype)).sum().backward()
    grads = {k: v.grad for k, v in sdd.items() if torch.is_tensor(v) and v.is_floating_point() and v.grad is not None}
    return lp.detach(), xd.grad, grads


class Reference:
    """the fp64 oracle's results and the fp32 oracle's distance from them, for one (flow, input, g_lp)"""

    def __init__(self, spec, sd, x, g_lp):
        self.lp, self.gx, self.g = oracle_run(spec, sd, x, g_lp, torch.float64)
        lp32, gx32, g32 = oracle_run(spec, sd, x, g_lp, torch.float32)
        self.e32_lp = ((lp32.double() - self.lp).abs() / self.lp.abs()).max().item()
        self.gx_scale = self.gx.abs().max().item()
        self.e32_x = (gx32.double() - self.gx).abs().max().item()
        self.e32_g = {k: (g32[k].double() - v).abs().max().item() for k, v in self.g.items() if k in g32}
        self.gmax = max(v.abs().max().item() for v in self.g.values())

    def input_grad_tol(self):
        """max(2e-5, 3 e32) of the gradient's scale, e32 = the fp32 oracle's error relative to that scale"""
        return max(2e-5, 3 * self.e32_x / self.gx_scale) * self.gx_scale

    def check_log_prob(self, lp, tol=2e-5):
        """row-wise relative error below max(tol, 3 x the fp32 oracle's).  A row whose log_prob cancels to near 0 (terms of a few
        nats each) has no relative accuracy in any fp32 evaluation: there the error is taken relative to 1 nat"""
        rel = ((lp.detach().cpu().double() - self.lp).abs() / self.lp.abs().clamp_min(1.0)).max().item()
        assert rel < max(tol, 3 * self.e32_lp), ("log_prob row-wise", rel, self.e32_lp)

    def check_input_grad(self, gx, what="", kink_rows=0):
        """kink_rows > 0 (batches of thousands of rows): a hidden unit whose pre-activation is within fp32 noise of zero takes the
        other LeakyReLU branch than in the fp64 oracle and changes its row's gradient by O(1) -- at most that many rows may miss"""
        assert gx is not None and tuple(gx.shape) == tuple(self.gx.shape), what
        d = (gx.detach().cpu().double() - self.gx).abs()
        if kink_rows:
            bad = d.amax(dim=1) > self.input_grad_tol()
            assert int(bad.sum()) <= kink_rows, ("input gradient rows", what, int(bad.sum()))
            d = d[~bad]
        err = d.max().item()
        assert err <= self.input_grad_tol(), ("input gradient", what, err, self.gx_scale, self.e32_x)
        return err / self.gx_scale

    def check_param_grads(self, flow, what="", kink_frac=0.0):
        """every trainable parameter of `flow` the oracle differentiates (the radial norm distribution's are constants there):
        within max(2e-4 |ref|max, 3 x the fp32 oracle's gap) + 1e-5 gmax (a gradient that cancels to ~1e-15 sits at the
        pass's noise).  kink_frac > 0: at most that fraction of a tensor's entries (or 2) may miss, by no more than 5 % of its
        largest entry (LeakyReLU branches taken differently at thousands of rows, see check_input_grad)"""
        n = 0
        params = {k: p for k, p in flow.named_parameters() if p.requires_grad}
        for k, ref in self.g.items():
            if "norm_distribution" in k or k not in params:
                continue
            got = params[k].grad
            big = ref.abs().max().item()
            if big == 0.0:
                assert got is None or got.abs().max().item() < 1e-6, (what, k)
                continue
            assert got is not None, (what, "no gradient for", k)
            err = (got.detach().cpu().double().reshape(ref.shape) - ref).abs().max().item()
            tol = max(2e-4 * big, 3 * self.e32_g.get(k, 0.0)) + 1e-5 * self.gmax
            if kink_frac > 0.0:
                diff = (got.detach().cpu().double().reshape(ref.shape) - ref).abs()
                n_bad = int((diff > tol).sum())
                assert n_bad <= max(2, int(kink_frac * diff.numel())) and err <= 0.05 * big, (what, k, n_bad, err, big)
            else:
                assert err <= tol, (what, k, err, big, self.e32_g.get(k))
            n += 1
        return n
