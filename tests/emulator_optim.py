"""A torch fp32 restatement of the arithmetic of usflows_amd/csrc/usf_optim.hip (usf_adam_step_f32 and the two gradient
clip kernels), operation by operation, for tests that run without a GPU and as the GPU tests' second reference.

A fused multiply-add is one rounding of the exact a * b + c: the product of two fp32 values is exact in fp64, so
``(a.double() * b.double() + c.double()).float()`` differs from it only where the fp64 sum lands within 2^-53 relative of a
rounding boundary of fp32."""
import math

import torch

CHUNK = 16384


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def adam_step(p, g, m, v, vmax, t, *, lr, betas, eps, weight_decay, maximize=False, amsgrad=False, decoupled=False):
    """one step of the kernel on fp32 tensors, IN PLACE; ``t`` is the step count after the kernel's advance (1 for the
    first step)"""
    f32 = torch.float32
    assert p.dtype == f32 and g.dtype == f32
    beta1, beta2 = betas
    w1 = torch.tensor(1.0 - beta1, dtype=f32)
    beta2f, omb2 = torch.tensor(beta2, dtype=f32), torch.tensor(1.0 - beta2, dtype=f32)
    epsf, wdf = torch.tensor(eps, dtype=f32), torch.tensor(weight_decay, dtype=f32)
    bc1, bc2 = 1.0 - beta1 ** float(t), 1.0 - beta2 ** float(t)           # fp64, as the device's pow
    neg_step = torch.tensor(-(lr / bc1), dtype=f32)
    bc2_sqrt = torch.tensor(math.sqrt(bc2), dtype=f32)
    g = -g if maximize else g.clone()
    if weight_decay != 0:
        if decoupled:
            p.mul_(torch.tensor(1.0 - lr * weight_decay, dtype=f32))
        else:
            g = _fma(wdf, p, g)
    d = g - m
    if abs(float(w1)) < 0.5:
        m.copy_(_fma(w1, d, m))
    else:
        m.copy_(_fma(d, w1 - 1.0, g))
    v.copy_(v * beta2f + (omb2 * g) * g)
    vv = v
    if amsgrad:
        torch.maximum(vmax, v, out=vmax)
        vv = vmax
    denom = vv.sqrt() / bc2_sqrt + epsf
    p.add_(neg_step * (m / denom))


def _block_sum_256(vals):
    """the kernels' block reduction of 256 fp64 lane values: a fixed tree, lane i += lane i + o for o = 128, 64, ..., 1"""
    vals = vals.clone()
    o = 128
    while o > 0:
        vals[:o] += vals[o: 2 * o]
        o //= 2
    return vals[0]


def _lane_sums(x):
    """thread t of a block sums elements t, t + 256, ... in ascending order (fp64)"""
    n = x.numel()
    pad = (-n) % 256
    rows = torch.cat([x, x.new_zeros(pad)]).reshape(-1, 256)
    s = torch.zeros(256, dtype=torch.float64)
    for r in rows:                                  # ascending: the order of the kernel's loop
        s = s + r
    return s


def clip_grad_norm(grads, max_norm):
    """usf_grad_sqnorm_partials_f32 + usf_grad_clip_scale_f32 on a list of fp32 tensors, IN PLACE"""
    partials = []
    for g in grads:
        flat = g.reshape(-1).double()
        for off in range(0, flat.numel(), CHUNK):
            c = flat[off: off + CHUNK]
            partials.append(_block_sum_256(_lane_sums(c * c)))
    total = _block_sum_256(_lane_sums(torch.stack(partials))) if partials else torch.tensor(0.0, dtype=torch.float64)
    coef = float(max_norm) / (torch.sqrt(total) + 1e-6)
    clamped = torch.tensor(1.0) if bool(coef > 1.0) else coef.float()
    for g in grads:
        g.mul_(clamped)
    return total
