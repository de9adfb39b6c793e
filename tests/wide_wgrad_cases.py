"""Cases, inputs and the fp64 reference of the usf_conv_wgrad_wide_f32 tests (test_wide_wgrad_gpu.py, test_wide_wgrad_cpu.py)."""
import torch
import torch.nn.functional as F

# (cin, cout, H, W, ks)
SHAPES = [
    (4, 16, 14, 14, 3), (16, 4, 14, 14, 3),      # a partial channel tile on either side
    (16, 16, 14, 14, 3),
    (16, 32, 14, 14, 1),
    (12, 16, 16, 16, 3), (16, 16, 16, 16, 1),    # 256 pixels, the maximum
    (5, 7, 9, 9, 3),                             # odd everything, 81 pixels
    (16, 16, 5, 13, 1), (16, 16, 5, 13, 3),      # 65 pixels: usf_conv_wgrad_f32's first refusal
    (32, 32, 10, 10, 3),
    (64, 64, 9, 9, 1),
    (3, 3, 16, 16, 3),
    (16, 16, 1, 65, 3),
    (16, 16, 65, 1, 3),                          # W == 1 is served: the column taps meet the pad column only
    (32, 32, 7, 7, 3),                           # a small map: cross-checked against usf_conv_wgrad_f32
]
# one shape per kernel instantiation the list above does not launch (tiles per wave 2, 4, 7, 8, 14, 15, 19, 21, 28, 37), the last
# two with the largest LDS images: 118 744 and 150 744 bytes, above the 64 KiB a kernel gets without raising its limit
MORE_SHAPES = [
    (32, 32, 9, 9, 1), (64, 48, 9, 9, 1), (48, 16, 9, 9, 3), (16, 48, 9, 9, 3), (48, 32, 9, 9, 3), (32, 48, 9, 9, 3),
    (64, 32, 9, 9, 3), (48, 48, 9, 9, 3), (64, 48, 9, 9, 3), (64, 64, 14, 14, 3), (64, 64, 16, 16, 3),
]
BATCHES = (1, 5, 300)
FORMS = ("plain", "mask_relu_nobias", "presub_leaky", "no_db")
REFUSED = [(16, 16, 1, 257, 3), (65, 16, 9, 9, 3), (16, 16, 9, 9, 5), (16, 65, 9, 9, 1), (16, 16, 257, 1, 1)]

# every (cin tiles, cout tiles, taps) the served range has -> the kernel instantiation (tiles per wave) each needs
def tiles_per_wave(cit: int, cot: int, taps: int) -> int:
    tiles = cot * (cit * taps + 1)
    groups = 4 if tiles >= 3 else tiles
    return -(-tiles // groups)


def inputs(cin, cout, H, W, B, form, device, seed=0):
    """x, dy and the call's keyword arguments for one form; the ReLU inputs keep clear of zero so that fp32 and fp64 agree on
    every gate"""
    g = torch.Generator().manual_seed(seed + 1000 * B + cin + 7 * cout + H * W)
    x = torch.randn(B, cin, H, W, generator=g)
    dy = torch.randn(B, cout, H, W, generator=g)
    kw = {}
    if form == "mask_relu_nobias":
        kw = dict(in_mul=(torch.rand(cin, H, W, generator=g) < 0.5).float().reshape(-1), in_act=1, in_slope=0.0, want_bias=False)
    elif form == "presub_leaky":
        kw = dict(pre_sub=torch.randn(cin, generator=g), in_act=1, in_slope=0.1)
    elif form == "no_db":
        kw = dict(want_bias=False)
    if "pre_sub" in kw or kw.get("in_act"):
        v = x - kw["pre_sub"].view(1, -1, 1, 1) if "pre_sub" in kw else x
        x = x + torch.where(v.abs() < 1e-3, torch.sign(v) * 2e-3 + (v == 0) * 2e-3, torch.zeros(()))
    x, dy = x.to(device), dy.to(device)
    kw = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in kw.items()}
    return x, dy, kw


def xin64(x, kw):
    """the convolution's effective input in fp64: in_act(x - pre_sub) * in_mul"""
    v = x.double()
    if kw.get("pre_sub") is not None:
        v = v - kw["pre_sub"].double().view(1, -1, 1, 1)
    if kw.get("in_act"):
        v = torch.where(v > 0, v, v * float(kw.get("in_slope", 0.0)))
    if kw.get("in_mul") is not None:
        v = v * kw["in_mul"].double().view(1, *x.shape[1:])
    return v


def ref64(x, dy, ks, kw):
    """dW [cout, cin, ks, ks], db [cout] in fp64: unfold + einsum"""
    v = xin64(x, kw)
    B, cin, H, W = v.shape
    cols = F.unfold(v, ks, padding=ks // 2).view(B, cin, ks * ks, H * W)
    dW = torch.einsum("bop,bctp->oct", dy.double().flatten(2), cols).view(dy.shape[1], cin, ks, ks)
    return dW, dy.double().sum((0, 2, 3))


def err32(x, dy, ks, kw):
    """max error against fp64 of a plain fp32 CPU computation of the same gradient (torch.nn.grad.conv2d_weight)"""
    v = xin64(x, kw).float().cpu()
    d = dy.float().cpu()
    g32 = torch.nn.grad.conv2d_weight(v, (dy.shape[1], x.shape[1], ks, ks), d, padding=ks // 2)
    g64 = torch.nn.grad.conv2d_weight(v.double(), (dy.shape[1], x.shape[1], ks, ks), d.double(), padding=ks // 2)
    return float((g32.double() - g64).abs().max())
