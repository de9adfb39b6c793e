"""Which kernel serves a convolution of an image-shaped flow: the rules networks.py (inference) and image_training.py (the
autograd Functions) share.  A leaf module: it imports neither.

* the geometry the kernels can express (``same_conv_ks``; the looser kernel-1 form ``pointwise_geometry``);
* the weight gradient's route: ``wgrad_kernels`` names the candidate kernels in the order tried, ``WGRAD_KERNELS`` maps each name
  to its served query and its launch, ``wgrad_route`` / ``wgrad_served`` ask and ``conv_wgrad`` launches -- off the SAME tuple;
* the per-layer predicates built from the two (``conv_shape_ok``, ``conv_ctx_shape_ok``, ``pointwise_shape_ok``,
  ``gate_halves_ok``) and the route of GatedConv's 1 x 1 convolution (``gate_conv_route``).
"""
from __future__ import annotations

import torch

from . import _ext
from .config import config

BAND_MIN_PIXELS = 257    # feature maps of 257 .. 4096 pixels: usf_conv2d_same_f32 refuses them, usf_conv2d_same_band_f32 serves them (training: knob train_band)
WIDE_MIN_PIXELS = 65      # feature maps of 65 .. 256 pixels: usf_conv_wgrad_f32 refuses them, usf_conv_wgrad_wide_f32 serves them


# ---- geometry -------------------------------------------------------------------------------------------------------------------
def conv_kernel_sizes() -> tuple:
    """kernel sizes of the "same" convolutions the device path takes, inference and training: 1 and 3, 4 under the knob
    ``conv_k4`` (padding="same" only: torch's placement, one zero before and two after), 5 under the knob ``conv_k5``"""
    return (1, 3) + ((4,) if config.conv_k4 else ()) + ((5,) if config.conv_k5 else ())


def same_padding(conv) -> bool:
    """the convolution's padding is the "same" placement the kernels compute: the string, or k // 2 on both sides at an odd
    kernel (at kernel 4 the integer padding (2, 2) yields H + 1 outputs: not "same")"""
    k, pad = conv.kernel_size[0], conv.padding
    return pad == "same" or (k % 2 == 1 and not isinstance(pad, str) and tuple(pad) == (k // 2, k // 2))


def same_conv_ks(conv) -> int:
    """the kernel size of an nn.Conv2d the kernels can express -- square and in ``conv_kernel_sizes()``, stride 1, dilation 1,
    groups 1, zero padding in the "same" placement -- else 0"""
    if not isinstance(conv, torch.nn.Conv2d):
        return 0
    k = conv.kernel_size
    if k[0] != k[1] or k[0] not in conv_kernel_sizes() or conv.stride != (1, 1) or conv.dilation != (1, 1) or conv.groups != 1 \
            or conv.padding_mode != "zeros" or not same_padding(conv):
        return 0
    return k[0]


def pointwise_geometry(conv) -> bool:
    """the kernel-1 form the per-pixel kernels take (usf_pointwise_conv_f32, usf_gated_tail_f32, the two halves of a gate
    convolution): stride 1, groups 1, padding "same" or 0.  Looser than ``same_conv_ks(conv) == 1``: dilation and padding mode
    are not looked at (neither means anything at kernel 1 without padding; GatedConv hands its dilation to this convolution)"""
    return (isinstance(conv, torch.nn.Conv2d) and conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.groups == 1
            and same_padding(conv))


def band_conv_ok(cin: int, cout: int, H: int, W: int, ks: int) -> bool:
    """under the knob ``conv_band``: a "same" convolution on a feature map too large for usf_conv2d_same_f32 (more than 256
    pixels) that the row-banded kernel serves (usf_conv2d_same_band_f32: kernel 1 / 3, up to 64 channels, up to 4096 pixels,
    W <= 64, a band of at least 4 rows beside the weight planes in the LDS).  Inference asks it per convolution; training asks
    it in both directions (``train_band_ok``) under the knob ``train_band``"""
    return bool(config.conv_band) and H * W >= BAND_MIN_PIXELS and ks in (1, 3) and \
        _ext.load().usf_conv2d_same_band_fits(cin, cout, H, W, ks) > 0


def train_band_ok(cin: int, cout: int, H: int, W: int, ks: int) -> bool:
    """under the knob ``train_band``: forward (cin -> cout) and data gradient (cout -> cin) of a convolution on a map above 256
    pixels both run on the row-banded kernel.  64 -> 64 channels at kernel 3 do not (no four rows beside the weight planes),
    nor kernel 4 / 5, nor maps wider than 64: those layers stay on torch"""
    return bool(config.train_band) and band_conv_ok(cin, cout, H, W, ks) and band_conv_ok(cout, cin, H, W, ks)


# ---- the weight gradient's route ------------------------------------------------------------------------------------------------
def wgrad_kernels(ks: int, pixels: int) -> tuple:
    """names of the weight-gradient kernels tried for a ks x ks convolution on a feature map of `pixels`, in order:
    kernel 5 / 4: usf_conv_wgrad_k5_f32 / _k4_f32 at every pixel count, under their knobs; kernel 1 / 3 at 257 pixels and more,
    under the knob ``train_band``: usf_conv_wgrad_band_f32 alone (the others refuse every such map); 65 pixels and more:
    usf_conv_wgrad_wide_f32 (knob ``wgrad_wide``) -- without a try of the narrow kernel first: it refuses every map above 64
    pixels (pinned by tests/test_wide_wgrad_cpu.py::test_the_old_queries_answer_what_they_answered_before); up to 64 pixels
    usf_conv_wgrad_f32 as ever, and under ``conv_k5`` / ``conv_k4`` (either) what it refuses (channel counts that are no
    multiple of 16: the 8 hidden channels of the hyper-parameter search) goes to the wide kernel, which serves small maps at
    any channel counts with the same sums in another order"""
    if ks == 5:
        return ("k5",) if config.conv_k5 else ()
    if ks == 4:
        return ("k4",) if config.conv_k4 else ()
    if pixels >= BAND_MIN_PIXELS and config.train_band:
        return ("band",)
    if pixels >= WIDE_MIN_PIXELS:
        return ("wide",) if config.wgrad_wide else ()
    return ("narrow",) + (("wide",) if config.wgrad_wide and (config.conv_k5 or config.conv_k4) else ())


def _workspace_query(entry: str):
    return lambda B, cin, cout, H, W, ks, masked: getattr(_ext.load(), entry)(B, cin, cout, H, W, ks) > 0


# name: (served query (B, cin, cout, H, W, ks, masked), launch (x, dy, ks, defer, owners, transforms) -> (dW, db) | None).
# The narrow kernel's two forms differ (64 -> 64 channels at kernel 1 and 57 .. 64 pixels run without a mask only), so its plan
# answers for the asked form; the other four are one kernel for both forms: their workspace is > 0 or the shape is refused.
# Only the narrow kernel may queue its last sum (defer / owners); the others' launches run in stream order.  The launches look
# their binding up on _ext when called.
WGRAD_KERNELS = {
    "narrow": (lambda B, cin, cout, H, W, ks, masked: _ext.conv_wgrad_kernel(B, cin, cout, H, W, ks, masked) != 0,
               lambda x, dy, ks, defer, owners, kw: _ext.conv_wgrad(x, dy, ks, defer=defer, owners=owners, **kw)),
    "wide": (_workspace_query("usf_conv_wgrad_wide_workspace"), lambda x, dy, ks, defer, owners, kw: _ext.conv_wgrad_wide(x, dy, ks, **kw)),
    "band": (lambda B, cin, cout, H, W, ks, masked: _ext.load().usf_conv_wgrad_band_workspace(B, cin, cout, H, W, ks, 0) > 0,
             lambda x, dy, ks, defer, owners, kw: _ext.conv_wgrad_band(x, dy, ks, **kw)),
    "k5": (_workspace_query("usf_conv_wgrad_k5_workspace"), lambda x, dy, ks, defer, owners, kw: _ext.conv_wgrad_k5(x, dy, **kw)),
    "k4": (_workspace_query("usf_conv_wgrad_k4_workspace"), lambda x, dy, ks, defer, owners, kw: _ext.conv_wgrad_k4(x, dy, **kw)),
}


def wgrad_route(B: int, cin: int, cout: int, H: int, W: int, ks: int, masked: bool, among=None):
    """the name of the first kernel of ``wgrad_kernels`` that serves this call -- with an input mask (in_mul) or without -- or
    None; among: only these candidates count"""
    for name in wgrad_kernels(ks, H * W):
        if (among is None or name in among) and WGRAD_KERNELS[name][0](max(B, 1), cin, cout, H, W, ks, masked):
            return name
    return None


def wgrad_served(B: int, cin: int, cout: int, H: int, W: int, ks: int, masked: bool) -> bool:
    return wgrad_route(B, cin, cout, H, W, ks, masked) is not None


def wide_wgrad_served(B: int, cin: int, cout: int, H: int, W: int, ks: int) -> bool:
    """does usf_conv_wgrad_wide_f32 take over this call as the map is too large for usf_conv_wgrad_f32?"""
    return H * W >= WIDE_MIN_PIXELS and wgrad_route(B, cin, cout, H, W, ks, False, among=("wide",)) is not None


def conv_wgrad(x, dy, ks, in_mul=None, pre_sub=None, in_act=_ext.ACT_NONE, in_slope=0.0, want_bias=True, defer=False, owners=()):
    """(dW, db | None) of a convolution's backward from the first kernel of ``wgrad_kernels`` that takes it, or None.  No query
    in front of a launch: a binding that refuses answers None"""
    kw = dict(in_mul=in_mul, pre_sub=pre_sub, in_act=in_act, in_slope=in_slope, want_bias=want_bias)
    for name in wgrad_kernels(ks, x.shape[2] * x.shape[3]):
        r = WGRAD_KERNELS[name][1](x, dy, ks, defer, owners, kw)
        if r is not None:
            return r
    return None


# ---- what a layer needs: forward, data gradient (the transposed shape) and weight gradient -------------------------------------
def _dgrad_fits(cin: int, cout: int, H: int, W: int, ks: int) -> int:
    """samples per group of the DATA-gradient convolution (cout -> cin channels): at an even kernel the mirrored placement's
    plan (usf_conv2d_same_pad_fits; the same LDS footprint, so the same answer as the forward placement's)"""
    lib = _ext.load()
    return lib.usf_conv2d_same_pad_fits(cout, cin, H, W, ks, ks // 2) if ks % 2 == 0 else lib.usf_conv2d_same_fits(cout, cin, H, W, ks)


def _both_convs_fit(cin: int, cout: int, H: int, W: int, ks: int) -> bool:
    if H * W >= BAND_MIN_PIXELS:        # (usf_conv2d_same_fits answers 0 there: the row-banded kernel or none)
        return train_band_ok(cin, cout, H, W, ks)
    return _ext.load().usf_conv2d_same_fits(cin, cout, H, W, ks) >= 2 and _dgrad_fits(cin, cout, H, W, ks) >= 2


def conv_shape_ok(conv, B: int, H: int, W: int, masked: bool = False) -> bool:
    """forward, data gradient and weight gradient of this nn.Conv2d at [B, cin, H, W] are all served; masked: the layer may be
    handed an input mask (the first convolution of a coupling's conditioner)"""
    ks = same_conv_ks(conv)
    if not ks:
        return False
    cin, cout = conv.in_channels, conv.out_channels
    return _both_convs_fit(cin, cout, H, W, ks) and wgrad_served(B, cin, cout, H, W, ks, masked)


def conv_ctx_shape_ok(conv, B: int, H: int, W: int) -> bool:
    """the first convolution of a conditional conditioner (C + 1 input channels, the last one the context) has a device forward,
    data gradient and weight gradient at [B, C, H, W].  It may be handed the coupling's mask; above 64 pixels conditional
    conditioners stay declined, and so does the small-map wide route"""
    ks = same_conv_ks(conv)
    if not ks or conv.in_channels < 2:
        return False
    C, cout = conv.in_channels - 1, conv.out_channels
    return (_both_convs_fit(C, cout, H, W, ks) and H * W < WIDE_MIN_PIXELS
            and wgrad_route(B, C, cout, H, W, ks, True, among=("narrow", "k4", "k5")) is not None)


def pointwise_shape_ok(conv, B: int, H: int, W: int) -> bool:
    """a kernel-1 nn.Conv2d whose forward and data gradient run on usf_pointwise_conv_f32"""
    if not pointwise_geometry(conv):
        return False
    cin, cout = conv.in_channels, conv.out_channels
    return (_ext.pointwise_conv_supported(cin, cout, False) and _ext.pointwise_conv_supported(cout, cin, False)
            and wgrad_served(B, cin, cout, H, W, 1, False))


def gate_halves_ok(conv, B: int, H: int, W: int) -> bool:
    """under the knobs ``conv_k5`` / ``conv_k4`` (either) only: GatedConv's 1 x 1 convolution C -> 2 C with more than the kernels'
    64 output channels (C = 33 .. 64: the 64 hidden channels of the hyper-parameter search) runs as TWO convolutions C -> C, the
    value rows and the gate rows of its weight (``image_training.gate_halves``), each with a device forward, data gradient and
    weight gradient"""
    if not ((config.conv_k5 or config.conv_k4) and pointwise_geometry(conv) and conv.out_channels == 2 * conv.in_channels
            and 64 < conv.out_channels <= 128):
        return False
    C = conv.in_channels
    return _ext.load().usf_conv2d_same_fits(C, C, H, W, 1) >= 2 and wgrad_served(B, C, C, H, W, 1, False)


def gate_conv_route(conv, B: int, H: int, W: int):
    """how GatedConv's 1 x 1 convolution trains at [B, cin, H, W]: "pointwise" (usf_pointwise_conv_f32), "conv" (the matrix-core
    convolution), "halves" (``gate_halves_ok``), in this order of preference, or None"""
    if pointwise_shape_ok(conv, B, H, W):
        return "pointwise"
    if conv_shape_ok(conv, B, H, W):
        return "conv"
    return "halves" if gate_halves_ok(conv, B, H, W) else None
