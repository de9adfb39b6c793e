"""What the image training path's rules answer, on a grid that sits on both sides of every boundary they have -- as data.

``python tests/golden/routes/record_image_rules.py`` adds this host's answers to ``image_rules_parent.json`` beside itself
(section "no_device", or "mi355x": the planners' answers with the device's occupancy); it was run once on each kind of host, on
the commit before the rules moved into ``usflows_amd/image_rules.py``.  ``tests/test_image_rules_cpu.py`` calls ``answers()``
again and compares.  Only public names of ``usflows_amd.image_training`` are used; nothing is launched."""
import functools
import itertools
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))

CHANNELS = (8, 16, 24, 32, 48, 64)
MAPS = ((7, 7), (7, 8), (3, 19), (8, 8), (5, 13), (9, 9), (14, 14), (16, 16))     # 49, 56, 57, 64, 65, 81, 196, 256 pixels
KERNELS = (1, 3, 4, 5)
BATCHES = (1, 300)
KNOBS = tuple(itertools.product((False, True), repeat=3))                           # (wgrad_wide, conv_k5, conv_k4)
GATE_C = (32, 33, 40, 48, 64)
AFFINE_C = (8, 12, 13, 16, 24, 32, 48, 64)


@functools.lru_cache(maxsize=None)
def _conv(*args, **kw):
    """an nn.Conv2d whose weights are never made, one per geometry: the rules only read it"""
    return torch.nn.Conv2d(*args, device="meta", **kw)


def grid():
    """(cin, cout, (H, W), ks, masked, B) in the order the packed strings follow"""
    return itertools.product(CHANNELS, CHANNELS, MAPS, KERNELS, (False, True), BATCHES)


def refused_convs():
    """(name, module) of geometries no rule may take, whatever the knobs"""
    C = _conv
    return (("stride2", C(16, 32, 3, padding=1, stride=2)), ("dilation2", C(16, 32, 3, padding=2, dilation=2)),
            ("groups2", C(16, 32, 3, padding=1, groups=2)), ("reflect", C(16, 32, 3, padding=1, padding_mode="reflect")),
            ("ks2", C(16, 32, 2, padding="same")), ("ks6", C(16, 32, 6, padding="same")), ("nonsquare", C(16, 32, (3, 1), padding="same")),
            ("ks4_pad1", C(16, 32, 4, padding=1)), ("ks4_pad2", C(16, 32, 4, padding=2)), ("ks3_pad0", C(16, 32, 3)),
            ("ks1_stride2", C(16, 32, 1, stride=2)), ("ks1_groups2", C(16, 32, 1, groups=2)), ("ks1_pad1", C(16, 32, 1, padding=1)))


class _DeviceInput:
    """what gated_tail_ok / channel_affine_train_ok read of a device tensor"""
    is_cuda, dtype = True, torch.float32

    def __init__(self, *shape):
        self.shape = tuple(shape)

    def dim(self):
        return len(self.shape)


def _bits(values) -> str:
    return "".join("1" if v else "0" for v in values)


def answers(it, config) -> dict:
    """{knob setting: {rule: packed answers}}, the rules of the grid one string per kernel size ("<rule>/ks<k>", the grid's order
    within it): an answer at kernel 4 or 5 depends on one knob, at 1 and 3 on two, so most strings recur; leaves the knobs as
    it found them"""
    conv = _conv
    keep = (config.wgrad_wide, config.conv_k5, config.conv_k4)
    out = {}
    try:
        for knobs in KNOBS:
            config.wgrad_wide, config.conv_k5, config.conv_k4 = knobs
            r = {}
            for cin, cout, (H, W), ks, masked, B in grid():
                row = {"wgrad_served": it.wgrad_served(B, cin, cout, H, W, ks, masked)}
                for tag, pad in (("same", "same"), ("int", ks // 2)):
                    row["conv_" + tag] = it.conv_shape_ok(conv(cin, cout, ks, padding=pad), B, H, W, masked=masked)
                    row["ctx_" + tag] = it.conv_ctx_shape_ok(conv(cin + 1, cout, ks, padding=pad), B, H, W)
                if ks == 1:
                    row["pointwise_0"] = it.pointwise_shape_ok(conv(cin, cout, 1), B, H, W)
                    row["pointwise_same"] = it.pointwise_shape_ok(conv(cin, cout, 1, padding="same"), B, H, W)
                for rule, v in row.items():
                    r.setdefault(f"{rule}/ks{ks}", []).append(v)
            r["gate_halves_0"] = [it.gate_halves_ok(conv(c, 2 * c, 1), B, H, W) for c, (H, W), B in itertools.product(GATE_C, MAPS, BATCHES)]
            r["gate_halves_same"] = [it.gate_halves_ok(conv(c, 2 * c, 1, padding="same"), B, H, W)
                                     for c, (H, W), B in itertools.product(GATE_C, MAPS, BATCHES)]
            r["gated_tail"] = [it.gated_tail_ok(conv(c, 2 * c, 1), _DeviceInput(B, c, H, W))
                               for c, (H, W), B in itertools.product(CHANNELS, MAPS, BATCHES)]
            r["channel_affine"] = [it.channel_affine_train_ok(_DeviceInput(B, c, H, W), c)
                                   for c, (H, W), B in itertools.product(AFFINE_C, MAPS, BATCHES)]
            r["refused"] = [f(m, 32, 7, 7) for _, m in refused_convs()
                            for f in (it.conv_shape_ok, it.conv_ctx_shape_ok, it.pointwise_shape_ok, it.gate_halves_ok)]
            out["".join(str(int(k)) for k in knobs)] = {k: _bits(v) for k, v in r.items()}
    finally:
        config.wgrad_wide, config.conv_k5, config.conv_k4 = keep
    return out


# ---- the file: {"strings": [every distinct string once], "hosts": {host: {knob setting: {rule: index into strings}}}} ------------
FIXTURE = os.path.join(HERE, "image_rules_parent.json")


def host_name() -> str:
    """the planners ask the device for its occupancy, and without one the LDS-staged form of usf_conv_wgrad_f32 has no plan: one
    recording per kind of host"""
    return "mi355x" if torch.cuda.is_available() else "no_device"


def load(path=FIXTURE) -> dict:
    """{host: {knob setting: {rule: packed answers}}}"""
    with open(path) as f:
        doc = json.load(f)
    return {h: {k: {rule: doc["strings"][i] for rule, i in by.items()} for k, by in rec.items()} for h, rec in doc["hosts"].items()}


def dump(hosts: dict, path=FIXTURE) -> None:
    strings = sorted({s for rec in hosts.values() for by in rec.values() for s in by.values()})
    at = {s: i for i, s in enumerate(strings)}
    doc = {"knob_order": ["wgrad_wide", "conv_k5", "conv_k4"], "strings": strings,
           "hosts": {h: {k: {rule: at[s] for rule, s in by.items()} for k, by in rec.items()} for h, rec in hosts.items()}}
    with open(path, "w") as f:
        f.write(json.dumps(doc, sort_keys=True).replace('"strings": [', '"strings": [\n').replace('", "', '",\n"') + "\n")


if __name__ == "__main__":
    # argv: [checkout to record from (default: this one) [, file to add this host's answers to (default: the fixture)]]
    sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.dirname(HERE))))
    from usflows_amd import image_training
    from usflows_amd.config import config as cfg
    path = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    hosts = load(path) if os.path.exists(path) else {}
    hosts[host_name()] = answers(image_training, cfg)
    dump(hosts, path)
    print(host_name(), os.path.getsize(path), "bytes")
