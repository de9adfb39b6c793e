"""What tests/test_conv4_kernels_gpu.py rests on, proved without a GPU: the table of tests/conv4_cases.py is its rules with the
planner's answers (usf_conv2d_same_variant at 256 compute units) and reaches both kernels, every instantiation of the streamed one
and the refusals, in both placements; the shapes the hyper-parameter search draws are served with two samples per group in both
placements and by the weight gradient; ks = 1, 3 and 5 plan exactly as the parent commit (recorded answers); ctx_tapmask4 against
a brute-force statement; the plane layout with the 16-tap K; the fp32 statement inside K32_4; the CPU modules at kernel_size = 4
against the live reference; the weight gradient's plan and the knob's gates."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import conv_kernel_cases as K  # noqa: E402
import conv4_cases as K4  # noqa: E402
from golden_util import LiveReference, RECORD_LIVE, live_threads, write_recorded_live  # noqa: E402
from usflows_amd import _ext  # noqa: E402
from usflows_amd.config import config  # noqa: E402

CUS = 256
ROOT = os.path.dirname(HERE)
SEARCH = (8, 16, 32, 64)                 # c_hidden of the hyper-parameter search


@pytest.fixture(scope="module")
def lib():
    if not _ext.lib_exists():
        import __graft_entry__
        __graft_entry__.build()
    return _ext.load()


def _probe(entry, B, cin, cout, H, W, ks, aligned, kn):
    assert not kn
    return _ext.conv2d_same_variant(entry, B, cin, cout, H, W, ks, aligned, CUS)


def test_the_table_is_its_rules_with_the_probes_answers(lib):
    rows = K4.generate_rows(_probe)
    assert len(rows) == len(K4.ROWS)
    for got, want in zip(rows, K4.ROWS):
        assert got == want
    names = [r[0] for r in K4.ROWS]
    assert len(set(names)) == len(names)
    # every row exists in both placements: the twin has the same shape and batch, and is a plain call
    by = {r[0]: r for r in K4.ROWS}
    for n, r in by.items():
        if not n.endswith("_m"):
            t = by[n + "_m"]
            assert t[2:8] == r[2:8] and t[1] == "plain" and "mir" in t[9].split("+") and "mir" not in r[9].split("+")
            assert t[10][:5] == r[10][:5]                              # one plan for both placements (CTX apart)
    assert len(names) == 2 * sum(1 for n in names if not n.endswith("_m"))


def test_the_table_covers_what_it_claims(lib):
    ans = []
    for c in K4.cases():
        a = _probe(c.entry, c.B, c.cin, c.cout_arg, c.H, c.W, 4, not (c.xoff or c.yoff), "")
        best = _probe(c.entry, 1 << 20, c.cin, c.cout_arg, c.H, c.W, 4, True, "")["S"]
        got = (a["kernel"], a["S"], a["NB"], a["CP"], a["NCT"], a["CTX"]) if a["kernel"] else (0,) * 6
        assert got == c.expect, c.name
        ans.append((c, a, best))
    assert all(a["lds_bytes"] <= 158 * 1024 for _, a, _ in ans)
    rule_b = lambda c, a, best: a["S"] == best and 2 * CUS < a["groups"] < 3 * CUS and a["grid"] == CUS and (best == 1 or c.B % best != 0)
    clipped = lambda c, a, best: a["S"] == c.B and (a["S"] < best or best == 1) and a["groups"] == 1
    for mirror in (False, True):
        sel = [(c, a, b) for c, a, b in ans if c.mirror == mirror]
        assert {a["kernel"] for _, a, _ in sel} == {0, 1, 4}                   # both kernels and the refusals, in each placement
        for k in (1, 4):
            for entry in (("plain",) if mirror else ("plain", "ctx")):
                assert any(rule_b(c, a, b) for c, a, b in sel if a["kernel"] == k and c.entry == entry), (k, entry, mirror)
                assert any(clipped(c, a, b) for c, a, b in sel if a["kernel"] == k and c.entry == entry), (k, entry, mirror)
        # the streamed kernel: every instantiation (row tiles per wave, CTX), each with several groups per block
        st = [(c, a, b) for c, a, b in sel if a["kernel"] == 4]
        want = {(nr, ctx) for nr in (1, 2, 4) for ctx in ((0,) if mirror else (0, 1))}
        assert {(a["PR_full"], a["CTX"]) for _, a, _ in st} == want
        assert {(a["PR_full"], a["CTX"]) for c, a, b in st if a["groups"] > a["grid"]} == want
        assert {a["NCT"] for _, a, _ in st} == {2}
        # K = 16 cp: no K padding, a whole number of slabs (the 5 x 5 table's short-slab and padded-K regimes cannot occur)
        assert all((16 * a["CP"]) % (32 * a["NB"]) == 0 for _, a, _ in st)
        assert {1, 4} <= {(c.cout + 15) // 16 for c, _, _ in st}              # one channel group of eight waves, two of four
        res = [(c, a) for c, a, _ in sel if a["kernel"] == 1]
        assert any((c.cin + 7) // 8 == 1 for c, _ in res) and any((c.cout + 15) // 16 == 3 for c, _ in res)
        shapes = {(a["PC_full"], a["PR_full"]) for _, a in res} | {(a["PC_last"], a["PR_last"]) for _, a in res}
        assert shapes == {(2, 2), (1, 2), (1, 1)}
        cs = [c for c, a, _ in sel if a["kernel"]]
        assert {1, 5, 16, 32, 33, 64} <= {c.cin for c in cs} and {7, 16, 32, 40, 64} <= {c.cout for c in cs}
        assert {(1, 1), (2, 3), (7, 7), (8, 8), (5, 13), (16, 16)} <= {(c.H, c.W) for c in cs}
        for k in (1, 4):
            assert any(c.xoff for c, a, _ in sel if a["kernel"] == k) and any(c.yoff for c, a, _ in sel if a["kernel"])
    for c, a, best in ans:
        stem = c.name[:-2] if c.name.endswith("_m") else c.name
        if stem.endswith("_a"):
            assert clipped(c, a, best), c.name
        if stem.endswith("_b"):
            assert rule_b(c, a, best), c.name
    assert {"p0", "p1", "p2", "p3", "c0", "c1"} == {c.preset for c, a, _ in ans if a["kernel"]}
    assert {c.entry for c, a, _ in ans if a["kernel"] == 0 and not c.mirror} == {"plain", "ctx"}


def test_the_required_shapes_are_served_with_two_samples_in_both_placements(lib):
    """every (cin, cout) of {8, 16, 32, 64}^2 at 7 x 7, forward (torch's placement) and data gradient (the mirrored one), and
    16 -> {8, 16, 32, 64} with the context channel; the two placements have one LDS footprint, so one answer serves both"""
    for cin in SEARCH:
        for cout in SEARCH:
            s = lib.usf_conv2d_same_fits(cin, cout, 7, 7, 4)
            assert s >= 2, (cin, cout)
            assert lib.usf_conv2d_same_pad_fits(cin, cout, 7, 7, 4, 1) == s == lib.usf_conv2d_same_pad_fits(cin, cout, 7, 7, 4, 2)
            a = _probe("plain", 1 << 16, cin, cout, 7, 7, 4, True, "")
            assert a["kernel"] in (1, 4) and a["S"] == s, (cin, cout)
            assert _ext.conv_wgrad_k4_variant(32, cin, cout, 7, 7, 4, CUS)["served"] == 1
    for cout in SEARCH:
        a = _probe("ctx", 1 << 16, 16, cout, 7, 7, 4, True, "")
        assert a["kernel"] in (1, 4) and a["S"] >= 2 and a["CTX"] == 1, cout
    # the budget the issue names: 64 -> 64 at 7 x 7, two samples, the image (86 400 B) beside a ring of two one-tap slabs (55 296 B)
    a = _probe("plain", 1 << 16, 64, 64, 7, 7, 4, True, "")
    assert (a["kernel"], a["S"], a["NB"], a["NCT"], a["lds_bytes"]) == (4, 2, 2, 2, 86400 + 55296)
    # placements the entry point refuses have no plan; odd kernels have one placement
    for ks, ok in ((4, (1, 2)), (3, (1,)), (5, (2,)), (1, (0,))):
        for pb in range(-1, 6):
            got = lib.usf_conv2d_same_pad_fits(16, 16, 7, 7, ks, pb)
            assert got == (lib.usf_conv2d_same_fits(16, 16, 7, 7, ks) if pb in ok else 0), (ks, pb)
    assert lib.usf_conv2d_same_fits(16, 16, 7, 7, 2) == 0 and lib.usf_conv2d_same_fits(16, 16, 7, 7, 6) == 0
    assert lib.usf_conv2d_same_pad_fits(16, 16, 7, 7, 6, 3) == 0 and lib.usf_conv2d_weight_elems(16, 16, 6) == -1
    assert lib.usf_conv2d_same_fits(65, 16, 7, 7, 4) == 0 and lib.usf_conv2d_same_fits(16, 16, 16, 17, 4) == 0
    # the fused forms stay kernel-3 only
    for entry in ("res", "gate_mul", "gate_add"):
        assert _probe(entry, 64, 16, 32, 7, 7, 4, True, "")["kernel"] == 0


def test_ks1_ks3_and_ks5_plan_as_the_parent_commit(lib):
    """usf_conv2d_same_fits and usf_conv2d_same_variant over {8, 16, 32, 64}^2 x {7x7, 8x8, 14x14, 16x16} x B in {1, 100, 4096} at
    256 compute units: the answers recorded once from a build of the parent commit (tests/golden/conv4/plans_parent.json)"""
    with open(os.path.join(HERE, "golden", "conv4", "plans_parent.json")) as f:
        rec = json.load(f)
    assert rec["compute_units"] == CUS
    assert len(rec["fits"]) == 3 * 16 * 4 and len(rec["variants"]) == 3 * 16 * 4 * 3 * 2
    assert {r[0] for r in rec["fits"]} == {1, 3, 5} and {r[5] for r in rec["variants"]} == {1, 100, 4096}
    for ks, cin, cout, H, W, want in rec["fits"]:
        assert lib.usf_conv2d_same_fits(cin, cout, H, W, ks) == want, (ks, cin, cout, H, W)
    fields = rec["variant_columns"][7:]
    for row in rec["variants"]:
        ks, cin, cout, H, W, B, entry = row[:7]
        a = _probe(entry, B, cin, cout, H, W, ks, True, "")
        assert sorted(a) == sorted(fields)
        assert [a[f] for f in fields] == row[7:], (ks, cin, cout, H, W, B, entry)


# ---- ctx_tapmask4 ----------------------------------------------------------------------------------------------------------
_TAPMASK_MAIN = r"""
#include "usf_common.h"
#include <cstdio>
int main() {
  for (int H = 1; H <= 6; ++H)
    for (int W = 1; W <= 6; ++W)
      for (int py = 0; py < H; ++py)
        for (int px = 0; px < W; ++px) std::printf("%d %d %d %d %u\n", H, W, py, px, usf::ctx_tapmask4(py, px, H, W));
  return 0;
}
"""


def test_ctx_tapmask4_against_brute_force(tmp_path):
    """the header's function compiled into a stand-alone host program: bit dy * 4 + dx is set exactly when 0 <= py + dy - 1 < H
    and 0 <= px + dx - 1 < W (torch's placement: one zero before, two after)"""
    src = tmp_path / "tapmask4.hip"
    src.write_text(_TAPMASK_MAIN)
    exe = tmp_path / "tapmask4"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "usflows_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    n = 0
    for line in out:
        if not line:
            continue
        H, W, py, px, got = (int(v) for v in line.split())
        want = sum(1 << (dy * 4 + dx) for dy in range(4) for dx in range(4) if 0 <= py + dy - 1 < H and 0 <= px + dx - 1 < W)
        assert got == want, (H, W, py, px, got, want)
        # ... which is what the context plane's convolution sees: the sum of a channel's taps over ones
        n += 1
    assert n == sum(h * w for h in range(1, 7) for w in range(1, 7))
    wc = torch.arange(16, dtype=torch.float64).view(1, 1, 4, 4).exp2()
    s = F.conv2d(F.pad(torch.ones(1, 1, 3, 5, dtype=torch.float64), (1, 2, 1, 2)), wc)[0, 0]
    for py in range(3):
        for px in range(5):
            assert int(s[py, px]) == sum(1 << (dy * 4 + dx) for dy in range(4) for dx in range(4) if 0 <= py + dy - 1 < 3 and 0 <= px + dx - 1 < 5)


# ---- plane layout -------------------------------------------------------------------------------------------------------------
def test_plane_layout_at_ks4(lib):
    """the binding's CPU formulation of the planes (the bits the device split gives, tests/test_conv4_kernels_gpu.py) against the
    builder that knows only the header's layout text; K = 16 cp exactly: the 16-tap form, not 4 x 4 embedded in 5 x 5"""
    ceil8, ceil16 = (lambda n: (n + 7) // 8 * 8), (lambda n: (n + 15) // 16 * 16)
    for cin in (1, 5, 8, 16, 33, 64):
        for cout in (1, 7, 16, 40, 64):
            assert lib.usf_conv2d_weight_elems(cin, cout, 4) == 3 * ceil16(cout) * 16 * ceil8(cin), (cin, cout)
    for cin, cout in ((1, 7), (5, 16), (16, 40), (33, 64), (64, 64)):
        c = K._case(("planes", "plain", 1, cin, cout, 2, 2, 4, "", "p0", (0,) * 6))
        w = K.data(c).w
        want, _ = K.planes(c, w, None)
        cp = ceil8(cin)
        assert tuple(want.shape) == (3, ceil16(cout), 16 * cp) == tuple(_ext.conv2d_planes_shape(cout, cin, 4))
        assert want.numel() == lib.usf_conv2d_weight_elems(cin, cout, 4)
        got = _ext.conv2d_weight_planes(w)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
        # tap-major, channel-minor: element [co][tap * cp + ci] of the first plane is bf16(W[co, ci, tap / 4, tap % 4])
        for co, ci, tap in ((0, 0, 0), (cout - 1, cin - 1, 15), (cout // 2, cin // 2, 6)):
            assert want[0, co, tap * cp + ci] == w[co, ci, tap // 4, tap % 4].to(torch.bfloat16)
        gt = _ext.conv2d_weight_planes(w, transposed=True)
        ct = K._case(("planes_t", "plain", 1, cout, cin, 2, 2, 4, "", "p0", (0,) * 6))
        want_t, _ = K.planes(ct, w.flip(2, 3).transpose(0, 1).contiguous(), None)
        assert torch.equal(gt.view(torch.int16), want_t.view(torch.int16))


# ---- the statements and the bound ---------------------------------------------------------------------------------------------------
def test_the_statements_are_torchs_convolution_and_its_gradient():
    """conv4_cases' placement is nn.Conv2d(..., 4, padding="same")'s, and the mirrored placement on the flipped, transposed weight
    is its data gradient (fp64)"""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 5, 6, generator=g, dtype=torch.float64, requires_grad=True)
    conv = torch.nn.Conv2d(3, 4, 4, padding="same", bias=False).double()
    y = conv(x)
    assert float((y - K4.conv4(x, conv.weight, 1)).detach().abs().max()) < 1e-14
    dy = torch.randn(2, 4, 5, 6, generator=g, dtype=torch.float64)
    (y * dy).sum().backward()
    dx = K4.conv4(dy, conv.weight.detach().flip(2, 3).transpose(0, 1), 2)
    assert float((dx - x.grad).abs().max()) < 1e-13
    imp = torch.zeros(1, 1, 5, 5, dtype=torch.float64)
    imp[0, 0, 2, 2] = 1.0
    w = torch.arange(16, dtype=torch.float64).view(1, 1, 4, 4)
    assert K4.conv4(imp, w, 1)[0, 0, 0, 0] == w[0, 0, 3, 3]           # an impulse at (2, 2) puts w[3][3] at output (0, 0)
    assert tuple(torch.nn.Conv2d(3, 4, 4, padding=2)(x.detach().float()).shape[2:]) == (6, 7)    # integer padding (2, 2): H + 1 outputs


def test_the_fp32_statement_stays_inside_k32_4():
    """the fp32 statement of every served row against the fp64 statement: no element over K32_4 * U * A, and the checker passes
    it at the device's bound"""
    worst = {}
    for c in K4.cases():
        if c.expect[0] == 0:
            continue
        d = K.data(c)
        ref64, A64 = K4.reference(c, d)
        y32 = K4.forward(c, d, torch.float32)[0]
        r = K.measure(c, y32, ref64, A64)
        key = c.entry + ("/mirrored" if c.mirror else "")
        worst[key] = max(worst.get(key, 0.0), r)
        assert r <= K4.K32_4, (c.name, r)
        buf, n = K.guarded(c)
        buf[K.GUARD:K.GUARD + n] = y32.flatten()
        assert K.check(c, buf, ref64, A64, bound=K.MARGIN * K4.K32_4) == [], c.name
    print("k32_4 per entry:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) > 0.5 * K4.K32_4          # K32_4 is the measured maximum, not a loose cap


# ---- the knob ----------------------------------------------------------------------------------------------------------------------
def test_the_knobs_give_the_kernel_size_sets(monkeypatch):
    from usflows_amd import image_training as it
    from usflows_amd import networks as N
    assert "conv_k4" in config._KNOBS and config.conv_k4 is False             # ships off
    for k4, k5, want in ((False, False, (1, 3)), (True, False, (1, 3, 4)), (False, True, (1, 3, 5)), (True, True, (1, 3, 4, 5))):
        monkeypatch.setattr(config, "conv_k4", k4)
        monkeypatch.setattr(config, "conv_k5", k5)
        assert N._conv_kernel_sizes() == want and it.train_kernel_sizes() == want


def test_the_knob_gates_training_at_kernel_size_4(monkeypatch):
    from usflows_amd import image_training as it
    conv = torch.nn.Conv2d(16, 32, 4, padding="same")
    cond = torch.nn.Conv2d(17, 32, 4, padding="same")
    monkeypatch.setattr(config, "conv_k5", False)
    monkeypatch.setattr(config, "conv_k4", False)
    assert not it.conv_shape_ok(conv, 32, 7, 7) and not it.conv_ctx_shape_ok(cond, 32, 7, 7) and not it.wgrad_served(32, 16, 32, 7, 7, 4, False)
    assert not it.gate_halves_ok(torch.nn.Conv2d(64, 128, 1), 32, 7, 7) and it.wgrad_route(32, 8, 8, 7, 7, 1, False) is None
    monkeypatch.setattr(config, "conv_k5", True)                      # the other knob does not open kernel 4
    assert not it.conv_shape_ok(conv, 32, 7, 7) and not it.wgrad_served(32, 16, 32, 7, 7, 4, False)
    monkeypatch.setattr(config, "conv_k5", False)
    monkeypatch.setattr(config, "conv_k4", True)
    assert _ext.conv_wgrad_k4_variant(32, 16, 32, 7, 7, 4, 0)["served"] == 1    # (cus = 0 asks the device; without one it plans for 256)
    assert it.conv_shape_ok(conv, 32, 7, 7, masked=True) and it.conv_ctx_shape_ok(cond, 32, 7, 7)
    for cin in SEARCH:
        for cout in SEARCH:
            assert it.conv_shape_ok(torch.nn.Conv2d(cin, cout, 4, padding="same"), 32, 7, 7), (cin, cout)
    assert not it.conv_ctx_shape_ok(torch.nn.Conv2d(17, 32, 4, padding="same"), 32, 9, 9)     # conditional first convolutions above 64 pixels
    # integer paddings at kernel 4 are not "same" (H + 1 outputs), other even kernels and kernel 5 stay closed
    assert not it.conv_shape_ok(torch.nn.Conv2d(16, 32, 4, padding=2), 32, 7, 7)
    assert not it.conv_shape_ok(torch.nn.Conv2d(16, 32, 4, padding=1), 32, 7, 7)
    assert not it.conv_ctx_shape_ok(torch.nn.Conv2d(17, 32, 4, padding=2), 32, 7, 7)
    assert not it.conv_shape_ok(torch.nn.Conv2d(16, 32, 2, padding="same"), 32, 7, 7)
    assert not it.conv_shape_ok(torch.nn.Conv2d(16, 32, 6, padding="same"), 32, 7, 7)
    assert not it.conv_shape_ok(torch.nn.Conv2d(16, 32, 5, padding="same"), 32, 7, 7)
    assert it.conv_shape_ok(torch.nn.Conv2d(16, 32, 3, padding=1), 32, 7, 7)                  # (odd kernels keep their integer form)
    # the two side routes open under either knob
    assert it.gate_halves_ok(torch.nn.Conv2d(64, 128, 1), 32, 7, 7) and it.wgrad_route(32, 8, 8, 7, 7, 1, False) == "wide"


def test_the_inference_rules_take_kernel_4_as_the_string_same_only(monkeypatch):
    """networks._conv_same_shaped's padding rule (the device predicate needs a device tensor; the rule itself does not)"""
    from usflows_amd import networks as N
    assert N._same_padding(torch.nn.Conv2d(4, 4, 4, padding="same")) and not N._same_padding(torch.nn.Conv2d(4, 4, 4, padding=2))
    assert not N._same_padding(torch.nn.Conv2d(4, 4, 4, padding=1))
    assert N._same_padding(torch.nn.Conv2d(4, 4, 3, padding=1)) and N._same_padding(torch.nn.Conv2d(4, 4, 5, padding=2))
    assert N._same_padding(torch.nn.Conv2d(4, 4, 1)) and not N._same_padding(torch.nn.Conv2d(4, 4, 3))


# ---- the CPU modules at kernel_size = 4 against the live reference ---------------------------------------------------------------
FIXTURE = os.path.join("conv4", "live_conv4")


@pytest.fixture(scope="module")
def _recording():
    with live_threads():
        yield
    if RECORD_LIVE:
        write_recorded_live()


def _reference():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import ref_shim
    return ref_shim.install()


@pytest.mark.parametrize("cls,kw", [("ConvNet2D", dict(c_in=4, c_hidden=6, num_layers=2, kernel_size=4, padding="same")),
                                    ("ConvNet2D", dict(c_in=3, c_hidden=8, num_layers=1, kernel_size=4, padding="same", gating=False,
                                                       normalize_layers=False)),
                                    ("CondConvNet2D", dict(c_in=4, c_hidden=6, num_layers=2, kernel_size=4, padding="same"))])
def test_conditioners_at_kernel_size_4_side_by_side(_recording, request, cls, kw):
    """same state-dict keys and the same bits on the CPU as the live reference's module (recorded: tests/golden/conv4/live_conv4.npz)"""
    from usflows_amd import networks as mnet
    R = LiveReference(FIXTURE, request.node.name)
    torch.manual_seed(0)
    ref = getattr(_reference()[2], cls)(**kw) if R.record else None
    mine = getattr(mnet, cls)(**kw)
    sd = R.state_dict("state_dict", lambda: ref.state_dict())
    assert list(sd.keys()) == list(mine.state_dict().keys())
    mine.load_state_dict(sd, strict=True)
    x = R.tensor("x", lambda: torch.randn(5, kw["c_in"], 7, 6))
    with torch.no_grad():
        if cls == "CondConvNet2D":
            ctx = R.tensor("ctx", lambda: torch.rand(5, 1))
            assert torch.equal(R.tensor("out", lambda: ref(x, ctx)), mine(x, ctx))
        else:
            assert torch.equal(R.tensor("out", lambda: ref(x)), mine(x))


# ---- the weight gradient's plan (usf_conv_wgrad_k4_variant, host only) ---------------------------------------------------------------
def test_the_wgrad_rows_reach_every_instantiation(lib):
    inst = _ext.conv_wgrad_k4_instances()
    assert inst == [2, 3, 6, 11, 16, 21] == _ext.conv_wgrad_k5_instances()
    used = {K4.wgrad_tiles_per_wave(ci, co) for ci in range(1, 65) for co in range(1, 65)}       # what the kernel-4 plan can ask for
    seen = set()
    for (cin, cout, H, W), nt in K4.WGRAD_ROWS:
        v = _ext.conv_wgrad_k4_variant(300, cin, cout, H, W, 4, CUS)
        assert v["served"] == 1 and v["tiles_per_wave"] == nt == K4.wgrad_tiles_per_wave(cin, cout), (cin, cout, H, W)
        assert v["T"] == 4 and v["position_parts"] == 4 and v["wave_groups"] == 4             # four tap rows of four taps
        assert v["tiles"] == -(-cout // 16) * (-(-cin // 16) * 4 + 1) <= 4 * nt and v["nacc"] == 256 * v["tiles"]
        assert v["lds_bytes"] <= 160 * 1024 and v["max_samples_per_block"] >= 3 and v["rounds"] in (1, 2)
        assert lib.usf_conv_wgrad_k4_workspace(300, cin, cout, H, W, 4) == 4 * (v["slots"] + 64) * v["nacc"] or CUS != v["cus"]
        # the LDS geometry is the 5 x 5 kernel's
        v5 = _ext.conv_wgrad_k5_variant(300, cin, cout, H, W, 5, CUS)
        assert all(v[k] == v5[k] for k in ("S", "q0", "CSx", "CSy", "nch", "lds_bytes", "CIT", "COT"))
        seen.add(nt)
    assert seen == used and sorted(seen) == inst
    v = _ext.conv_wgrad_k4_variant(32, 64, 64, 7, 7, 4, CUS)
    assert (v["tiles"], v["tiles_per_wave"]) == (68, 21)
    top = max(_ext.conv_wgrad_k4_variant(4, ci, co, H, W, 4, CUS)["lds_bytes"] for ci in (16, 32, 48, 64) for co in (16, 32, 48, 64)
              for H in range(1, 17) for W in range(1, 256 // H + 1))
    assert top == max(_ext.conv_wgrad_k4_variant(4, *s, 4, CUS)["lds_bytes"] for s, _ in K4.WGRAD_ROWS) == 163832
    for cin, cout, H, W, ks in K4.WGRAD_REFUSED:
        assert _ext.conv_wgrad_k4_variant(4, cin, cout, H, W, ks, CUS)["served"] == 0
        assert lib.usf_conv_wgrad_k4_workspace(4, cin, cout, H, W, ks) == 0
    # the other entry points keep refusing kernel 4, and the 5 x 5 entry everything but 5
    for cin in SEARCH:
        for cout in SEARCH:
            assert _ext.conv_wgrad_k5_variant(32, cin, cout, 7, 7, 4, CUS)["served"] == 0
            assert _ext.conv_wgrad_wide_variant(32, cin, cout, 7, 7, 4, CUS)["served"] == 0
            assert _ext.conv_wgrad_k4_variant(32, cin, cout, 7, 7, 5, CUS)["served"] == 0
