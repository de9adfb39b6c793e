"""What tests/test_conv5_kernels_gpu.py rests on, proved without a GPU: the table of tests/conv5_cases.py is its rules with the
planner's answers (usf_conv2d_same_variant at 256 compute units) and reaches both regimes, every instantiation of the streamed
kernel and every patch shape of the resident one; the shapes the hyper-parameter search draws are served with two samples per
group; ks = 1 and 3 plan as before; ctx_tapmask against a brute-force statement; the plane layout; the fp32 statement inside
K32_5; the CPU modules at kernel_size = 5 against the live reference; the weight gradient's plan and the knob's gates."""
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import conv_kernel_cases as K  # noqa: E402
import conv5_cases as K5  # noqa: E402
from golden_util import LiveReference, RECORD_LIVE, live_threads, write_recorded_live  # noqa: E402
from usflows_amd import _ext  # noqa: E402
from usflows_amd.config import config  # noqa: E402

CUS = 256
ROOT = os.path.dirname(HERE)


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
    rows = K5.generate_rows(_probe)
    assert len(rows) == len(K5.ROWS)
    for got, want in zip(rows, K5.ROWS):
        assert got == want
    names = [r[0] for r in K5.ROWS]
    assert len(set(names)) == len(names)


def test_the_table_covers_what_it_claims(lib):
    ans = []
    for c in K5.cases():
        a = _probe(c.entry, c.B, c.cin, c.cout_arg, c.H, c.W, 5, not (c.xoff or c.yoff), "")
        best = _probe(c.entry, 1 << 20, c.cin, c.cout_arg, c.H, c.W, 5, True, "")["S"]
        got = (a["kernel"], a["S"], a["NB"], a["CP"], a["NCT"], a["CTX"]) if a["kernel"] else (0,) * 6
        assert got == c.expect, c.name
        ans.append((c, a, best))
    assert {a["kernel"] for _, a, _ in ans} == {0, 1, 4}                       # both regimes and the refusals
    assert all(a["lds_bytes"] <= 158 * 1024 for _, a, _ in ans)
    rule_b = lambda c, a, best: a["S"] == best and 2 * CUS < a["groups"] < 3 * CUS and a["grid"] == CUS and (best == 1 or c.B % best != 0)
    clipped = lambda c, a, best: a["S"] == c.B and (a["S"] < best or best == 1) and a["groups"] == 1
    for k in (1, 4):
        for entry in ("plain", "ctx"):
            assert any(rule_b(c, a, b) for c, a, b in ans if a["kernel"] == k and c.entry == entry), (k, entry)
            assert any(clipped(c, a, b) for c, a, b in ans if a["kernel"] == k and c.entry == entry), (k, entry)
    for c, a, best in ans:
        if c.name.endswith("_a"):
            assert clipped(c, a, best), c.name
        if c.name.endswith("_b"):
            assert rule_b(c, a, best), c.name
    # the streamed kernel: every instantiation (row tiles per wave, CTX), each with several groups per block; both slab sizes;
    # walks of an odd and of an even number of slabs; a last slab that is short; K padded beyond 25 cp
    st = [(c, a, b) for c, a, b in ans if a["kernel"] == 4]
    want = {(nr, ctx) for nr in (1, 2, 4) for ctx in (0, 1)}
    assert {(a["PR_full"], a["CTX"]) for _, a, _ in st} == want
    assert {(a["PR_full"], a["CTX"]) for c, a, b in st if a["groups"] > a["grid"]} == want
    assert {a["NB"] for _, a, _ in st} == {1, 2} and {a["NCT"] for _, a, _ in st} == {2}
    kp = lambda a: (25 * a["CP"] + 31) // 32 * 32
    slabs = lambda a: -(-kp(a) // (32 * a["NB"]))
    assert {slabs(a) % 2 for _, a, _ in st} == {0, 1}
    assert any(kp(a) % (32 * a["NB"]) for _, a, _ in st) and any(kp(a) != 25 * a["CP"] for _, a, _ in st)
    assert {1, 2} <= {(c.cout + 15) // 16 for c, _, _ in st} and any((c.cout + 15) // 16 == 3 for c, _, _ in st)
    # the resident kernel: K 200 -> 224 (cp = 8), every patch shape a plain / ctx group can take
    res = [(c, a) for c, a, _ in ans if a["kernel"] == 1]
    assert any((c.cin + 7) // 8 == 1 for c, _ in res)
    shapes = {(a["PC_full"], a["PR_full"]) for _, a in res} | {(a["PC_last"], a["PR_last"]) for _, a in res}
    assert shapes == {(2, 2), (1, 2), (1, 1)}
    cs = [c for c, a, _ in ans if a["kernel"]]
    assert {1, 5, 16, 33, 64} <= {c.cin for c in cs} and {7, 16, 40, 64} <= {c.cout for c in cs}
    assert {(1, 1), (2, 3), (7, 7), (8, 8), (5, 13), (16, 16)} <= {(c.H, c.W) for c in cs}
    assert {"p0", "p1", "p2", "p3", "c0", "c1"} == {c.preset for c in cs}
    for k in (1, 4):
        assert any(c.xoff for c, a, _ in ans if a["kernel"] == k) and any(c.yoff or c.xoff for c, a, _ in ans if a["kernel"] == k)
    assert any(c.yoff for c in cs)
    assert {c.entry for c, a, _ in ans if a["kernel"] == 0} == {"plain", "ctx"}


def test_the_required_shapes_are_served_with_two_samples(lib):
    """every (cin, cout) of {8, 16, 32, 64}^2 at 7 x 7 (both orientations: the data gradient runs the transposed shape), and
    16 -> {8, 16, 32, 64} with the context channel"""
    for cin in (8, 16, 32, 64):
        for cout in (8, 16, 32, 64):
            assert lib.usf_conv2d_same_fits(cin, cout, 7, 7, 5) >= 2, (cin, cout)
            a = _probe("plain", 1 << 16, cin, cout, 7, 7, 5, True, "")
            assert a["kernel"] in (1, 4) and a["S"] == lib.usf_conv2d_same_fits(cin, cout, 7, 7, 5), (cin, cout)
    for cout in (8, 16, 32, 64):
        a = _probe("ctx", 1 << 16, 16, cout, 7, 7, 5, True, "")
        assert a["kernel"] in (1, 4) and a["S"] >= 2 and a["CTX"] == 1, cout
    # the budget the streamed kernel was laid out for: 64 -> 64 at 7 x 7, two samples, a ring of two one-tap slabs
    a = _probe("plain", 1 << 16, 64, 64, 7, 7, 5, True, "")
    assert (a["kernel"], a["S"], a["NB"], a["NCT"], a["lds_bytes"]) == (4, 2, 2, 2, 159840)
    assert lib.usf_conv2d_weight_elems(64, 64, 5) == 3 * 64 * 1600 and lib.usf_conv2d_weight_elems(5, 7, 5) == 3 * 16 * 224
    assert lib.usf_conv2d_weight_elems(16, 16, 7) == -1 and lib.usf_conv2d_same_fits(16, 16, 7, 7, 7) == 0
    assert lib.usf_conv2d_same_fits(65, 16, 7, 7, 5) == 0 and lib.usf_conv2d_same_fits(16, 16, 16, 17, 5) == 0


def _fits_before(cin, cout, H, W, ks):
    """usf_conv2d_same_fits at ks 1 / 3 as it was before ks = 5: the first kernel's LDS image and staging registers"""
    if min(cin, cout, H, W) <= 0 or cin > 64 or cout > 64 or H * W > 256 or ks not in (1, 3):
        return 0
    cp, coutp = (cin + 7) // 8 * 8, (cout + 15) // 16 * 16
    kp = (ks * ks * cp + 31) // 32 * 32
    PP = (H + 2 * (ks // 2)) * (W + 2 * (ks // 2))
    for S in range(8, 0, -1):
        lds = 3 * coutp * ((kp // 8) | 1) * 16 + 3 * S * PP * ((cp // 8) | 1) * 16
        if lds <= 158 * 1024 and ((S * ((cin + 1) // 2) + 7) // 8) * ((H * W + 63) // 64) <= 16:
            return S
    return 0


def test_ks1_and_ks3_plan_as_before(lib):
    """over the shapes tests/test_image_flows.py launches and its random sweep's ranges"""
    import random
    shapes = [(1, 1, 1, 1, 1), (16, 32, 7, 7, 3), (32, 32, 7, 7, 3), (32, 64, 7, 7, 1), (32, 16, 7, 7, 3), (48, 32, 8, 8, 3), (4, 32, 14, 14, 3),
              (5, 7, 3, 9, 3), (32, 32, 16, 16, 3), (64, 64, 5, 5, 1), (33, 17, 5, 6, 1), (64, 64, 16, 16, 3)]
    rnd = random.Random(1234)
    for _ in range(4000):
        H = rnd.randint(1, 16)
        shapes.append((rnd.randint(1, 64), rnd.randint(1, 64), H, rnd.randint(1, min(16, 256 // H)), rnd.choice([1, 3])))
    for s in shapes:
        assert lib.usf_conv2d_same_fits(*s) == _fits_before(*s), s
        a = _probe("plain", 1000, *s, True, "")
        assert a["kernel"] != 4 and (a["kernel"] != 0 or _fits_before(*s) == 0), s


# ---- ctx_tapmask -----------------------------------------------------------------------------------------------------------
_TAPMASK_MAIN = r"""
#include "usf_common.h"
#include <cstdio>
int main() {
  for (int ks = 3; ks <= 5; ks += 2)
    for (int H = 1; H <= 6; ++H)
      for (int W = 1; W <= 6; ++W)
        for (int py = 0; py < H; ++py)
          for (int px = 0; px < W; ++px) std::printf("%d %d %d %d %d %u\n", ks, H, W, py, px, ks == 5 ? usf::ctx_tapmask5(py, px, H, W) : usf::ctx_tapmask(py, px, H, W, ks));
  return 0;
}
"""


def test_ctx_tapmask_against_brute_force(tmp_path):
    """the header's functions (ctx_tapmask for ks = 3, ctx_tapmask5) compiled into a stand-alone host program: bit dy * ks + dx is set exactly when tap (dy, dx) of
    output pixel (py, px) reads inside the H x W image -- ks = 5, and ks = 3 as before"""
    src = tmp_path / "tapmask.hip"
    src.write_text(_TAPMASK_MAIN)
    exe = tmp_path / "tapmask"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "usflows_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    n = 0
    for line in out:
        if not line:
            continue
        ks, H, W, py, px, got = (int(v) for v in line.split())
        want = sum(1 << (dy * ks + dx) for dy in range(ks) for dx in range(ks)
                   if 0 <= py + dy - ks // 2 < H and 0 <= px + dx - ks // 2 < W)
        assert got == want, (ks, H, W, py, px, got, want)
        n += 1
    assert n == 2 * sum(h * w for h in range(1, 7) for w in range(1, 7))


# ---- plane layout -------------------------------------------------------------------------------------------------------------
def test_plane_layout_at_ks5(lib):
    """the binding's CPU formulation of the planes (the bits the device split gives, tests/test_conv5_kernels_gpu.py) against the
    builder that knows only the header's layout text; sizes from usf_conv2d_weight_elems"""
    for cin, cout in ((1, 7), (5, 16), (16, 40), (33, 64), (64, 64)):
        c = K._case(("planes", "plain", 1, cin, cout, 2, 2, 5, "", "p0", (0,) * 6))
        w = K.data(c).w
        want, _ = K.planes(c, w, None)
        cp = (cin + 7) // 8 * 8
        assert tuple(want.shape) == (3, (cout + 15) // 16 * 16, (25 * cp + 31) // 32 * 32) == tuple(_ext.conv2d_planes_shape(cout, cin, 5))
        assert want.numel() == lib.usf_conv2d_weight_elems(cin, cout, 5)
        got = _ext.conv2d_weight_planes(w)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
        # tap-major, channel-minor: element [co][tap * cp + ci] of the first plane is bf16(W[co, ci, tap / 5, tap % 5])
        for co, ci, tap in ((0, 0, 0), (cout - 1, cin - 1, 24), (cout // 2, cin // 2, 7)):
            assert want[0, co, tap * cp + ci] == w[co, ci, tap // 5, tap % 5].to(torch.bfloat16)
        gt = _ext.conv2d_weight_planes(w, transposed=True)
        ct = K._case(("planes_t", "plain", 1, cout, cin, 2, 2, 5, "", "p0", (0,) * 6))
        want_t, _ = K.planes(ct, w.flip(2, 3).transpose(0, 1).contiguous(), None)
        assert torch.equal(gt.view(torch.int16), want_t.view(torch.int16))


# ---- the bound ------------------------------------------------------------------------------------------------------------------
def test_the_fp32_statement_stays_inside_k32_5():
    """the fp32 statement of every served row against the fp64 statement: no element over K32_5 * U * A, and the checker passes
    it at the device's bound"""
    worst = {}
    for c in K5.cases():
        if c.expect[0] == 0:
            continue
        d = K.data(c)
        ref64, A64 = K.reference(c, d)
        y32 = K.forward(c, d, torch.float32)[0]
        r = K.measure(c, y32, ref64, A64)
        worst[c.entry] = max(worst.get(c.entry, 0.0), r)
        assert r <= K5.K32_5, (c.name, r)
        buf, n = K.guarded(c)
        buf[K.GUARD:K.GUARD + n] = y32.flatten()
        assert K.check(c, buf, ref64, A64, bound=K.MARGIN * K5.K32_5) == [], c.name
    print("k32_5 per entry:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) > 0.5 * K5.K32_5          # K32_5 is the measured maximum, not a loose cap


# ---- the knob ----------------------------------------------------------------------------------------------------------------------
def test_the_knob_gates_the_kernel_size(monkeypatch):
    from usflows_amd import networks as N
    assert "conv_k5" in config._KNOBS
    monkeypatch.setattr(config, "conv_k5", False)
    assert N._conv_kernel_sizes() == (1, 3)
    monkeypatch.setattr(config, "conv_k5", True)
    assert N._conv_kernel_sizes() == (1, 3, 5)


# ---- the CPU modules at kernel_size = 5 against the live reference ---------------------------------------------------------------
FIXTURE = os.path.join("conv5", "live_conv5")


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


@pytest.mark.parametrize("cls,kw", [("ConvNet2D", dict(c_in=4, c_hidden=6, num_layers=2, kernel_size=5, padding="same")),
                                    ("ConvNet2D", dict(c_in=3, c_hidden=8, num_layers=1, kernel_size=5, padding="same", gating=False,
                                                       normalize_layers=False)),
                                    ("CondConvNet2D", dict(c_in=4, c_hidden=6, num_layers=2, kernel_size=5, padding="same"))])
def test_conditioners_at_kernel_size_5_side_by_side(_recording, request, cls, kw):
    """same state-dict keys and the same bits on the CPU as the live reference's module (recorded: tests/golden/conv5/live_conv5.npz)"""
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


# ---- the weight gradient's plan (usf_conv_wgrad_k5_variant, host only) ---------------------------------------------------------------
def test_the_wgrad_rows_reach_every_instantiation(lib):
    inst = _ext.conv_wgrad_k5_instances()
    assert inst == [2, 3, 6, 11, 16, 21] and max(inst) <= 37
    seen = set()
    for (cin, cout, H, W), nt in K5.WGRAD_ROWS:
        v = _ext.conv_wgrad_k5_variant(300, cin, cout, H, W, 5, CUS)
        assert v["served"] == 1 and v["tiles_per_wave"] == nt == K5.wgrad_tiles_per_wave(cin, cout), (cin, cout, H, W)
        assert v["T"] == 5 and v["position_parts"] == 5 and v["wave_groups"] == 4             # five tap rows of five taps
        assert v["tiles"] == -(-cout // 16) * (-(-cin // 16) * 5 + 1) <= 4 * nt and v["nacc"] == 256 * v["tiles"]
        assert v["lds_bytes"] <= 160 * 1024 and v["max_samples_per_block"] >= 3 and v["rounds"] in (1, 2)
        assert lib.usf_conv_wgrad_k5_workspace(300, cin, cout, H, W, 5) == 5 * (v["slots"] + 64) * v["nacc"] or CUS != v["cus"]
        seen.add(nt)
    assert sorted(seen) == inst
    # the largest LDS image any served shape has is in the table
    top = max(_ext.conv_wgrad_k5_variant(4, ci, co, H, W, 5, CUS)["lds_bytes"] for ci in (16, 32, 48, 64) for co in (16, 32, 48, 64)
              for H in range(1, 17) for W in range(1, 256 // H + 1))
    assert top == max(_ext.conv_wgrad_k5_variant(4, *s, 5, CUS)["lds_bytes"] for s, _ in K5.WGRAD_ROWS) == 163832
    for cin, cout, H, W, ks in K5.WGRAD_REFUSED:
        assert _ext.conv_wgrad_k5_variant(4, cin, cout, H, W, ks, CUS)["served"] == 0
    # every (cin, cout) of the hyper-parameter search at 7 x 7, and the existing entry points' refusal of kernel 5
    for cin in (8, 16, 32, 64):
        for cout in (8, 16, 32, 64):
            assert _ext.conv_wgrad_k5_variant(32, cin, cout, 7, 7, 5, CUS)["served"] == 1
            assert _ext.conv_wgrad_wide_variant(32, cin, cout, 7, 7, 5, CUS)["served"] == 0


def test_the_knob_gates_training_at_kernel_size_5(monkeypatch):
    from usflows_amd import image_training as it
    conv = torch.nn.Conv2d(16, 32, 5, padding="same")
    cond = torch.nn.Conv2d(17, 32, 5, padding="same")
    monkeypatch.setattr(config, "conv_k5", False)
    assert it.train_kernel_sizes() == (1, 3)
    assert not it.conv_shape_ok(conv, 32, 7, 7) and not it.conv_ctx_shape_ok(cond, 32, 7, 7) and not it.wgrad_served(32, 16, 32, 7, 7, 5, False)
    monkeypatch.setattr(config, "conv_k5", True)
    assert _ext.conv_wgrad_k5_variant(32, 16, 32, 7, 7, 5, 0)["served"] == 1    # (cus = 0 asks the device; without one it plans for 256)
    assert it.conv_shape_ok(conv, 32, 7, 7, masked=True) and it.conv_ctx_shape_ok(cond, 32, 7, 7)
    assert not it.conv_ctx_shape_ok(torch.nn.Conv2d(17, 32, 5, padding="same"), 32, 9, 9)     # conditional first convolutions above 64 pixels
    assert not it.conv_shape_ok(torch.nn.Conv2d(16, 32, 4, padding="same"), 32, 7, 7)
