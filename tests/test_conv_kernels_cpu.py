"""What tests/test_conv_kernels_gpu.py rests on, proved without a GPU: the table of tests/conv_kernel_cases.py reaches every
kernel, instantiation, batch rule, patch shape, form and refusal it claims (computed from usf_conv2d_same_variant's answers
for 256 compute units, never by hand), the register-weight kernel is unreachable with default knobs, the kernels' magic-number
divisions are exact over their whole reach, the checker reports planted defects and passes the fp32 statement."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_kernel_cases as K  # noqa: E402
from usflows_amd import _ext  # noqa: E402

CUS = 256
ENTRIES = ("plain", "ctx", "res", "gate_mul", "gate_add")


@pytest.fixture(scope="module")
def lib():
    if not _ext.lib_exists():
        import __graft_entry__
        __graft_entry__.build()
    return _ext.load()


knobs = K.knobs


def _probe(lib):
    def probe(entry, B, cin, cout, H, W, ks, aligned, kn):
        kv = kn if isinstance(kn, dict) else {k: int(v) for k, v in (s.split("=") for s in kn.split(",") if s)}
        with knobs(lib, kv):
            return _ext.conv2d_same_variant(entry, B, cin, cout, H, W, ks, aligned, CUS)
    return probe


def _answers(lib):
    p = _probe(lib)
    out = []
    for c in K.cases():
        a = p(c.entry, c.B, c.cin, c.cout_arg, c.H, c.W, c.ks, not (c.xoff or c.yoff), c.knobs)
        best = p(c.entry, 1 << 20, c.cin, c.cout_arg, c.H, c.W, c.ks, not (c.xoff or c.yoff), c.knobs)["S"]
        out.append((c, a, best))
    return out


def test_the_table_is_its_rules_with_the_probes_answers(lib):
    """every row's (kernel, S, instantiation) is what the launch path's own planner says for 256 compute units"""
    rows = K.generate_rows(_probe(lib))
    assert len(rows) == len(K.ROWS) <= 160
    for got, want in zip(rows, K.ROWS):
        assert got == want
    names = [r[0] for r in K.ROWS]
    assert len(set(names)) == len(names)


def _rule_b(c, a, best):
    """B = S_best (2 * 256 + k) + r: blocks with three groups and blocks with two, a ragged last group"""
    return a["S"] == best and 2 * CUS < a["groups"] < 3 * CUS and a["grid"] == CUS and c.B % best != 0


def test_the_table_covers_what_it_claims(lib):
    ans = _answers(lib)
    for c, a, _ in ans:
        got = (a["kernel"], a["S"], a["NB"], a["CP"], a["NCT"], a["CTX"]) if a["kernel"] else (0,) * 6
        assert got == c.expect, c.name
    # wave-specialised kernel: every reachable (NB, CP, NCT, CTX), each under both batch rules
    want3 = {(nb, cp, nct, ctx) for nb, cp in ((5, 16), (9, 32), (14, 48)) for nct in (1, 2, 4) for ctx in (0, 1)}
    inst = lambda a: (a["NB"], a["CP"], a["NCT"], a["CTX"])
    small3 = {inst(a) for c, a, best in ans if a["kernel"] == 3 and (a["S"] < best or a["S"] > c.B)}
    big3 = {inst(a) for c, a, best in ans if a["kernel"] == 3 and _rule_b(c, a, best)}
    assert small3 == want3 and big3 == want3
    # 48 output channels run the four-tile instance; a 1 x 1 picture's S exceeds a small batch at 48 and 64 channels
    assert {a["NCT"] for c, a, _ in ans if a["kernel"] == 3 and c.cout == 48} == {4}
    assert {c.cout for c, a, _ in ans if a["kernel"] == 3 and c.H * c.W == 1 and a["S"] > c.B} == {48, 64}
    shapes3 = {(c.H, c.W) for c, a, _ in ans if a["kernel"] == 3}
    assert {(7, 7), (8, 8), (5, 5), (2, 2), (3, 4), (1, 1)} <= shapes3 and any(h != w for h, w in shapes3)
    # register-weight kernel: all 12 instantiations, both batch rules (its S does not depend on the batch: (a) = one group per block)
    want2 = {(nb, cp, nct, ctx) for nb, cp in ((5, 16), (9, 32)) for nct in (1, 2, 4) for ctx in (0, 1)}
    small2 = {inst(a) for c, a, best in ans if a["kernel"] == 2 and a["groups"] <= CUS}
    big2 = {inst(a) for c, a, best in ans if a["kernel"] == 2 and _rule_b(c, a, best)}
    assert small2 == want2 and big2 == want2
    assert all(c.knobs == {"conv_wsp": 0} for c, a, _ in ans if a["kernel"] == 2)
    # every form on every kernel that serves it, each fused form under both batch rules
    served = {(a["kernel"], c.entry) for c, a, _ in ans if a["kernel"]}
    assert served == {(3, e) for e in ENTRIES} | {(2, e) for e in ENTRIES[:4]} | {(1, "plain"), (1, "ctx"), (1, "gated")}
    for k, forms in ((3, ENTRIES[2:]), (2, ENTRIES[2:4])):
        assert {c.entry for c, a, best in ans if a["kernel"] == k and _rule_b(c, a, best)} >= set(forms)
    # the residual form caps S below the plain launch's (16 -> 64 at 7 x 7)
    p = _probe(lib)
    assert p("res", 1 << 20, 16, 64, 7, 7, 3, True, "")["S"] == 2 < p("plain", 1 << 20, 16, 64, 7, 7, 3, True, "")["S"] == 4
    assert any(c.entry == "res" and (c.cin, c.cout, c.H) == (16, 64, 7) and a["kernel"] == 3 and a["S"] == 2 for c, a, _ in ans)
    # the refusals: gate-add and 48 input channels on the register-weight kernel (return code 1), no first-kernel form at 48 -> 48 / 64
    refused = {c.name for c, a, _ in ans if a["kernel"] == 0}
    assert refused == {"wreg_refuses_gadd_16_16_7x7", "wreg_refuses_48_in", "refused_48_64_8x8_x_offset", "refused_ctx_48_48_8x8_wreg0"}
    # first kernel
    first = [(c, a) for c, a, _ in ans if a["kernel"] == 1]
    assert any(c.ks == 1 for c, _ in first)
    assert {1, 3, 5, 33, 64} <= {c.cin for c, _ in first if c.ks == 3} and 7 in {c.cout for c, _ in first}
    assert {(14, 14), (16, 16)} <= {(c.H, c.W) for c, _ in first} and any(c.H * c.W == 256 for c, _ in first)
    assert any(c.H * c.W == 1 and c.cout <= 32 and c.ks == 3 and c.cin in (16, 32) for c, _ in first)
    assert any(c.xoff for c, _ in first) and any(c.yoff for c, _ in first) and any(c.knobs == {"conv_wreg": 0} for c, _ in first)
    assert {a["CTX"] for _, a in first} == {0, 1}
    assert any(a["S"] == c.B < 8 for c, a in first)                                   # S clipped to the batch
    assert any(a["groups"] > 2 * a["grid"] and c.cin == 48 for c, a in first)          # 48 input channels, several groups per block
    full = {(a["PC_full"], a["PR_full"]) for _, a in first}
    ragged = {(a["PC_last"], a["PR_last"]) for c, a in first if (a["PC_last"], a["PR_last"]) != (a["PC_full"], a["PR_full"])}
    assert full == {(2, 2), (2, 1), (1, 2), (1, 1)}
    assert ragged == {(2, 1), (1, 2), (1, 1)}            # (2, 2) needs the most rows: it cannot be a SHORTER group's shape alone
    gated = [(c, a) for c, a in first if c.entry == "gated"]
    assert {c.C for c, _ in gated} == {6, 16, 20, 32} and {(a["PC_full"], a["PR_full"]) for _, a in gated} == {(2, 2), (2, 1)}
    # edge values: every slope, masked channels, no bias, both context strides
    cs = K.cases()
    assert {c.gate_slope for c in cs if "gate_slope" in c} == {0.0, 0.01, 1.0} == {c.in_slope for c in cs if c.get("in_act") == K.LEAKY}
    assert any(c.get("in_mul") == "chan" for c in cs) and any(c.get("bias") is False for c in cs)
    assert {c.ctx_stride for c in cs if c.entry == "ctx"} == {0, 1} and {c.res_sign for c in cs if c.entry == "res"} == {1.0, -1.0}


def _grid():
    for cin in (16, 32, 48):
        for cout in (16, 32, 48, 64):
            for H in range(1, 65):
                for W in range(1, 64 // H + 1):
                    yield cin, cout, H, W


BATCHES = (1, 2, 7, 100, 255, 256, 257, 1000, 4099, 65536)


def test_the_register_weight_kernel_is_unreachable_with_default_knobs(lib):
    """over the whole grid of shapes the second and third kernel accept, every entry and batch: kernel 2 never answers unless
    conv_wsp=0 -- and there its two refusals of the residual forms are gate-add alone: the staging limit (S cout H W / 4 <= 2048)
    holds for every S its planner returns, so that refusal cannot happen"""
    q = _ext.ConvVariantQuery()
    out = _ext.ConvVariant()

    def ask(entry, B, cin, cout, H, W):
        q.entry, q.aligned, q.B, q.cin, q.cout, q.H, q.W, q.ks, q.cus = _ext.CONV_ENTRIES[entry], 1, B, cin, cout, H, W, 3, CUS
        assert lib.usf_conv2d_same_variant(q, out) == 0
        return out.kernel, out.S

    hits = [(e, B, s) for s in _grid() for e in ENTRIES for B in BATCHES if ask(e, B, *s)[0] == 2]
    assert hits == []
    with knobs(lib, {"conv_wsp": 0}):
        for s in _grid():
            k, S = ask("plain", 1000, *s)
            assert k == 2 or s[0] == 48 or s[1] == 48 or ((s[2] * s[3] + 15) // 16 > 32 // ((s[1] + 15) // 16)) or k == 1
            if k == 2:
                assert S * s[1] * s[2] * s[3] // 4 <= 2048
                assert ask("res", 1000, *s) == (2, S) and ask("gate_mul", 1000, *s) == (2, S) and ask("gate_add", 1000, *s)[0] == 0
            else:
                assert ask("res", 1000, *s)[0] == 0


def test_magic_number_divisions_are_exact_over_their_reach(lib):
    """umulhi(n, floor(2^32 / d) + 1) == n // d for every n the kernels divide (the probe's maxima), all below 2^16"""
    seen = set()
    q = _ext.ConvVariantQuery()
    out = _ext.ConvVariant()
    for kn in ({}, {"conv_wsp": 0}, {"conv_small_s": 0}):
        with knobs(lib, kn):
            for cin, cout, H, W in _grid():
                for e in ENTRIES:
                    for B in (1, 100, 65536):
                        q.entry, q.aligned, q.B, q.cin, q.cout, q.H, q.W, q.ks, q.cus = _ext.CONV_ENTRIES[e], 1, B, cin, cout, H, W, 3, CUS
                        assert lib.usf_conv2d_same_variant(q, out) == 0
                        if out.kernel in (2, 3):
                            seen |= {(H * W, out.max_mHW), (W, out.max_mW), (cin * H * W, out.max_mSE), (cout * H * W, out.max_mSO)}
                            assert out.max_mHW >= out.S * H * W - 1 and out.max_mW == H * W - 1
    assert len(seen) > 100
    wrapped = 0
    for d, top in sorted(seen):
        if top < 0:
            continue
        assert top < 1 << 16
        n = np.arange(top + 1, dtype=np.uint64)
        m = (((1 << 32) // d) & 0xFFFFFFFF) + 1                # as the host computes it: (unsigned)(2^32 / d) + 1u
        if m == 1:
            # d == 1 (a 1 x 1 picture's H W, a one-pixel-wide picture's W): 2^32 + 1 wraps to 1 and umulhi(n, 1) == 0 -- the
            # kernels' cw_div takes m == 1 for n / 1 (it did not: every row of such a picture was sample 0, row 0)
            assert d == 1 and (top == 0 or not np.array_equal((n * np.uint64(1)) >> np.uint64(32), n))
            wrapped += top > 0
            continue
        assert np.array_equal((n * np.uint64(m)) >> np.uint64(32), n // np.uint64(d)), (d, top)
    assert wrapped >= 2                                       # reached as H W and as W: the table launches both


# ---- the checker ---------------------------------------------------------------------------------------------------------
def _named(name):
    return next(c for c in K.cases() if c.name == name)


def _result(c, d, y):
    buf, n = K.guarded(c)
    buf[K.GUARD:K.GUARD + n] = y.float().flatten()
    return buf


@pytest.mark.parametrize("name,defect,finding", [
    ("wsp_16_64_7x7_a", "swap", "over"), ("first_16_16_7x7_clipped", "tap_dropped", "1 elements over"),
    ("wsp_16_64_7x7_a", "bias_missing_48", "over"), ("first_16_16_2x2_wreg0_ragged", "ragged_sentinel", "left unwritten (first in sample 24)"),
    ("wsp_16_16_7x7_a", "behind", "written behind y"), ("wsp_16_48_5x5_a", "in_mul_neighbour", "over"),
    ("wsp_gmul_16_64_7x7_a", "gate_ge", "over"), ("wsp_res_16_64_7x7_a", "res_sign", "over")])
def test_the_checker_reports_a_planted_defect(name, defect, finding):
    c = _named(name)
    d = K.data(c)
    ref64, A64 = K.reference(c, d)
    clean = _result(c, d, ref64)
    assert K.check(c, clean, ref64, A64) == []
    if defect in ("swap", "ragged_sentinel", "behind"):
        bad = clean.clone()
        y = bad[K.GUARD:-K.GUARD].view(c.B, -1)
        if defect == "swap":
            y[[0, 1]] = y[[1, 0]]                        # two samples of one group
        elif defect == "ragged_sentinel":
            y[-1] = K.sentinel()
        else:
            bad[K.GUARD + y.numel()] = 0.0
    else:
        bad = _result(c, d, K.forward(c, d, torch.float64, defect=defect)[0])
    found = K.check(c, bad, ref64, A64)
    assert found and any(finding in f for f in found), found


def test_the_fp32_statement_passes_and_stays_inside_k32():
    """the fp32 statement of every case: no element over K32 * U * A (so the reference alone excludes nothing), and the
    checker passes it"""
    worst = {}
    for c in K.cases():
        d = K.data(c)
        ref64, A64 = K.reference(c, d)
        y32 = K.forward(c, d, torch.float32)[0]
        r = K.measure(c, y32, ref64, A64)
        worst[c.entry] = max(worst.get(c.entry, 0.0), r)
        assert r <= K.K32, (c.name, r)
        assert K.check(c, _result(c, d, y32), ref64, A64) == [], c.name
    print("k32 per entry:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) > 0.5 * K.K32             # K32 is the measured maximum, not a loose cap
