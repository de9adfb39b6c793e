"""What tests/test_image_grad_kernels_gpu.py rests on, proved without a GPU: the tables of tests/image_grad_cases.py are their
rules with the planners' own answers (usf_conv_wgrad_variant for 256 compute units, usf_layernorm_channels_bwd_variant) and
reach every instantiation, batch regime, rsplit value, reduction depth and refusal they claim; the LDS-staged kernel's
addressing stays inside its images for every shape it serves; the direct kernel's four position blocks take every position
once; the checker reports planted defects; the fp32 statements stay inside the measured constants."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_grad_cases as G  # noqa: E402
from usflows_amd import _ext  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    if not _ext.lib_exists():
        import __graft_entry__
        __graft_entry__.build()
    return _ext.load()


def _wg_probe(lib):
    def probe(B, cin, cout, H, W, ks, masked, kn, bpc=G.BLOCKS_PER_CU):
        with G.knobs(lib, kn):
            return _ext.conv_wgrad_variant(B, cin, cout, H, W, ks, masked, G.CUS, bpc)
    return probe


def test_the_tables_are_their_rules_with_the_probes_answers(lib):
    wg, ln = G.generate_rows(_wg_probe(lib), _ext.layernorm_channels_bwd_variant)
    assert len(wg) == len(G.WG_ROWS) and len(ln) == len(G.LN_ROWS)
    for got, want in zip(wg + ln, G.WG_ROWS + G.LN_ROWS):
        assert got == want
    names = [r[0] for r in G.WG_ROWS + G.LN_ROWS + G.GR_ROWS + G.CTX_ROWS]
    assert len(set(names)) == len(names)
    assert 150 <= len(G.WG_ROWS) + len(G.LN_ROWS) + len(G.GR_ROWS) + len(G.CTX_ROWS) + len(G.JOB_GROUPS) <= 240
    assert all(c.B <= 300 and c.H * c.W <= 65 for c in G.wg_cases())


def test_no_expectation_depends_on_the_devices_occupancy_answer(lib):
    """every row plans the same grid for 1, 2, 4 and 8 resident blocks per compute unit and for 80, 256 and 304 compute units: the GPU
    file may compare `blocks` on whatever device it runs"""
    p = _wg_probe(lib)
    for c in G.wg_cases():
        if c.B > 0:
            for bpc in (1, 2, 4, 8):
                assert G.wg_expect(p(c.B, c.cin, c.cout, c.H, c.W, c.ks, c.mask, c.knobs, bpc)) == c.expect, (c.name, bpc)
            for cus in (80, 304):
                with G.knobs(lib, c.knobs):
                    assert G.wg_expect(_ext.conv_wgrad_variant(c.B, c.cin, c.cout, c.H, c.W, c.ks, c.mask, cus, 1)) == c.expect, (c.name, cus)
    # the occupancy cap itself, through the probe: 256 x min(bpc, 4) blocks of the LDS-staged kernel, 256 x min(bpc, 8) of the direct one
    assert [p(65536, 32, 32, 7, 7, 3, False, {}, b)["blocks"] for b in (1, 3, 4, 9)] == [256, 768, 1024, 1024]
    assert [p(65536, 32, 32, 7, 7, 1, False, {}, b)["blocks"] for b in (1, 8, 9)] == [256, 2048, 2048]
    assert p(65536, 32, 32, 7, 7, 3, False, {"conv_wgrad_blocks": 5})["blocks"] == 5
    a = p(65536, 32, 32, 7, 7, 3, False, {})
    assert a["max_samples_per_wave"] == 64 and a["slots"] == 1024 and (a["rounds"], a["rows_used"], a["per"]) == (2, 64, 16)


def test_the_knob_defaults_of_the_case_tables_are_the_sources():
    """conv_kernel_cases.KNOB_DEFAULTS (what the knob context restores a never-set knob to) against every tuning("name", default)
    of the kernels' host code"""
    import glob
    import re
    from conv_kernel_cases import KNOB_DEFAULTS
    found = {}
    for path in glob.glob(os.path.join(os.path.dirname(_ext.__file__), "csrc", "*.hip")):
        for name, dflt in re.findall(r'tuning\("(\w+)",\s*(-?\d+)\)', open(path).read()):
            found.setdefault(name, set()).add(int(dflt))
    for name, dflt in KNOB_DEFAULTS.items():
        assert found.get(name) == {dflt}, (name, found.get(name))


def _regime(c):
    e = c.expect
    if e[0] == 0 or c.rc != 0:
        return None
    if c.knobs.get("conv_wgrad_blocks") == 2 and e[9] == 3:
        nsw = 4 * e[5] // e[4]
        return "b" if c.B > 2 * nsw and c.B % nsw else None
    return "a" if e[9] == 1 and not c.knobs else None


def test_the_tables_cover_what_they_claim(lib):
    cs = G.wg_cases()
    inst = lambda c: c.expect[:4]
    want = {(1, i, j, 9) for i, j in G.T9_TILES} | {(1, i, j, 1) for i, j in G.T1_TILES} | {(2, i, j, 1) for i, j in G.T1_TILES}
    assert len(want) == 40
    src = open(os.path.join(os.path.dirname(_ext.__file__), "csrc", "usf_image_grad.hip")).read()
    import re
    mac = lambda name: re.findall(r"X\((\d), (\d)(?:, (\d))?\)", src.split(f"#define {name}(X)")[1].split("\n\n")[0])
    assert {(1, int(i), int(j), int(t)) for i, j, t in mac("USF_WG_INSTANCES")} | \
        {(2, int(i), int(j), 1) for i, j, _ in mac("USF_WG_K1_INSTANCES")} == want          # written out == the source's lists: 24 + 16
    a = {inst(c) for c in cs if _regime(c) == "a"}
    b = {inst(c) for c in cs if _regime(c) == "b"}
    assert a == want and b == want
    # regime (a): the grid is ceil(B rsplit / 4); regime (b): two blocks, waves of three and of two samples
    assert all(c.expect[5] == (c.B * c.expect[4] + 3) // 4 for c in cs if _regime(c) == "a")
    assert all(c.expect[5] == 2 for c in cs if _regime(c) == "b") and {c.expect[4] for c in cs if _regime(c) == "b"} >= {1, 4}
    # the forms: all four on every LDS-staged instantiation, plain and pre_sub + slope on every direct one
    for k in want:
        assert {c.form for c in cs if inst(c) == k and c.rc == 0} >= (set(G.FORMS) if k[0] == 1 else {"plain", "presub_leaky"}), k
    # pictures: both kernel sizes on the LDS-staged kernel, every H W of the direct kernel, single rows, 48 pixels
    for ks in (1, 3):
        assert {(c.H, c.W) for c in cs if c.expect[0] == 1 and c.ks == ks} >= set(G.PICTURES)
    assert {c.H * c.W for c in cs if c.expect[0] == 2} == set(range(49, 65))
    assert {c.W for c in cs if c.expect[0] == 2 and c.H == 1} >= {49, 53, 59, 61, 64}
    assert any(c.H * c.W == 48 and c.ks == 1 and not c.mask and c.expect[0] == 1 for c in cs)
    # rsplit
    by = {c.name: c for c in cs}
    assert [by[f"rs_B{B}"].expect[4] for B in (64, 65, 128, 129)] == [4, 2, 2, 1]
    assert [by[f"rs_nch{n}"].expect[4] for n in (3, 4, 7, 8)] == [1, 2, 2, 4]
    p = _wg_probe(lib)
    for n, (H, W) in G.NCH_PICTURES.items():
        assert p(9, 16, 32, H, W, 3, False, {})["nch"] == n
    assert [by[n].expect[4] for n in ("rs_B64_off", "rs_B128_off", "rs_nch8_off")] == [1, 1, 1]
    assert {c.expect[4] for c in cs if c.expect[0] == 1 and c.ks == 1} == {1} == {c.expect[4] for c in cs if c.expect[0] == 2}
    # the sum over the slots: 64 in one round, 68 in two with a ragged last row, 80 in two even rows, 300 at B = 300
    red = lambda n: (by[n].expect[5] * 4,) + by[n].expect[6:9]
    assert red("red_64_slots") == (64, 1, 1, 64) and red("red_68_slots") == (68, 2, 5, 14) and 68 % 14
    assert red("red_80_slots") == (80, 2, 5, 16) and red("red_300_slots_k3") == (300, 2, 19, 16) == red("red_300_slots_k1_direct") and 300 % 16
    assert max(c.expect[5] * 4 for c in cs if not c.knobs) == 300
    # a finding: rsplit = 4 at B = 64 makes 256 slots -- two rounds, not the one round wgrad_plan's comment promises
    assert red("rs_B64") == (256, 2, 16, 16)
    # refusals and argument checks
    assert {c.name: c.rc for c in cs if c.rc} == {
        "ref_cin_24": 1, "ref_cout_40": 1, "ref_tiles_3x3_k3": 1, "ref_no_instance_16_64_k3": 1, "ref_no_instance_64_16_k3": 1, "ref_W1": 1, "ref_65_pixels": 1, "ref_lds_1x64_32_32_k3": 1, "ref_lds_8x8_64_64_k1_masked": 1, "ref_B0": -2,
        "ref_x_offset": -2, "ref_short_workspace": -2}
    assert all(c.expect[0] == 0 for c in cs if c.rc == 1)
    # ... the LDS refusal is the LDS size and nothing else: the same picture is served at 16 + 16 channels
    assert by["pic_1x64_k3"].expect[0] == 1 and p(9, 16, 16, 1, 64, 3, False, {})["lds_bytes"] <= 160 * 1024 < \
        4 * (p(9, 16, 16, 1, 64, 3, False, {})["tab_floats"] + 4 * (64 * p(9, 16, 16, 1, 64, 3, False, {})["CS"] + 4))
    # the job groups: one tile shape each, pictures / batches / rsplit / mask / pre_sub differ, one group with unequal LDS sizes
    for g, members in G.JOB_GROUPS.items():
        ms = [by[m] for m in members]
        assert 3 <= len(ms) <= 6 and len({c.expect[1:4] for c in ms}) == 1 and all(c.expect[0] == 1 for c in ms), g
        assert len({(c.H, c.W, c.B) for c in ms}) >= 3
    assert {by[m[0]].expect[3] for m in G.JOB_GROUPS.values()} == {1, 9}
    assert len({by[m].expect[4] for m in G.JOB_GROUPS["jobs_T9_1x1"]}) == 3
    lds = [p(c.B, c.cin, c.cout, c.H, c.W, c.ks, c.mask, c.knobs)["lds_bytes"] for c in map(by.get, G.JOB_GROUPS["jobs_T1_1x1_mixed_lds"])]
    assert max(lds) > 2 * min(lds)
    # LayerNorm: the 7 branches, the channel counts at their edges, every nonlinearity on each kernel family, small and ragged B P,
    # the block cap on each family, a refusal
    ln = G.ln_cases()
    assert {c.expect[:2] for c in ln if c.rc == 0} == {(1, 16), (1, 32), (1, 64), (2, 8), (2, 16), (2, 24), (2, 32)}
    assert {c.C for c in ln} >= {1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64}
    for fam in (1, 2):
        assert {(c.act, c.slope) for c in ln if c.expect[0] == fam} == {(G.NONE, 0.0), (G.LEAKY, 0.0), (G.LEAKY, 0.1)}
        assert any(c.expect[2] == 2048 and c.B * c.P == 2048 * 256 + 1 for c in ln if c.expect[0] == fam)
        assert any(c.B * c.P < 32 for c in ln if c.expect[0] == fam) and any(c.B * c.P % 32 for c in ln if c.expect[0] == fam)
    assert {c.expect[3] for c in ln if c.rc == 0} == {1, 2}
    assert [c.name for c in ln if c.rc] == ["ln_ref_C65"]
    assert any(c.act == G.LEAKY and c.slope == 0.0 and bool((G.ln_data(c).x == 0).any()) for c in ln)
    # gated residual and context gradient
    gr = {c.name: c for c in G.gr_cases()}
    assert gr["gr_ragged"].B * gr["gr_ragged"].CP % 256 and gr["gr_cap"].B * gr["gr_cap"].CP > 256 * 64 * 256 and gr["gr_empty"].B == 0
    cx = G.ctx_cases()
    assert {(c.ks, c.ctx_stride) for c in cx} == {(1, 0), (1, 1), (3, 0), (3, 1)} and {c.B for c in cx} == {1, 37}
    assert {(c.H, c.W) for c in cx} == {(1, 1), (1, 5), (5, 1), (7, 7), (8, 8)} and any(c.B * c.H * c.W % 256 for c in cx if c.B > 1)
    # exact zeros: in x, and in x - pre_sub, once per kernel family at the least
    for fam in (1, 2):
        c = next(c for c in cs if c.expect[0] == fam and c.pre_sub and c.rc == 0)
        d = G.wg_data(c)
        assert bool((d.x == 0).any()) and bool((d.x - d.pre_sub.view(1, -1, 1, 1) == 0).any())


# ---- the LDS-staged kernel's addressing, from the probe's geometry ---------------------------------------------------------------
def _shapes():
    for H in range(1, 65):
        for W in range(2, 64 // H + 1):
            yield H, W


def test_lds_addressing_of_the_staged_kernel_stays_inside_its_images(lib):
    """a numpy model of conv_wgrad_body's staging and fragment reads over every served (H, W, ks, cin, cout): all it knows of
    the kernel is the index arithmetic, all it knows of the plan is the probe's answer"""
    p = _wg_probe(lib)
    n_served = 0
    e4096 = np.arange(4096, dtype=np.uint64)
    for H, W in _shapes():
        HW = H * W
        m_hw, m_w = ((1 << 32) + HW - 1) // HW, ((1 << 32) + W - 1) // W
        assert np.array_equal((e4096 * np.uint64(m_hw)) >> np.uint64(32), e4096 // np.uint64(HW))      # element -> channel: e < 64 * 64
        assert np.array_equal((e4096 * np.uint64(m_w)) >> np.uint64(32), e4096 // np.uint64(W))
        for ks in (1, 3):
            geo = {}
            for cin in (16, 32, 48, 64):
                for cout in (16, 32, 48, 64):
                    a = p(9, cin, cout, H, W, ks, True, {})
                    if not a["kernel"]:
                        continue
                    assert a["kernel"] == 1
                    n_served += 1
                    wsz = (cin + cout) * a["CS"] + 4
                    assert a["lds_bytes"] == 4 * (a["tab_floats"] + 4 * wsz) <= 160 * 1024 and wsz - 4 < 1 << 16      # table entries are u16
                    assert a["tab_floats"] % 4 == 0 and a["tab_floats"] >= (a["CIT"] + a["COT"]) * 512 + a["CIT"] * 1024 + cin
                    geo[(a["S"], a["base"], a["q0"], a["CS"], a["nch"])] = 1
            if not geo:
                continue
            assert len(geo) == 1                                   # the picture's geometry does not depend on the channel counts
            S, base, q0, CS, nch = next(iter(geo))
            assert CS % 2 == 0 and (CS // 2) % 2 == 1
            pix = np.arange(HW)
            staged = base + pix + (pix // W) * (S - W)             # lidx within a channel
            assert len(set(staged.tolist())) == HW and staged.min() >= 0 and staged.max() < CS
            toff = [((t // 3) - 1) * S + (t % 3) - 1 for t in range(9)] if ks == 3 else [0]
            lane_q = np.arange(4)
            for ch in range(nch + 1):                                # the slack chunk included
                for t in toff:
                    o = q0 + lane_q + 4 * ch + t
                    assert o.min() >= 0 and o.max() < CS, (H, W, ks, ch, t)
            # dy fragments of the real chunks cover every pixel exactly once; what else they read is never staged to (zeros)
            read = q0 + np.arange(4 * nch)
            assert set(staged.tolist()) <= set(read.tolist())
            # a tap read at a position outside the picture sees a word no element is staged to
            if ks == 3:
                st = set(staged.tolist())
                for y in range(H):
                    for x in range(W):
                        for t in range(9):
                            yy, xx = y + t // 3 - 1, x + t % 3 - 1
                            w = base + y * S + x + toff[t]
                            assert (w in st) == (0 <= yy < H and 0 <= xx < W) and (w not in st or w == base + yy * S + xx)
    assert n_served > 2000


def test_the_direct_kernels_four_position_blocks_take_every_position_once():
    """conv_wgrad_k1_kernel: p0[m] = 16 m + 4 kq, p0[3] = HW - 16 + 4 kq, keep = (p0[3] + r >= 48)"""
    for HW in range(49, 65):
        count = np.zeros(HW, dtype=int)
        for kq in range(4):
            for m in range(4):
                p0 = 16 * m + 4 * kq if m < 3 else HW - 16 + 4 * kq
                for r in range(4):
                    assert 0 <= p0 + r < HW                         # whole loads inside the channel row
                    if m < 3 or p0 + r >= 48:
                        count[p0 + r] += 1
        assert (count == 1).all(), HW


# ---- the checker -------------------------------------------------------------------------------------------------------------------
def _buf(ref):
    b = G.guarded(ref.numel())
    b[G.GUARD:G.GUARD + ref.numel()] = ref.float().flatten()
    return b


def _wg(name):
    c = next(c for c in G.wg_cases() if c.name == name)
    d = G.wg_data(c)
    return c, d, G.wg_forward(c, d, torch.float64)


# (defect, the row it is planted in, does the suite's earlier max-norm bound pass it?)
WG_DEFECTS = [("dropped_sample", "red_300_slots_k3", False), ("sample_twice", "red_300_slots_k3", False),
              ("dropped_sample_small_channel", "red_300_slots_k3", True), ("tap_shifted", "t9_2x2_nobias_a", False),
              ("tap_shifted_small_channel", "t9_2x2_nobias_a", True), ("tile_transposed", "t9_2x2_nobias_a", False),
              ("lanes_reversed_small_row", "t9_2x2_nobias_a", True), ("db_over_cin", "t9_1x2_plain_b", False), ("past_dW", "t9_1x1_plain_a", None)]


@pytest.mark.parametrize("defect,name,old_passes", WG_DEFECTS)
def test_the_checker_reports_a_planted_weight_gradient_defect(defect, name, old_passes):
    c, d, r = _wg(name)
    assert G.check("dW", _buf(r.dW), r.dW, r.A_dW, "wg_dW") == [] and G.check("db", _buf(r.db), r.db, r.A_db, "wg_db") == []
    dW, db = r.dW.clone(), r.db.clone()
    small = slice(1, None, 16)                                       # the output channels whose dy is scaled by 2^-24
    if defect.startswith("dropped_sample") or defect == "sample_twice":
        s = list(range(c.B))
        s = s[:-1] if defect.startswith("dropped") else s + [7]
        bad = G.wg_forward(c, d, torch.float64, samples=s).dW
        if defect.endswith("small_channel"):
            dW[small] = bad[small]
        else:
            dW = bad
    elif defect.startswith("tap_shifted"):                           # tap (1, 1) reads the pixel one column to the right
        shifted = G.wg_forward(c, G.Case(d, x=d.x.roll(-1, 3)), torch.float64).dW[:, :, 1, 1]
        co = 1 if defect.endswith("small_channel") else 0
        dW[co, :, 1, 1] = shifted[co]
    elif defect.startswith("tile_transposed"):                       # the slot -> dW map with co and ci swapped inside the first tile
        dW[:16, :16] = r.dW[:16, :16].transpose(0, 1).clone()
    elif defect == "lanes_reversed_small_row":                       # ... a wrong lane -> ci map that only a small row shows
        dW[1, :16] = r.dW[1, :16].flip(0)
    elif defect == "db_over_cin":                                    # the bias tile count taken from the other operand: cin / 16 tiles of cout / 16
        db[c.cin:] = 0
    buf = _buf(dW)
    if defect == "past_dW":
        buf[G.GUARD + dW.numel()] = 0.0
        assert any("written behind dW" in f for f in G.check("dW", buf, r.dW, r.A_dW, "wg_dW"))
        return
    found = G.check("dW", buf, r.dW, r.A_dW, "wg_dW", maxnorm=False) + G.check("db", _buf(db), r.db, r.A_db, "wg_db", maxnorm=False)
    assert found and any("over" in f for f in found), found
    assert (G.maxnorm_ok(dW, r.dW, "wg_dW") and G.maxnorm_ok(db, r.db, "wg_db")) == old_passes


@pytest.mark.parametrize("defect,name", [("channel_left_out", "ln_C32_B9_P64"), ("gate_at_zero", "ln_C33_B5_P49")])
def test_the_checker_reports_a_planted_layernorm_defect(defect, name):
    """one channel left out of the mean; the ReLU gate taken as x >= 0 (what act(x) >= 0 gives) where x == 0 -- neither passes
    the earlier max-norm bound either"""
    c = next(c for c in G.ln_cases() if c.name == name)
    d = G.ln_data(c)
    r = G.ln_forward(c, d, torch.float64)
    bad = G.ln_forward(c, d, torch.float64, defect=defect)
    for k in ("dx", "dgamma", "dbeta"):
        assert G.check(k, _buf(r[k]), r[k], r["A_" + k], "ln_" + k) == []
    found = G.check("dx", _buf(bad.dx), r.dx, r.A_dx, "ln_dx", maxnorm=False)
    assert found and "over" in found[0], found
    assert not G.maxnorm_ok(bad.dx, r.dx, "ln_dx")


def test_the_fp32_statements_stay_inside_the_measured_constants():
    """the fp32 statements of every row (for the sums over the batch: torch's einsum / sum AND a strictly sequential accumulation
    over the samples): no element over K * U * A -- and K is the measured maximum, not a loose cap"""
    worst = {}

    def see(fam, name, got, ref, A, mode):
        v = G.ratio(got, ref, A)
        if v > worst.get(fam, (0.0,))[0]:
            worst[fam] = (v, name, mode)

    for c in G.wg_cases():
        if c.rc == 0:
            d = G.wg_data(c)
            r = G.wg_forward(c, d, torch.float64)
            for mode in ("einsum", "seq"):
                f = G.wg_forward(c, d, torch.float32, mode)
                see("wg_dW", c.name, f.dW, r.dW, r.A_dW, mode)
                see("wg_db", c.name, f.db, r.db, r.A_db, mode)
    for c in G.ln_cases():
        if c.rc == 0:
            d = G.ln_data(c)
            r = G.ln_forward(c, d, torch.float64)
            for mode in ("einsum", "seq"):
                f = G.ln_forward(c, d, torch.float32, mode)
                for k in ("dx", "dgamma", "dbeta"):
                    see("ln_" + k, c.name, f[k], r[k], r["A_" + k], mode)
    for c in G.gr_cases():
        d = G.gr_data(c)
        see("gr_dvg", c.name, G.gr_forward(c, d, torch.float32).dvg, *(lambda r: (r.dvg, r.A_dvg))(G.gr_forward(c, d, torch.float64)), "")
    for c in G.ctx_cases():
        d = G.ctx_data(c)
        r = G.ctx_forward(c, d, torch.float64)
        for mode in ("einsum", "seq"):
            see("ctx_dw", c.name, G.ctx_forward(c, d, torch.float32, mode).dw, r.dw, r.A_dw, mode)
    print("measured K per family:", {k: (round(v[0], 3), v[1], v[2]) for k, v in worst.items()})
    assert set(worst) == set(G.K)
    for fam, (v, name, mode) in worst.items():
        assert v <= G.K[fam], (fam, name, mode, v)
        assert v > 0.9 * G.K[fam], (fam, name, mode, v, "K is not the measured maximum rounded up in the second digit")
