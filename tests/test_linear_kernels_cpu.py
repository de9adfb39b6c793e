"""tests/linear_kernel_cases.py held to account without a GPU: the table reaches every instantiation and edge its docstring
claims (the list of instantiations is written out here, not derived from a dispatcher), every case names the kernel the library
would launch (usf_linear_variant under the case's knobs, host-only), the checker accepts the fp32 torch-CPU evaluation of every
case and rejects each of ten planted defects in every kernel family.  The library calls here launch nothing and read no pointer;
without the built library they cannot run (as in tests/test_abi.py, the library is built first when it is missing)."""
import inspect

import pytest
import torch

import linear_kernel_cases as lk


@pytest.fixture(scope="module")
def ext():
    from usflows_amd import _ext
    if not _ext.lib_exists():
        import __graft_entry__
        __graft_entry__.build()
    _ext.load()
    return _ext


# every instantiation the table must reach, written out: (family, variant code, ...)
EXPECTED = (
    # small-batch kernel: (SK_G, mw, ks)
    {("skinny", 1000, 4, mw, ks) for mw in (1, 2) for ks in (1, 2, 3, 4)}
    | {("skinny", 1000, 8, 1, 4), ("skinny", 1000, 8, 2, 4), ("skinny", 1000, 4, 1, 8), ("skinny", 1000, 4, 1, 5)}
    # exact-f32 tiles: (PRO, EPI, vec_ok) -- 3 tiles x 2 prologues x 3 epilogues = 18 kernels, each on both store paths
    | {("f32", tile, pro, epi, vec) for tile in (2122, 2244, 2254) for pro in (0, 1) for epi in (0, 1, 2) for vec in (0, 1)}
    # bf16x3 tiles: (template, epilogue) -- 4 tiles x {plain, PRO, SIDE} = 12 kernels
    | {("bf16x3", tile, "plain", form) for tile in (3244, 3442, 3542, 3584)
       for form in ("bias_leaky", "residual", "addend_leaky", "gate", "post_mul")}
    | {("bf16x3", tile, "PRO", form) for tile in (3244, 3442, 3542, 3584) for form in ("bias_leaky", "post_mul")}
    | {("bf16x3", tile, "SIDE", form) for tile in (3244, 3442, 3542, 3584) for form in ("bias", "addend_leaky")}
)


def test_table_reaches_exactly_the_listed_instantiations():
    assert len(EXPECTED) == 12 + 36 + 36
    assert len(set(lk.CASES)) == len(lk.CASES) and len({lk.case_id(c) for c in lk.CASES}) == len(lk.CASES)
    assert {lk.instantiation(c) for c in lk.CASES} == EXPECTED
    assert 100 <= len(lk.CASES) <= 160


def test_every_case_names_the_kernel_the_library_would_launch(ext):
    lib = ext.load()
    for c in lk.CASES:
        assert lk.variant(c, lib, ext.LinearDesc) == lk.instantiation(c)[1], lk.case_id(c)
    # the knob matters: without it the small tiled cases are the small-batch kernel's, and it is put back after every query
    from usflows_amd.config import config
    assert config.get_lib("skinny_max", 768) == 768 and config.get_lib("skinny_g", 4) == 4 and config.get_lib("skinny_ks_small", 4) == 4
    c = next(c for c in lk.CASES if c.family == "f32" and c.M <= 768)
    assert lk.variant(c._replace(knobs=()), lib, ext.LinearDesc) == 1000
    # without its planes a bf16x3 case is the exact-f32 tile's; so is one whose residual rows are not 16-byte aligned
    c = next(c for c in lk.CASES if c.family == "bf16x3" and c.form == "residual")
    assert lk.variant(c._replace(family="f32"), lib, ext.LinearDesc) // 1000 == 2
    import ctypes
    with lk.knobs(c.knobs):
        d = lk.descriptor(c, lk.fake_ptr, ext.LinearDesc)
        d.ldr += 1
        assert lib.usf_linear_variant(ctypes.byref(d)) // 1000 == 2


def test_no_case_is_skipped_or_expected_to_fail():
    import test_linear_kernels_gpu as gpu_file
    src = inspect.getsource(gpu_file) + inspect.getsource(lk)
    assert "xfail" not in src and "skip" not in src
    params = [m for m in gpu_file.test_linear_kernel_vs_fp64.pytestmark if m.name == "parametrize"]
    assert len(params) == 1 and list(params[0].args[1]) == lk.CASES


def _fam(name, knobs=None):
    return [c for c in lk.CASES if c.family == name and (knobs is None or bool(c.knobs) == knobs)]


def test_small_batch_cases_hold_what_the_docstring_says():
    sk = _fam("skinny", False)
    assert all(c.M <= 768 for c in _fam("skinny"))
    shape = lk.skinny_shape
    assert {shape(c) for c in sk} == {(4, mw, ks) for mw in (1, 2) for ks in (1, 2, 3, 4)}
    assert {c.M for c in sk} == {1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 100, 768}
    assert {c.N for c in sk} == {1, 3, 4, 15, 16, 17, 20, 33, 161}
    assert {c.K for c in sk} == {4, 16, 20, 32, 36, 48, 52, 64, 260, 528, 784}
    for mw in (1, 2):
        at = [c for c in sk if shape(c)[1] == mw]
        assert {c.form for c in at} == {"bias_leaky", "residual", "addend_leaky", "gate", "post_mul"}, mw
        assert {lk.store_vec_ok(c) for c in at} == {0, 1} and {c.pro for c in at} == {"none", "div", "sub", "both"}, mw
        # 3 and 4 fetch groups of four 16-k steps in K-range wave 0, one fewer in the others (K = 528: 9 / 8 steps, 784: 13 / 12)
        assert {c.K for c in at} >= {528, 784}, mw
    for K, steps in [(528, (9, 8)), (784, (13, 12))]:
        nstep = -(-K // 16)
        assert tuple(-(-(nstep - wk) // 4) for wk in (0, 3)) == steps and -(-steps[0] // 4) == -(-steps[1] // 4) + 1
    # unequal step counts between the K-range waves, and a ragged last step (K % 16 != 0)
    assert any(-(-c.K // 16) % shape(c)[2] for c in sk) and {c.K % 16 for c in sk} >= {0, 4}
    tuned = _fam("skinny", True)
    assert sorted((c.knobs, shape(c)) for c in tuned) == [((("skinny_g", 8),), (8, 1, 4)), ((("skinny_g", 8),), (8, 2, 4)),
                                                          ((("skinny_ks_small", 8),), (4, 1, 5)), ((("skinny_ks_small", 8),), (4, 1, 8))]
    assert {c.K for c in tuned if shape(c) == (4, 1, 5)} == {80}
    # SK_G = 8: more than one fetch group of eight steps in wave 0
    assert all(-(-(-(-c.K // 16)) // 4) > 8 for c in tuned if shape(c)[0] == 8)


def test_exact_f32_tile_cases_hold_what_the_docstring_says():
    f32 = _fam("f32")
    assert all(c.knobs == (("skinny_max", 0),) for c in f32)
    tile = lambda c: lk.instantiation(c)[1]      # noqa: E731
    form = lambda c: lk.FORMS[c.form]      # noqa: E731
    assert {c.K for c in f32} == {4, 8, 12, 16, 20, 36, 52, 100}
    assert {c.pro for c in f32} == {"none", "div", "sub", "both"}
    for t in (2122, 2244, 2254):
        at = [c for c in f32 if tile(c) == t]
        assert {form(c).extra for c in at if lk.instantiation(c)[3] == 2} == {"addend", "gate"}, t
        assert {lk.store_vec_ok(c) for c in at if lk.instantiation(c)[3] == 0} == {0, 1}, t
        # bias_vec: N % 4 == 0 with a 16-byte aligned bias, and not
        assert {c.N % 4 == 0 and c.bias_al for c in at if form(c).bias} == {True, False}, t
        assert {c.pro for c in at} == {"none", "div", "sub", "both"}, t
    small = [c for c in f32 if tile(c) == 2122]
    assert {c.M for c in small} == {1, 31, 33, 64, 130, 800} and {c.N for c in small} == {1, 3, 4, 33, 63, 64}
    assert all(c.M <= 64 or c.N <= 64 for c in small)
    assert {c.N for c in f32 if tile(c) == 2244} == {68, 100, 128, 161, 250, 256}
    assert {c.N for c in f32 if tile(c) == 2254} == {129, 160, 300}
    for t in (2244, 2254):
        assert {c.M for c in f32 if tile(c) == t} == {65, 255, 256, 257, 520, 2100}, t
        assert -(-2100 // 256) == 9                  # nine row panels: the second round of the block map, and its early return
    # the residual form is the one with every later step at work (the order mutants need it)
    assert {(t, p) for t in (2122, 2244, 2254) for p in (0, 1)} == {(tile(c), lk.instantiation(c)[2]) for c in f32 if form(c).extra == "residual"}


def test_bf16x3_tile_cases_hold_what_the_docstring_says():
    b3 = _fam("bf16x3")
    assert all(c.knobs == (("skinny_max", 0),) and c.N % 4 == 0 and c.N > 64 and c.M > 64 and c.K % 8 == 0 and c.vec for c in b3)
    tile = lambda c: lk.instantiation(c)[1]      # noqa: E731
    width = {3244: 64, 3442: 128, 3542: 160, 3584: 160}
    for t in (3244, 3442, 3542, 3584):
        at = [c for c in b3 if tile(c) == t]
        assert len(at) == 9 and {c.K for c in at} == {8, 40, 64, 72, 104, 136}, t
        assert sorted(c.pro for c in at if c.pro != "none") == ["both", "sub"] and sum(c.side for c in at) == 2, t
        assert not any(c.side and c.pro != "none" for c in at)                     # A_planes_out takes no prologue
        assert any(c.N % width[t] for c in at), t                                  # a ragged last column block
        assert {c.bias_al for c in at} == {True, False}, t
    assert {c.M for c in b3 if tile(c) == 3244} == {65, 129, 257, 769, 1025}
    assert {(c.M, c.N) for c in b3 if tile(c) != 3244} == {(32641, 68), (32641, 124), (32641, 156), (32641, 132), (1921, 2692)}


def test_the_large_bf16x3_shapes_are_the_smallest_that_qualify(ext):
    """the dispatcher leaves tile 3244 at 256 tiles of 128 x 160: one row panel fewer and the case is 3244's again.  3442 / 3584
    (one column block of 160): 255 * 128 + 1 rows; 3542 below 2048 rows: 16 row panels x 17 column blocks -- with 16 column blocks
    (N <= 2560) no N pads less on 160 than on 128 columns, with 17 the first such N % 4 == 0 is 2692"""
    lib = ext.load()
    at = lambda M, N: lk.variant(lk.Case("bf16x3", M, N, 64, "bias", "none", True, True, False, lk.TILES_OFF), lib, ext.LinearDesc)      # noqa: E731
    for (M, N), code in [((32641, 68), 3442), ((32641, 124), 3442), ((32641, 156), 3584), ((32641, 132), 3584), ((1921, 2692), 3542)]:
        assert at(M, N) == code and at(M - 1, N) == 3244, (M, N)
    assert all(at(1921, N) in (3244, 3442) for N in range(68, 2692, 4))
    assert all(at(32641, N) == 3442 for N in range(68, 129, 4)) and all(at(32641, N) == 3584 for N in range(132, 161, 4))


def test_buffers_are_poisoned_as_the_docstring_says():
    c = next(c for c in lk.CASES if c.family == "bf16x3" and c.form == "residual" and c.M < 2000)
    p, L = lk.prepared(c), lk.layout(c)
    M, N, K = c.M, c.N, c.K
    assert L["lda"] > K and L["ldw"] > K and L["ldc"] > N and L["ldx"] > N and L["lda"] % 4 == 0 and L["ldw"] % 4 == 0
    for name, rows, cols in [("A", M, K), ("W", N, K), ("extra", M, N)]:
        finite = torch.isfinite(p[name])
        assert finite[:rows, :cols].all() and not finite[rows:].any() and not finite[:, cols:].any(), name
        assert p[name].shape[0] == rows + lk.EXTRA_ROWS
    b0 = L["b_off"]
    assert torch.isfinite(p["bias"][b0: b0 + N]).all() and torch.isnan(p["bias"][b0 + N:]).all() and torch.isnan(p["bias"][:b0]).all()
    assert torch.isfinite(p["post_mul"][:N]).all() and torch.isnan(p["post_mul"][N:]).all() and p["post_mul"].numel() > N
    assert torch.isnan(p["C0"]).all() and p["C0"].shape == (M + lk.EXTRA_ROWS, L["ldc"])
    bits = lk._bits(p["C0"]).reshape(-1)
    assert bits.unique().numel() == bits.numel()                                   # a payload of its own each
    # W_split as the header words it: planes that sum to W, zero in [K, ceil32(K)), NaN beyond and between the planes
    kp = lk.ceil_to(K, 32)
    ws = p["W_split"].float()
    assert p["W_split"].dtype == torch.bfloat16 and ws.shape == (3, N + 1, L["ldws"]) and L["ldws"] >= kp and L["ldws"] % 8 == 0
    assert torch.equal(ws[:, :N, :K].sum(0), p["W"][:N, :K]) and (ws[:, :N, K:kp] == 0).all()
    assert torch.isnan(ws[:, :N, kp:]).all() and torch.isnan(ws[:, N]).all()
    w = p["W"][:N, :K]
    p1 = w.to(torch.bfloat16)
    assert torch.equal(p["W_split"][0, :N, :K], p1) and torch.equal(p["W_split"][1, :N, :K], (w - p1.float()).to(torch.bfloat16))
    c = next(c for c in lk.CASES if c.pro == "both" and c.family == "f32")
    p = lk.prepared(c)
    for name in ("pre_div", "pre_sub"):
        assert torch.isfinite(p[name][: c.K]).all() and torch.isnan(p[name][c.K:]).all() and p[name].numel() > c.K
    # zeros of either sign in every gate
    c = next(c for c in lk.CASES if c.form == "gate" and c.M >= 31 and c.N >= 16)
    gate = lk.prepared(c)["extra"][: c.M, : c.N]
    assert (gate == 0).any() and (lk._bits(gate) == -2 ** 31).any() and (lk._bits(gate) == 0).any()


def test_checker_accepts_the_fp32_evaluation_of_every_case():
    for c in lk.CASES:
        C = lk.fp32_result(c)
        assert lk.check(C, c) == [], lk.case_id(c)
        m = lk.measure(C, c)
        assert m["err"] == m["err32"] <= m["bound"]


def _pick(family, pred):
    found = [c for c in lk.CASES if c.family == family and c.M < 2000 and pred(c)]
    assert found, family
    return found[0]


FAMILIES = ["skinny", "f32", "bf16x3"]


@pytest.mark.parametrize("family", FAMILIES)
def test_checker_rejects_each_planted_defect(family):
    """the six defects of the arithmetic on the fp64 result of a case that has the step in question, then the four of the
    stores on the fp32 result"""
    big = lambda c: c.M >= 17 and c.N >= 16 and c.K >= 20      # noqa: E731
    res = _pick(family, lambda c: c.form == "residual" and big(c))
    add = _pick(family, lambda c: c.form == "addend_leaky" and big(c))
    gate = _pick(family, lambda c: c.form == "gate" and big(c))
    for c, defect in [(res, "drop_last_kstep"), (add, "drop_last_kstep"), (res, "act_after_residual"), (res, "post_mul_before_residual"),
                      (add, "addend_after_act"), (gate, "gate_positive_at_zero"), (res, "ignore_res_sign")]:
        p = lk.prepared(c)
        assert lk.check(lk.with_result(c, p["ref64"]), c) == []
        bad = lk.check(lk.with_result(c, lk.forward(c, p, torch.float64, defect=defect)), c)
        assert len(bad) == 1 and "above the bound" in bad[0], (defect, bad)
    assert set(lk.DEFECTS) == {"drop_last_kstep", "act_after_residual", "post_mul_before_residual", "addend_after_act",
                               "gate_positive_at_zero", "ignore_res_sign"}
    for c in (res, gate):
        p = lk.prepared(c)
        clean = lk.fp32_result(c)
        M, N, ldc = c.M, c.N, clean.shape[1]
        # one element in the last row and last column off by 1e-4 of the largest value (at least 1: the scale of the bound)
        C = lk.with_result(c, p["ref64"])
        C[M - 1, N - 1] += 1e-4 * max(1.0, p["ref64"].abs().max().item())
        bad = lk.check(C, c)
        assert len(bad) == 1 and f"at row {M - 1}, column {N - 1}" in bad[0], bad
        # one write into C[:, N], one into row M
        for row, col in [(0, N), (M - 1, N), (M, 0), (M, N - 1)]:
            C = clean.clone()
            C[row, col] = clean[0, 0]
            bad = lk.check(C, c)
            assert len(bad) == 1 and f"1 elements outside C[:M, :N] changed, the first at row {row}, column {col}" in bad[0], bad
        # one payload NaN moved
        C = clean.clone()
        C[M + 1, ldc - 1] = clean[0, N]
        assert torch.isnan(C[M + 1, ldc - 1]) and (lk._bits(C) != lk._bits(clean)).sum() == 1
        bad = lk.check(C, c)
        assert len(bad) == 1 and f"the first at row {M + 1}, column {ldc - 1}" in bad[0], bad
        # an element of C[:M, :N] left as it was
        C = clean.clone()
        C[M // 2, N // 2] = p["C0"][M // 2, N // 2]
        assert any("NaN in 1 elements" in b for b in lk.check(C, c))
