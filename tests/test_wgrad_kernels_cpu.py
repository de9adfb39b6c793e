"""tests/wgrad_kernel_cases.py held to account without a GPU: the case tables reach every instantiation, tile class, reduction
depth and load path they claim (derived from launch rules restated there, which are held against the library's own
usf_wgrad_variant / usf_wgrad_plan / usf_wgrad_planes_plan); every poisoned region holds NaN; the census operands are exact in
three orders; the checkers pass the references and fail every mutant on a named check of a named case."""
import ctypes as C
import os
import re

import pytest
import torch

import wgrad_kernel_cases as wk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEMM = wk.F32_CASES + wk.PLANES_CASES + wk.PLAN_CASES


def _reached(cases):
    out = set()
    for c in cases:
        out |= wk.case_instantiations(c)
    return out


def _pick(pred, cases=GEMM):
    found = [c for c in cases if pred(c)]
    assert found, "no such case in the table"
    return found[0]


def _variant(c):
    return wk.case_plan(c).get("variant", -1)


F32 = [c for c in wk.F32_CASES if c.entry in ("f32", "bias")]
MODE0 = [c for c in F32 if c.mode == 0]
BF = [c for c in F32 if _variant(c) == 1]
LW = [c for c in F32 if _variant(c) == 2]
JOBS = [c for c in wk.F32_CASES if c.entry == "jobs"]
PLANES = [c for c in wk.PLANES_CASES if c.entry == "planes"]
BLOCKED = [c for c in wk.PLANES_CASES if c.entry == "blocked"]


# ---- coverage ------------------------------------------------------------------------------------------------------------------------
def test_mode0_table_reaches_both_paths_every_subtile_count_and_both_stores():
    got = _reached(MODE0)
    assert "f32-full" in got and "direct" in got and "partials" in got and "empty-range" in got
    edge = [tuple(map(int, re.findall(r"\d", x[x.index("<"):]))) for x in got if x.startswith("f32-edge")]
    assert {e[0] for e in edge} == {1, 2, 3, 4} == {e[1] for e in edge}
    assert {c.M for c in MODE0} >= set(wk.F32_M) and set(wk.F32_M) == {0, 1, 15, 16, 17, 31, 32, 33, 256, 257, 601}
    assert {c.N for c in MODE0} >= set(wk.F32_NK) <= {c.K for c in MODE0}
    assert {(c.alpha, c.beta) for c in MODE0} == set(wk.AB)
    # partials with ranges of different length
    assert any(len({e - b for b, e in wk.case_ranges(c)[0]}) > 1 for c in MODE0 if not wk.case_plan(c)["direct"])
    assert all(wk.case_plan(c)["direct"] == int(c.M <= 256) for c in MODE0)


def test_bf16x3_table_reaches_every_subtile_count_both_loads_and_both_colsum_forms():
    got = _reached(BF)
    pairs = [tuple(map(int, re.findall(r"\d", x[x.index("<"):]))) for x in got if x.startswith("bf<")]
    assert {a for a, _ in pairs} == {1, 2, 3, 4} == {b for _, b in pairs}
    assert {"bf-load-scalar", "bf-load-vector", "empty-range"} <= got
    assert {x for x in got if x.startswith("bf-cs")} == {f"bf-cs<{i}>" for i in (1, 2, 3, 4)}
    assert {c.cs for c in BF} == {True, False} and {c.M for c in BF} >= set(wk.BF_M) == {2048, 2049, 2079, 2081}
    # row ranges of 8 slabs, and a ragged last one
    assert any(all(e - b == 256 for b, e in wk.case_ranges(c)[0]) for c in BF)
    assert any((wk.case_ranges(c)[0][-1][1] - wk.case_ranges(c)[0][-1][0]) % 32 for c in BF)
    for kind in ("census", "table"):
        assert {c.cs for c in BF if c.kind == kind} == {True, False}


def test_loader_wave_table_reaches_all_twelve_instantiations_the_straddling_pair_and_the_slab_count_edges():
    want = {f"lw<{a},{b}>" for a in (1, 2, 4) for b in (1, 2, 4)} | {f"lw<{a},4,cs>" for a in (1, 2, 4)}
    assert {x for x in _reached(LW) if x.startswith("lw<")} == want
    assert {x for x in _reached([c for c in LW if c.kind != "table"]) if x.startswith("lw<")} == want, "an instantiation without a census"
    assert any("lw-straddle-NK" in wk.case_instantiations(c) for c in LW)
    for c in LW:          # an odd N / K: the 8-byte pair holding the last column of row M - 1 straddles the buffer bound
        ldy, lda, _ = wk.case_lds(c)
        assert ldy % 4 == 0 and lda % 4 == 0 and (c.M + 448) * max(ldy, lda) * 4 < 2 ** 32
    last = {}
    for c in LW:
        b, e = [r for r in wk.case_ranges(c)[0] if r[0] < r[1]][-1]
        if (e - b) % 32 == 1:
            last[wk.cdiv(e - b, 32) % 4] = c
    assert set(last) == {0, 1, 2, 3}, "the last range's slab count does not take every value mod 4 with a one-row slab"
    assert len(wk.lw_last_range_Ms(*wk.LW_SHAPES[4])) == 4 and wk.lw_last_range_Ms(*wk.LW_SHAPES[4])[1] == 8193
    # an EMPTY row range exists below 70 000 rows, and it is a case (both kinds); the 256-thread kernels have one too
    M = wk.find_empty_range(*wk.EMPTY_NK, 1, 8192, 70000)
    assert M is not None and {c.kind for c in LW if c.M == M and (c.N, c.K) == wk.EMPTY_NK} == {"census", "table"}
    assert all("empty-range" in wk.case_instantiations(c) for c in LW if c.M == M)
    assert wk.find_empty_range(*wk.EMPTY_SMALL_NK, 0, 1, 70000) == 65537 == wk.find_empty_range(*wk.EMPTY_SMALL_NK, 1, 2048, 70000)
    assert any(c.kn == (("wgrad_lw_min", 4096),) and c.M < 8192 for c in LW)
    assert {c.cs for c in LW} == {True, False}


def test_planes_table_reaches_all_nineteen_instantiations_every_class_and_both_schedules():
    want = ({f"wp<{a},{b}>" for a in (1, 2, 4, 5) for b in (1, 2, 4, 5)} - {"wp<5,5>"}) | {f"wp<{a},4,cs>" for a in (1, 2, 4, 5)}
    got = _reached(PLANES)
    assert {x for x in got if x.startswith("wp<")} == want and len(want) == 19
    assert {x for x in _reached([c for c in PLANES if c.kind != "table"]) if x.startswith("wp<")} == want, "an instantiation without a census"
    assert {x for x in got if x.startswith("class-")} == {"class-" + n for n in wk.CLASS_NAMES if n != "ww"}
    assert {"balanced", "plain"} <= got and "cs-without-instantiation" not in got
    assert {k for c in PLANES for k, _ in c.kn} == {"wgrad_sched", "wgrad_fold", "wgrad_rounds"}
    assert {c.off[0] for c in PLANES} == set(wk.OFFS) == {c.off[1] for c in PLANES} == {0, 8, 24}
    assert {c.M for c in PLANES} >= set(wk.PL_M) == {1, 31, 32, 33, 96, 97, 128, 129, 255, 288, 1001}
    assert {c.N for c in PLANES} | {c.K for c in PLANES} >= {8, 16, 17, 40, 64, 65, 128, 129, 144, 145, 272, 273}
    folded = {(wk.case_plan(c)["foldN"] and c.N % 128, wk.case_plan(c)["foldK"] and c.K % 128) for c in PLANES}
    assert {a for a, _ in folded} >= {1, 16} and {b for _, b in folded} >= {1, 8, 16}
    assert any(c.N % 128 == 17 and c.N > 128 for c in PLANES) and any(c.K % 128 == 17 and c.K > 128 for c in PLANES)
    # fN or fK = 0 and = 1 with column sums: the reduction's tk0 rule
    with_cs = [(c.N // 128, c.K // 128, wk.case_plan(c)["foldK"]) for c in PLANES if c.cs]
    assert {fk for _, fk, _ in with_cs} >= {0, 1, 2} and {fn for fn, _, _ in with_cs} >= {0, 1, 2}
    assert any(fk == 1 and fold for _, fk, fold in with_cs) and any(fk == 1 and not fold for _, fk, fold in with_cs)
    # slab counts 1 .. 9 per range, a last range one row long, balanced from four slabs
    slabs = {wk.cdiv(e - b, 32) for c in PLANES for b, e in wk.case_ranges(c)[0]}
    assert slabs >= set(range(1, 10))
    assert any(wk.case_ranges(c)[0][-1][1] - wk.case_ranges(c)[0][-1][0] == 1 for c in PLANES)
    assert all(wk.case_plan(c)["balanced"] == int(c.M >= 97) for c in PLANES if ("wgrad_sched", 0) not in c.kn)


def test_blocked_table_reaches_all_eleven_instantiations_and_the_jobs_launch_has_three_shapes():
    want = ({f"wpb<{a},{b}>" for a in (2, 4, 5) for b in (2, 4, 5)} - {"wpb<5,5>"}) | {f"wpb<{a},4,cs>" for a in (2, 4, 5)}
    assert {x for x in _reached(BLOCKED) if x.startswith("wpb<")} == want and len(want) == 11
    assert {x for x in _reached([c for c in BLOCKED if c.kind != "table"]) if x.startswith("wpb<")} == want
    assert any(c.off[0] > 0 for c in BLOCKED) and any(c.off[1] > 0 for c in BLOCKED)
    assert any(wk.case_plan(c)["foldN"] or wk.case_plan(c)["foldK"] for c in BLOCKED), "no wide tile"
    assert any(c.N % 128 < 32 and c.N % 32 for c in BLOCKED) and any(c.K % 128 < 32 and c.K % 32 for c in BLOCKED)
    assert all(wk.case_nkb(c)[0] > c.off[0] + wk.cdiv(c.N, 32) and wk.case_nkb(c)[1] > c.off[1] + wk.cdiv(c.K, 32) for c in BLOCKED)
    assert len({(c.M, c.N, c.K) for c in wk.PLAN_CASES}) == 3 == len(wk.PLAN_CASES)
    assert {c.kind for c in wk.PLAN_CASES} == {"table", "census"} and any(c.cs for c in wk.PLAN_CASES)


def test_jobs_colsum_and_split_tables_reach_what_they_claim():
    assert {c.M for c in JOBS} >= {1, 32, 33, 256} and all(c.M <= 256 for c in JOBS)
    assert any(x.startswith("f32-edge") for x in _reached(JOBS)) and "f32-full" in _reached(JOBS)
    col = [c for c in wk.COLSUM_CASES if c.entry == "colsum"]
    assert {wk.colsum_levels(c.M) for c in col} == {1, 2, 3}
    assert {c.M for c in col} >= {0, 1, 17, 256, 257, 65536, 65537} and {c.N for c in col} >= {1, 63, 64, 65}
    assert all(c.N <= 8 for c in col if c.M == 65537) and [wk.colsum_levels(m) for m in (256, 257, 65536, 65537)] == [1, 2, 2, 3]
    jc = [c for c in wk.COLSUM_CASES if c.entry == "jobcs"]
    assert {c.N for c in jc} >= {1, 63, 64, 65, 130} and any(c.M % 4 for c in jc) and any(c.beta == 0 for c in jc)
    sp = wk.SPLIT_CASES
    assert {c.path for c in sp} == {"vec", "ldx_odd", "misaligned", "sweep_vec", "sweep_scalar"}
    assert {wk.split_is_vector(c) for c in sp if c.path.startswith("sweep")} == {True, False}
    assert all(wk.split_is_vector(c) == (c.path in ("vec", "sweep_vec")) for c in sp)
    assert all(c.ldx % 2 for c in sp if c.path == "ldx_odd") and all(c.ldx % 4 == 0 for c in sp if c.path == "misaligned")
    assert {c.M for c in sp} >= {1, 31, 32, 33} and any(c.N % 8 for c in sp)


# ---- the restated rules against the library -------------------------------------------------------------------------------------------
def _lib():
    from usflows_amd import _ext
    if not _ext.lib_exists():
        import __graft_entry__
        __graft_entry__.build()
    return _ext.load()


def _plan_of_lib(lib, M, N, K, ldy, lda, mode, cs):
    out = (C.c_int64 * 8)()
    assert lib.usf_wgrad_plan(M, N, K, ldy, lda, mode, int(cs), out, 8) == 8, lib.usf_last_error()
    return dict(zip(("variant", "splits", "rows", "direct", "grid", "threads", "reduce", "need"), out))


def _planes_plan_of_lib(lib, M, N, K, ws, cs, cus):
    out = (C.c_int64 * 35)()
    assert lib.usf_wgrad_planes_plan(M, N, K, ws, int(cs), cus, out, 35) == 35, lib.usf_last_error()
    return dict(balanced=out[0], foldN=out[1], foldK=out[2], blocks=out[3], items=out[4], parts=out[6], T=list(out[7:16]),
                nseg=list(out[16:25]), rows=list(out[25:34])), out[5], out[34]


def test_restated_rules_match_the_library_on_every_case_and_on_a_sweep():
    lib = _lib()
    for c in GEMM:
        plan = wk.case_plan(c)
        with wk.knobs(c.kn):
            if c.entry in ("f32", "bias"):
                ldy, lda, _ = wk.case_lds(c)
                assert _plan_of_lib(lib, c.M, c.N, c.K, ldy, lda, c.mode, c.cs) == plan, wk.case_id(c)
                assert lib.usf_wgrad_variant(c.M, c.N, c.K, ldy, lda, c.mode) == plan["variant"]
                assert lib.usf_wgrad_workspace_floats(c.M, c.N, c.K) == wk.case_workspace_floats(c) >= plan["need"]
                assert lib.usf_wgrad_bias_ok(c.M, c.N, c.K, ldy, lda, c.mode) == int(plan["variant"] >= 1 and c.K >= 64)
            elif c.entry != "jobs":
                ws = wk.case_workspace_floats(c)
                got, need, assumed = _planes_plan_of_lib(lib, c.M, c.N, c.K, -1, c.cs, wk.CUS)
                assert got == {k: plan[k] for k in got}, wk.case_id(c)
                assert assumed == ws and need == plan["parts"] * c.N * (c.K + int(c.cs)) <= ws
    g = torch.Generator().manual_seed(5)
    for _ in range(400):
        M, N, K = (int(torch.randint(1, hi, (1,), generator=g)) for hi in (70000, 900, 900))
        mode, ld = int(torch.randint(0, 2, (1,), generator=g)), wk.ceil_to(max(N, K), 4)
        assert _plan_of_lib(lib, M, N, K, ld, ld, mode, False) == wk.f32_plan(M, N, K, ld, ld, mode, False), (M, N, K, mode)
        for cus in (256, 304, 64):
            ws = wk.planes_workspace_floats(M, N, K, cus)
            got, _, assumed = _planes_plan_of_lib(lib, M, N, K, -1, False, cus)
            want = wk.planes_plan(M, N, K, ws, cus)
            assert assumed == ws and got == {k: want[k] for k in got}, (M, N, K, cus)
    # a workspace too small for the balanced schedule: the plain grid
    got, _, _ = _planes_plan_of_lib(lib, 1001, 272, 144, wk.wp_plain_splits(1001, 272, 144) * 272 * 145, False, 256)
    assert got["balanced"] == 0 == wk.planes_plan(1001, 272, 144, wk.wp_plain_splits(1001, 272, 144) * 272 * 145)["balanced"]
    assert lib.usf_wgrad_plan(10, 10, 10, 12, 12, 0, 1, (C.c_int64 * 8)(), 8) < 0          # no column sums there


def test_headers_state_what_was_found():
    text = open(os.path.join(ROOT, "include", "usflows_hip_internal.h")).read()
    assert f"2^{wk.SPLIT_EXACT_EMIN} <= |x| < 2^{wk.SPLIT_EXACT_EMAX + 1}" in text
    for name in ("usf_wgrad_plan", "usf_wgrad_planes_plan"):
        assert re.search(name + r" \(an addition: USF_INTERNAL_VERSION is unchanged", text)


# ---- buffers --------------------------------------------------------------------------------------------------------------------------
def _all_nan16(bits):
    return bool(torch.isnan(bits.contiguous().view(torch.bfloat16).float()).all())


@pytest.mark.parametrize("c", GEMM, ids=wk.case_id)
def test_poison_sits_everywhere_the_contract_names_and_the_checker_passes_the_reference(c):
    p = wk.prepared(c)
    M, N, K = c.M, c.N, c.K
    ldy, lda, ldg = wk.case_lds(c)
    if c.entry in ("f32", "bias", "jobs"):
        for name, n, ld in (("Y", N, ldy), ("A", K, lda)):
            buf = p[name]
            body = buf[wk.GF:-wk.GF].view(M + wk.EXTRA_ROWS, ld)
            assert ld > n and ld % 4 == 0 and torch.isnan(body[:, n:]).all() and torch.isnan(body[M:]).all()
            assert torch.isnan(buf[:wk.GF]).all() and torch.isnan(buf[-wk.GF:]).all() and not torch.isnan(body[:M, :n]).any()
    elif c.entry == "planes":
        for name, n, ld, off, stride in (("Y", N, ldy, c.off[0], p["ystride"]), ("A", K, lda, c.off[1], p["astride"])):
            buf, R = p[name], wk.ceil_to(M, 32)
            assert ld % 8 == 0 and off % 8 == 0 and stride % 8 == 0 and stride >= R * ld and ld > off + n
            assert _all_nan16(buf[:wk.GH]) and _all_nan16(buf[-wk.GH:])
            for q in range(3):
                pl = buf[wk.GH + q * stride: wk.GH + q * stride + R * ld].view(R, ld)
                assert _all_nan16(pl[:M, :off]) and _all_nan16(pl[:M, off + n:]) and not (pl[M:] != 0).any()
                assert _all_nan16(buf[wk.GH + q * stride + R * ld: wk.GH + (q + 1) * stride])
                assert not torch.isnan(pl[:M, off: off + n].contiguous().view(torch.bfloat16).float()).any()
    else:
        for name, n, nkb, kb0, zero in (("Y", N, wk.case_nkb(c)[0], c.off[0], True), ("A", K, wk.case_nkb(c)[1], c.off[1], False)):
            buf = p[name]
            logical = wk.from_chunks(buf[wk.GH:-wk.GH], 3, wk.cdiv(M, 16), nkb)
            assert _all_nan16(logical[:, :, :32 * kb0]) and _all_nan16(logical[:, :, 32 * kb0 + n:][:, :M])
            assert _all_nan16(logical[:, :, 32 * (kb0 + wk.cdiv(n, 32)):])
            pad = logical[:, M:, 32 * kb0: 32 * (kb0 + wk.cdiv(n, 32))]
            vals = pad.contiguous().view(torch.bfloat16).float()
            assert (not (pad != 0).any()) if zero else (bool(torch.isfinite(vals).all()) and (M % 16 == 0 or bool((vals != 0).any())))
    G = wk.g_view(c, p["G0"], ldg)
    assert ldg > K and torch.isnan(G[N:]).all() and torch.isnan(G[:, K:]).all()
    assert bool(torch.isnan(G[:N, :K]).all()) if c.beta == 0 else not torch.isnan(G[:N, :K]).any()
    cs = p["cs0"][wk.GF:-wk.GF]
    assert torch.isnan(cs[N:]).all() and torch.isnan(p["cs0"][:wk.GF]).all() and torch.isnan(p["cs0"][-wk.GF:]).all()
    assert bool(torch.isnan(cs[:N]).all()) if not (c.cs and c.cs_ab[1] != 0) else not torch.isnan(cs[:N]).any()
    assert torch.isnan(p["ws0"]).all() and p["ws0"].numel() == wk.case_workspace_floats(c) + wk.GF
    # a NaN that moved is another NaN: the payloads differ from place to place
    assert wk.bits32(p["G0"][:wk.GF]).unique().numel() == wk.GF
    bad, fig = wk.check(c, wk.emulate(c, p), p)
    assert bad == [] and (c.kind == "table" or fig["census"] == "exact")
    if c.kind != "table" and c.mode == 1:
        exp = wk.bits32(p["census"].float())
        assert torch.equal(p["census"].float().double(), p["census"]), "the census sum is not an fp32 number"
        for got in wk.census_orders(c, p):
            assert torch.equal(wk.bits32(got), exp), "the census operands are not exact in every order"
        rows = wk.census_rows(c)
        assert (p["Yv"] != 0).sum(0).max() <= (4 if c.kind == "census4" else 7) and bool((p["Av"] != 0).all())
        if 7 * N >= len(wk.risk_rows(c)):
            assert set(rows.flatten().tolist()) >= set(wk.risk_rows(c)), "a risk row without a non-zero"
        pl = wk.split_planes(p["Av"], 3).float()
        assert bool((pl != 0).all()) and torch.equal(pl[0] + pl[1] + pl[2], p["Av"])


@pytest.mark.parametrize("c", wk.COLSUM_CASES, ids=wk.ccase_id)
def test_colsum_buffers_and_checker(c):
    p = wk.colsum_prepared(c)
    body = p["Y"][wk.GF:-wk.GF].view(c.M + wk.EXTRA_ROWS, p["ld"])
    assert torch.isnan(body[c.M:]).all() and torch.isnan(body[:, c.N:]).all() and torch.isnan(p["ws0"]).all()
    out = p["out0"][wk.GF:-wk.GF]
    assert torch.isnan(out[c.N:]).all() and bool(torch.isnan(out[:c.N]).all()) == (c.beta == 0)
    assert wk.colsum_check(c, wk.colsum_emulate(c, p), p)[0] == []
    if c.M > 0:
        for mutant, name in (("row_ge_M", "nan"), ("store_past_K", "guard")) + ((("beta_where_zero", "nan"),) if c.beta == 0 else ()) \
                + ((("last_row_of_range", "census"),) if c.kind == "census" else ()):
            bad = wk.colsum_check(c, wk.colsum_emulate(c, p, mutant), p)[0]
            assert any(b.startswith(name) for b in bad), (mutant, bad)


@pytest.mark.parametrize("c", wk.SPLIT_CASES, ids=wk.scase_id)
def test_split_buffers_and_the_exact_range(c):
    p = wk.split_prepared(c)
    assert wk.split_check(c, p["expected"], p) == [] and wk.split_check(c, p["P0"], p) != []
    assert _all_nan16(p["P0"]) and torch.isnan(p["X"][:p["x_off"]]).all()
    # a NaN of the split itself only where the first plane overflowed: |x| above bf16's largest value
    assert int(p["any_nan"].sum()) == (48 if c.path.startswith("sweep") else 0)
    body = p["X"][p["x_off"]: -wk.GF].view(c.M + wk.EXTRA_ROWS, c.ldx)
    assert torch.isnan(body[c.M:]).all() and torch.isnan(body[:, c.N:]).all()
    if c.path.startswith("sweep"):
        R, st = wk.ceil_to(c.M, 32), p["stride"]
        planes = torch.stack([p["expected"][wk.GH + q * st: wk.GH + q * st + R * c.ldp].view(R, c.ldp)[:c.M, :c.N] for q in range(3)])
        assert wk.split_exact_exponents(wk.split_exact_rows(planes, p["Xv"])) == (wk.SPLIT_EXACT_EMIN, wk.SPLIT_EXACT_EMAX)
        # the sweep holds every exponent, subnormals and both signs
        bits = wk.bits32(p["Xv"]).long() & 0xFFFFFFFF
        assert set(((bits >> 23) & 0xFF).flatten().tolist()) >= set(range(255)) and set((bits >> 31).flatten().tolist()) == {0, 1}


# ---- mutants --------------------------------------------------------------------------------------------------------------------------
def _is_lw_census(c):
    return c.entry == "f32" and c.kind == "census" and _variant(c) == 2 and c.M == 8193


MUTANT_CASES = {
    "drop_Y2A0": ("census", [_is_lw_census, lambda c: c.entry == "planes" and c.kind == "census", lambda c: c.entry == "blocked" and c.kind == "census",
                             lambda c: c.kind == "census" and _variant(c) == 1]),
    "drop_Y1A1": ("census", [_is_lw_census, lambda c: c.entry == "planes" and c.kind == "census"]),
    "drop_Y0A2": ("census", [_is_lw_census, lambda c: c.entry == "planes" and c.kind == "census"]),
    "dup_Y1A0": ("census", [_is_lw_census, lambda c: c.entry == "blocked" and c.kind == "census"]),
    "last_row_of_range": ("census", [_is_lw_census, lambda c: c.entry == "planes" and c.kind == "census" and c.M == 1001]),
    "second_range_first_slab_twice": ("census", [_is_lw_census, lambda c: c.entry == "planes" and c.kind == "census" and c.M == 1001]),
    "partial_left_out": ("census", [_is_lw_census, lambda c: c.entry == "f32" and c.kind == "census" and c.mode == 0 and c.M > 256]),
    "class_count_from_other_class": ("parity", [lambda c: c.entry == "planes" and c.kind == "table" and c.N == 273 and wk.case_plan(c)["parts"] > 1]),
    "dead_subtile_stored": ("guard", [lambda c: c.entry == "f32" and c.mode == 0 and c.N % 16 == 1 and c.M > 0]),
    "store_past_K": ("guard", [lambda c: c.entry == "f32" and c.mode == 0 and c.M > 0, lambda c: c.entry == "planes"]),
    "colsum_from_tile_column_1": ("nan", [lambda c: c.entry == "bias" and c.K <= 128, lambda c: c.entry == "planes" and c.cs and c.K <= 128]),
    "beta_where_zero": ("nan", [lambda c: c.entry == "f32" and c.beta == 0 and c.M > 0, lambda c: c.entry == "planes" and c.beta == 0]),
    "nan_from_padding_column": ("nan", [lambda c: c.entry == "f32" and _variant(c) == 2 and c.kind == "table"]),
    "extension_swapped": ("parity", [lambda c: c.entry == "planes" and c.kind == "table" and wk.case_plan(c)["foldK"]]),
    "blk_pos_identity": ("parity", [lambda c: c.entry == "blocked" and c.kind == "table" and c.K >= 32]),
    "row_ge_M": ("nan", [lambda c: c.entry == "f32" and c.mode == 0 and c.M > 0, lambda c: c.entry == "f32" and _variant(c) == 2]),
}


def test_every_mutant_has_its_cases():
    assert set(MUTANT_CASES) == set(wk.MUTANTS) and len(wk.MUTANTS) >= 14


@pytest.mark.parametrize("mutant", wk.MUTANTS)
def test_mutant_fails_its_named_check(mutant):
    name, preds = MUTANT_CASES[mutant]
    for pred in preds:
        c = _pick(pred)
        p = wk.prepared(c)
        bad, _ = wk.check(c, wk.emulate(c, p, mutant), p)
        assert any(b.startswith(name) for b in bad), f"{mutant} passes '{name}' on {wk.case_id(c)}: {bad}"


def test_a_norm_bound_cannot_see_a_lost_product_but_the_census_can():
    """gap 1 of the kernels' old tests, in numbers: with half the products gone a randn case stays far inside the old bound
    2e-6 sqrt(M) -- the census differs in most elements"""
    c = _pick(lambda c: c.entry == "f32" and c.kind == "table" and c.mode == 1 and c.M == 2081 and not c.cs)
    p = wk.prepared(c)
    half = wk.census_expected(c, p, wk.KEPT[3:])
    err = float((half - p["ref"]).abs().max() / p["ref"].abs().max())
    assert 1e-7 < err < 0.1 * 2e-6 * c.M ** 0.5
    cc = _pick(_is_lw_census)
    cp = wk.prepared(cc)
    for drop in wk.KEPT[:3]:
        d = wk.census_expected(cc, cp, [q for q in wk.KEPT if q != drop]).float() != cp["census"].float()
        assert float(d.double().mean()) > 0.8
