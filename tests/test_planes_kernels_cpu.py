"""tests/planes_kernel_cases.py held to account without a GPU: both tables reach every instantiation and every edge their
docstrings and the lists below claim (the instantiations are written out here, not derived from a dispatcher), every case names
the kernel the library would launch (usf_gemm_planes_variant / usf_coupling_planes_variant, host-only), every poisoned region
really holds NaN, the checkers accept the fp64 and the fp32 CPU evaluation of every case and reject each planted defect, and the
census operands meet the condition under which every kept product and partial sum is exact in fp32.  The library calls here
launch nothing and read no pointer; without the built library they cannot run (as in tests/test_abi.py, it is built first)."""
import ctypes
import inspect
import math

import pytest
import torch

import planes_kernel_cases as pk


@pytest.fixture(scope="module")
def ext():
    from usflows_amd import _ext
    if not _ext.lib_exists():
        import __graft_entry__
        __graft_entry__.build()
    _ext.load()
    return _ext


G, CP = pk.GEMM_CASES, pk.COUPLING_CASES
GROUPS = [(npl, tn) for npl in (3, 2) for tn in (4, 5)]


def _grp(npl, tn, kind="table"):
    return [c for c in G if (c.npl, c.tn) == (npl, tn) and (kind is None or c.kind == kind)]


# ---- GEMM table ---------------------------------------------------------------------------------------------------------------------
def test_gemm_table_reaches_every_instantiation():
    """(NPL, TN, form, DEAD): 12 kernels, each in its full and its DEAD tile form"""
    expected = {(npl, tn, form, dead) for npl in (2, 3) for tn in (4, 5) for form in ("planes", "fp32", "side") for dead in (0, 1)}
    assert len(expected) == 24
    assert {pk.gemm_instantiation(c) for c in G} == expected
    assert len(set(G)) == len(G) and len({pk.gemm_case_id(c) for c in G}) == len(G)
    assert 90 <= len(G) <= 120
    for c in G:
        assert pk.gemm_tn(pk.gemm_nblk(c)) == c.tn, pk.gemm_case_id(c)
        # DEAD runs only where the table means it to: kind "dead"
        assert pk.gemm_instantiation(c)[3] == int(c.kind == "dead"), pk.gemm_case_id(c)
        assert c.w_rows % 4 == 0 and c.w_rows >= pk.gemm_cols(c)


def test_gemm_dead_cases_meet_both_conditions():
    for c in G:
        if c.kind in ("dead", "scan"):
            end = pk.gemm_grid(c)[1] * 32 * c.tn
            assert end <= c.w_rows, pk.gemm_case_id(c)                      # the last column block lies wholly inside w_rows
    for npl, tn in GROUPS:
        dead = _grp(npl, tn, "dead")
        assert {c.form for c in dead} == {"planes", "fp32", "side"}
        # the issue's examples: c_kbn = TN with 32 TN - 16 live features; N = 32 TN - 10 with w_rows = 32 TN
        assert any(c.form == "planes" and c.n_out == tn for c in dead)
        assert any(c.form == "fp32" and (c.n_out, c.w_rows) == (32 * tn - 10, 32 * tn) for c in dead)
        for c in dead:
            end = pk.gemm_grid(c)[1] * 32 * tn
            assert (pk.bits16(pk.gemm_prepared(c)["W_planes"][:, end - 16: end]) == 0).all()


@pytest.mark.parametrize("npl,tn", GROUPS)
def test_gemm_table_holds_every_listed_edge(npl, tn):
    at = _grp(npl, tn)
    assert {c.nk for c in at} == {1, 2, 3, 4, 5, 6, 7}
    assert {c.M for c in at} == {1, 15, 16, 17, 33, 255, 256, 257, 2049}
    assert any(c.a_kb0 > 0 and c.a_nkb > c.a_kb0 + c.nk for c in at) and any(c.a_kb0 == 0 for c in at)
    # 257 rows: a second 256-row panel group; 2049: nine groups -- the map's second seq round and its pg >= nbm skip
    assert any(pk.gemm_grid(c)[0] == 2 for c in at) and any(pk.gemm_grid(c)[0] == 9 and pk.gemm_grid(c)[2] == 16 * pk.gemm_grid(c)[1] for c in at)
    pl = [c for c in at if c.form != "fp32"]
    f32 = [c for c in at if c.form == "fp32"]
    assert any(c.n_out % tn for c in pl) and any(c.n_out % tn == 0 for c in pl)          # ragged and full last column block
    assert any(c.n_out % 4 for c in f32) and any(c.n_out % 32 and c.n_out % 4 == 0 for c in f32)
    assert any(c.w_rows == pk.ceil_to(c.n_out, 4) != pk.ceil_to(c.n_out, 32) for c in f32)
    assert {c.bias for c in at} == {True, False}
    assert {(c.act, c.slope) for c in at} == {(pk.ACT_NONE, 0.0), (pk.ACT_LEAKY_RELU, 0.01), (pk.ACT_LEAKY_RELU, 0.0)}
    assert {(c.res, c.sign) for c in at if c.res} == {("alias", 1.0), ("alias", -1.0), ("sep", 1.0), ("sep", -1.0)}
    assert any(c.post_mul for c in f32) and any(not c.post_mul for c in f32)
    assert {c.vec for c in f32 if c.store} == {0, 1, 2}
    for c in f32:
        p = pk.gemm_prepared(c)
        assert (p["ldc"] % 4 == 0 and p["c_off"] == 0) == (c.vec == 2) and p["ldc"] >= c.n_out
    assert {(c.base, c.store) for c in f32 if c.base} == {(b, s) for b in ("laplace", "normal") for s in (True, False)}
    assert any(c.base and c.n_out % 4 for c in f32)
    side = [c for c in at if c.form == "side"]
    kinds = set()
    for c in side:
        s0, sn, b0, bn = c.side
        assert 0 <= s0 and sn > 0 and s0 + sn <= c.n_out and (bn == 0 or (s0 <= b0 and b0 + bn <= s0 + sn))
        kinds.add(("all" if (s0, sn) == (0, c.n_out) else "prefix" if s0 == 0 else "interior" if s0 + sn < c.n_out else "suffix",
                   "empty" if bn == 0 else "full" if bn == sn else "partial"))
    assert {k[0] for k in kinds} >= {"all", "prefix", "interior"} and {k[1] for k in kinds} == {"empty", "partial", "full"}
    # the dead-tile scan: three images whose dead rows are not quite dead, and a -0
    scan = _grp(npl, tn, "scan")
    assert sorted(c.dead for c in scan) == ["first", "last", "lastplane", "negzero"]
    for c in scan:
        p, end, K = pk.gemm_prepared(c), pk.gemm_grid(c)[1] * 32 * tn, 32 * c.nk
        rows = pk.bits16(p["W_planes"][:, end - 16: end])
        nz = rows.nonzero()
        assert len(nz) >= 1 and pk.gemm_instantiation(c)[3] == 0
        if c.dead == "first":
            assert {(int(r), int(k)) for _, r, k in nz} == {(0, 0)} and len(nz) == npl
        if c.dead == "last":
            assert {(int(r), int(k)) for _, r, k in nz} == {(15, K - 1)} and len(nz) == npl
        if c.dead == "lastplane":
            assert [tuple(map(int, t)) for t in nz] == [(npl - 1, 15, K - 1)]
            assert (pk.bits16(p["A_planes"][1:]) == 0).all()          # A is exactly representable in plane 0
        if c.dead == "negzero":
            assert (rows[nz[:, 0], nz[:, 1], nz[:, 2]] == -32768).all() and (p["W_eff"][end - 16: end] == 0).all()
    assert len(_grp(npl, tn, "census")) == 1


def test_gemm_persistent_cases_take_a_second_tile():
    per = [c for c in G if c.kind == "persist"]
    assert sorted((c.tn, c.n_out) for c in per) == [(4, 28), (5, 35)]
    for c in per:
        assert (c.nk, c.M) == (1, 8193) and pk.gemm_grid(c) == (33, 7, 280)
        assert pk.gemm_grid(c)[2] > 256                                      # (the GPU test asserts it against the device's CU count)
        assert pk.gemm_prepared(c)["C0"].numel() * 2 < 48 * 2 ** 20


def test_every_gemm_case_names_the_kernel_the_library_would_launch(ext):
    lib = ext.load()
    for c in G:
        d, side = pk.gemm_descriptor(c, pk.fake_ptr, ext.GemmPlanesDesc)
        assert lib.usf_gemm_planes_variant(ctypes.byref(d)) == pk.gemm_variant_code(c) == 5000 + 10 * c.tn + int(c.form == "fp32")
        assert (side is not None) == (c.form == "side")


# ---- coupling table -------------------------------------------------------------------------------------------------------------------
COUPLING_CODES = (
    {70000 + 1000 * npl + 100 * nh + 2 * ctx + side for npl in (2, 3) for nh in (1, 2, 3) for ctx, side in ((0, 0), (1, 0), (0, 1))}
    | {73000 + 100 * nh + 10 + 2 * ctx for nh in (1, 2) for ctx in (0, 1)}          # MODE 1, MODE 1 + CTX
    | {73000 + 100 * nh + 20 for nh in (1, 2)})                                        # MODE 2


def test_coupling_table_reaches_all_24_instantiations():
    assert len(COUPLING_CODES) == 24
    assert {pk.coupling_variant_code(c) for c in CP} == COUPLING_CODES
    assert len(set(CP)) == len(CP) and len({pk.coupling_case_id(c) for c in CP}) == len(CP) == 72
    for code in COUPLING_CODES:
        assert sum(pk.coupling_variant_code(c) == code for c in CP) == pk.C_PER_INSTANCE


def test_coupling_table_holds_every_listed_edge():
    assert {c.nk_p for c in CP} == {1, 2, 3, 5} and {c.nk_t for c in CP} == {1, 2, 3}
    assert {c.M for c in CP} == {1, 15, 16, 17, 127, 128, 129, 250, 1025}
    assert {w for c in CP for w in c.hidden} == {256, 200, 17, 1}
    assert {c.sign for c in CP} == {1.0, -1.0}
    acts = {(c.act, c.slope, math.copysign(1.0, c.slope)) for c in CP if c.mode != "gate"}
    assert acts == {(1, 0.01, 1.0), (1, 0.0, 1.0), (1, 1.0, 1.0), (1, 1.5, 1.0), (1, -0.5, -1.0), (1, 0.0, -1.0), (0, 0.0, 1.0)}
    # the max form (0 <= slope <= 1, not -0) and the select form both run
    assert {c.act == 1 and 0.0 <= c.slope <= 1.0 and math.copysign(1.0, c.slope) > 0 for c in CP if c.act == 1} == {True, False}
    assert {c.ctx_stride for c in CP if "ctx" in c.mode} == {0, 1}
    assert {c.geo for c in CP} == {"front", "behind", "shared"}
    for c in CP:
        geo = pk.coupling_geometry(c)
        used = max(geo["kb_p0"] + c.nk_p, geo["kb_t0"] + c.nk_t)
        assert geo["z_nkb"] > used                                              # z_nkb larger than what is used
        pr, tr = set(range(geo["kb_p0"], geo["kb_p0"] + c.nk_p)), set(range(geo["kb_t0"], geo["kb_t0"] + c.nk_t))
        if c.geo == "front":
            assert max(pr) + 1 < min(tr) and not pr & tr                       # a (poisoned) gap block between the ranges
        if c.geo == "behind":
            assert max(tr) < min(pr)
        if c.geo == "shared":
            assert len(pr & tr) == 1
        assert int(geo["p_cols"].sum()) + int(geo["t_cols"].sum()) == 32 * len(pr | tr) and not (geo["p_cols"] & geo["t_cols"]).any()
    gate = [c for c in CP if c.mode == "gate"]
    assert all(c.act == pk.ACT_GATE and c.npl == 3 and c.nh <= 2 for c in gate)


def test_every_coupling_case_names_the_kernel_the_library_would_launch(ext):
    lib = ext.load()
    for c in CP:
        d, entry, extra = pk.coupling_descriptor(c, pk.fake_ptr, ext.CouplingPlanesDesc)
        code = lib.usf_coupling_planes_variant(ctypes.byref(d), int("ctx" in c.mode), int(c.mode == "side"))
        assert code == pk.coupling_variant_code(c), (pk.coupling_case_id(c), code, lib.usf_last_error())
        assert entry == {"plain": "usf_coupling_planes", "hout": "usf_coupling_planes", "gate": "usf_coupling_planes", "ctx": "usf_coupling_planes_ctx",
                         "hout_ctx": "usf_coupling_planes_ctx", "side": "usf_coupling_planes_side"}[c.mode]
    # the code follows the launch branches: a rejected descriptor reports the launch's error, an empty one 0
    c = next(c for c in CP if c.mode == "gate")
    d, _, _ = pk.coupling_descriptor(c, pk.fake_ptr, ext.CouplingPlanesDesc)
    assert lib.usf_coupling_planes_variant(ctypes.byref(d), 1, 0) == -2 and b"USF_ACT_GATE" in lib.usf_last_error()
    d.M = 0
    assert lib.usf_coupling_planes_variant(ctypes.byref(d), 0, 0) == 0
    assert lib.usf_coupling_planes_variant(None, 0, 0) == -1


def test_no_case_is_skipped_or_expected_to_fail():
    import test_planes_kernels_gpu as gpu_file
    src = inspect.getsource(gpu_file) + inspect.getsource(pk)
    assert "xfail" not in src and "skip(" not in src and "skipif" not in src
    for fn, cases in ((gpu_file.test_gemm_planes_kernel_vs_fp64, G), (gpu_file.test_coupling_planes_kernel_vs_fp64, CP)):
        params = [m for m in fn.pytestmark if m.name == "parametrize"]
        assert len(params) == 1 and list(params[0].args[1]) == cases


# ---- poison ---------------------------------------------------------------------------------------------------------------------------
def _all_nan16(bits, npl):
    return bool(torch.isnan(bits.contiguous().view(pk.plane_dtype(npl)).float()).all())


def _image_poison(flat, npl, rows, K, ld, stride):
    """everything of a weight image but [rows, K] of each plane is NaN"""
    keep = torch.zeros(npl * stride, dtype=torch.bool)
    for q in range(npl):
        keep[q * stride: q * stride + rows * ld].view(rows, ld)[:, :K] = True
    assert stride > rows * ld and ld > K
    return _all_nan16(flat[~keep], npl) and not torch.isnan(flat[keep].view(pk.plane_dtype(npl)).float()).any()


def test_every_poisoned_region_of_the_gemm_cases_holds_nan():
    for c in G:
        if c.kind == "persist":
            continue
        p = pk.gemm_prepared(c)
        npl, M, R = c.npl, c.M, pk.ceil_to(c.M, 16)
        g = pk.GUARD // 2
        assert _all_nan16(p["A"][:g], npl) and _all_nan16(p["A"][-g:], npl)
        A = pk.from_chunks(pk.unguarded(p["A"]), npl, R // 16, c.a_nkb)
        inside = torch.zeros(32 * c.a_nkb, dtype=torch.bool)
        inside[32 * c.a_kb0: 32 * (c.a_kb0 + c.nk)] = True
        assert _all_nan16(A[:, :, ~inside], npl) or c.a_nkb == c.nk
        assert R == M or _all_nan16(A[:, M:], npl)                               # rows >= M of the last panel
        assert not torch.isnan(A[:, :M, inside].contiguous().view(pk.plane_dtype(npl)).float()).any()
        assert _image_poison(p["W"], npl, c.w_rows, 32 * c.nk, p["ldw"], p["w_plane_stride"]), pk.gemm_case_id(c)
        for name in ("bias", "post_mul"):
            if name in p:
                assert torch.isnan(p[name][c.w_rows:]).all() and p[name].numel() > c.w_rows and not torch.isnan(p[name][: c.w_rows]).any()
        if c.form == "fp32":
            assert torch.isnan(p["C0"]).all() and p["C0"].numel() >= (M + pk.EXTRA_ROWS) * p["ldc"]
            if c.base:
                assert torch.isnan(p["part0"]).all() and torch.isnan(p["base_tab"][3 * p["tab_stride"]:]).all()
        else:
            C = p["C0_bits"]
            out = torch.ones(32 * c.c_nkb, dtype=torch.bool)
            out[32 * c.c_kb0: 32 * c.c_kb0 + pk.gemm_cols(c)] = False
            assert out.any() and _all_nan16(C[:, :, out], npl) and (R == M or _all_nan16(C[:, M:], npl))
            assert c.res == "alias" or _all_nan16(C, npl)
            if c.res == "sep":
                Rb = pk.from_chunks(pk.unguarded(p["Rbuf"]), npl, R // 16, c.c_nkb)
                assert _all_nan16(Rb[:, :, out], npl) and (R == M or _all_nan16(Rb[:, M:], npl))
            if c.form == "side":
                assert torch.isnan(p["S0"]).all()


def test_every_poisoned_region_of_the_coupling_cases_holds_nan():
    for c in CP:
        p, geo = pk.coupling_prepared(c), pk.coupling_geometry(c)
        npl, M, R = c.npl, c.M, pk.ceil_to(c.M, 16)
        z = p["z0_bits"]
        used = torch.zeros(32 * geo["z_nkb"], dtype=torch.bool)
        used[32 * geo["kb_p0"]: 32 * (geo["kb_p0"] + c.nk_p)] = True
        used[32 * geo["kb_t0"]: 32 * (geo["kb_t0"] + c.nk_t)] = True
        assert (~used).sum() >= 64 and _all_nan16(z[:, :, ~used], npl) and (R == M or _all_nan16(z[:, M:], npl))
        lds = [p["ld"][0]] + [p["ld"][1]] * (c.nh - 1) + [p["ld"][2]]
        strides = [p["stride"][0]] + [p["stride"][1]] * (c.nh - 1) + [p["stride"][2]]
        for l in range(c.nh + 1):
            rows, K = (256 if l < c.nh else 32 * c.nk_t), (32 * c.nk_p if l == 0 else 256)
            assert _image_poison(p["W"][l], npl, rows, K, lds[l], strides[l]), (pk.coupling_case_id(c), l)
            assert torch.isnan(p["b"][l][rows:]).all() and p["b"][l].numel() > rows
            # zeros where the header demands them: hidden padding, the other set's features of the shared block
            w_out = c.hidden[l] if l < c.nh else None
            if w_out is not None:
                assert (p["W_eff"][l][w_out:] == 0).all() and (p["b"][l][w_out:256] == 0).all()
            if l > 0:
                assert (p["W_eff"][l][:, c.hidden[l - 1]:] == 0).all()
        if c.mode == "side":
            assert torch.isnan(p["S"][: pk.GUARD // 4]).all() and torch.isnan(p["S"][-(pk.GUARD // 4):]).all()
            t_only = torch.zeros_like(used)
            t_only[32 * geo["kb_t0"]: 32 * (geo["kb_t0"] + c.nk_t)] = True
            t_only[32 * geo["kb_p0"]: 32 * (geo["kb_p0"] + c.nk_p)] = False
            assert _all_nan16(p["z0_side_bits"][:, :, t_only], npl)
        if c.mode == "gate":
            for l in range(c.nh):
                gb = pk.from_chunks(pk.unguarded(p["gate"][l]), 3, R // 16, 8)
                assert _all_nan16(gb[1:], 3) and (R == M or _all_nan16(gb[0, M:], 3))        # planes 1 and 2: never read
        if "ctx" in c.mode:
            n = M if c.ctx_stride == 1 else 1
            assert torch.isnan(p["ctx"][n:]).all() and p["ctx"].numel() == n + pk.EXTRA_ROWS


# ---- the checkers: references pass, mutants fail ----------------------------------------------------------------------------------------
def test_gemm_references_pass_the_checker():
    for c in G:
        p = pk.gemm_prepared(c)
        for name in ("ref64", "ref32"):
            bad, fig = pk.gemm_check(c, pk.gemm_as_launch(c, p[name]))
            assert bad == [] and fig["err"] <= fig["bound"], (pk.gemm_case_id(c), name, bad)


def test_coupling_references_pass_the_checker():
    for c in CP:
        p = pk.coupling_prepared(c)
        for name in ("ref64", "ref32"):
            bad, fig = pk.coupling_check(c, pk.coupling_as_launch(c, p[name]))
            assert bad == [] and fig["err"] <= fig["bound"], (pk.coupling_case_id(c), name, bad)


def _gemm_mutants(c):
    """{name: buffers after a wrong launch} for a case; every one must fail gemm_check"""
    p = pk.gemm_prepared(c)
    ref = p["ref64"]
    out = {}

    def shifted(**kw):
        return {k: (v.clone() if v is not None else None) for k, v in ref.items()}

    if c.M >= 2:
        m = shifted()
        m["C"][c.M - 2] = ref["C"][c.M - 1]
        if m["part"] is not None:
            m["part"][c.M - 2] = ref["part"][c.M - 1]
        out["row_from_neighbour"] = pk.gemm_as_launch(c, m)
    m = shifted()
    m["C"][c.M - 1, 0] = float("nan")
    if m["part"] is not None:
        m["part"][c.M - 1, 0] = float("nan")
    out["padding_nan_in_last_row"] = pk.gemm_as_launch(c, m)
    if c.bias:
        out["bias_shifted"] = pk.gemm_as_launch(c, pk.gemm_forward(c, p, torch.float64, "bias_shifted"))
    if c.res:
        out["res_sign"] = pk.gemm_as_launch(c, pk.gemm_forward(c, p, torch.float64, "res_sign"))
    if c.kind == "scan" and c.dead != "negzero":
        out["no_dead_rows"] = pk.gemm_as_launch(c, pk.gemm_forward(c, p, torch.float64, "no_dead_rows"))
    if c.kind == "census":
        out["drop_product"] = pk.gemm_as_launch(c, pk.gemm_forward(c, p, torch.float64, "drop_product"))
        out["add_product"] = pk.gemm_as_launch(c, pk.gemm_forward(c, p, torch.float64, "add_product"))
    # one slack chunk / element written
    good = pk.gemm_as_launch(c, ref)
    if c.form == "fp32":
        good["C"][-1] = 1.0
    else:
        R = pk.ceil_to(c.M, 16)
        bits = pk.from_chunks(pk.unguarded(good["C"]), c.npl, R // 16, c.c_nkb).clone()
        kb = c.c_kb0 + c.n_out if c.c_kb0 + c.n_out < c.c_nkb else 0          # a block outside the written range
        bits[:, :16, 32 * kb: 32 * kb + 32] = 0
        good["C"] = pk.guarded(pk.to_chunks(bits), c.npl, 12)
    out["slack_chunk_written"] = good
    return out


def test_gemm_checker_rejects_every_mutant():
    seen = set()
    picked = [c for c in G if c.kind != "persist" and (c.idx % 3 == 0 or c.kind != "table")]
    for c in picked:
        for name, got in _gemm_mutants(c).items():
            bad, _ = pk.gemm_check(c, got)
            assert bad, (pk.gemm_case_id(c), name)
            seen.add((name, c.form))
    assert {n for n, _ in seen} == {"row_from_neighbour", "padding_nan_in_last_row", "bias_shifted", "res_sign", "no_dead_rows", "drop_product",
                                    "add_product", "slack_chunk_written"}
    assert {f for n, f in seen if n == "slack_chunk_written"} == {"planes", "fp32", "side"}
    # the `lastplane` scan image: its one product is held to bit equality
    for c in (c for c in G if c.dead == "lastplane"):
        p = pk.gemm_prepared(c)
        got = pk.gemm_as_launch(c, pk.gemm_forward(c, p, torch.float64, "no_dead_rows"))
        bad, fig = pk.gemm_check(c, got)
        assert any("exact columns" in b for b in bad)


def test_coupling_checker_rejects_every_mutant():
    names = set()
    for c in CP[::2]:
        p = pk.coupling_prepared(c)
        ref = p["ref64"]
        geo = pk.coupling_geometry(c)
        tc = geo["t_cols"][32 * geo["kb_t0"]: 32 * (geo["kb_t0"] + c.nk_t)]
        first = int(tc.nonzero()[0])
        muts = {}
        if c.M >= 2:
            m = dict(t=ref["t"].clone(), hidden=ref["hidden"])
            m["t"][c.M - 2] = ref["t"][c.M - 1]
            muts["row_from_neighbour"] = pk.coupling_as_launch(c, m)
        m = dict(t=ref["t"].clone(), hidden=ref["hidden"])
        m["t"][c.M - 1, first] = float("nan")
        muts["padding_nan_in_last_row"] = pk.coupling_as_launch(c, m)
        muts["res_sign"] = pk.coupling_as_launch(c, pk.coupling_forward(c, p, torch.float64, "res_sign"))
        if c.mode != "gate" and c.hidden[0] > 16:
            muts["bias_shifted"] = pk.coupling_as_launch(c, pk.coupling_forward(c, p, torch.float64, "bias_shifted"))
        good = pk.coupling_as_launch(c, ref)
        R = pk.ceil_to(c.M, 16)
        bits = pk.from_chunks(pk.unguarded(good["z"]), c.npl, R // 16, geo["z_nkb"]).clone()
        bits[:, :16, -32:] = 0                                                   # the last, unused block of z
        good["z"] = pk.guarded(pk.to_chunks(bits), c.npl, 21)
        muts["slack_chunk_written"] = good
        if c.M % 16 and "ctx" not in c.mode:
            leak = pk.coupling_as_launch(c, ref, pad_rows=1.0)                    # finite values in the rows >= M
            muts["finite_padding_rows"] = leak
        if c.M % 16 and "ctx" in c.mode:
            leak = pk.coupling_as_launch(c._replace(mode="plain" if c.mode == "ctx" else "hout"), ref, p=p)
            muts["ctx_wrote_padding_rows"] = leak
        if c.mode in ("hout", "hout_ctx", "gate"):
            m = dict(t=ref["t"], hidden=[h.clone() for h in ref["hidden"]])
            m["hidden"][-1][0, 0] += 1e-3 * (1 + m["hidden"][-1].abs().max())
            muts["hidden_out_off"] = pk.coupling_as_launch(c, m)
        for name, got in muts.items():
            bad, _ = pk.coupling_check(c, got)
            assert bad, (pk.coupling_case_id(c), name)
            names.add(name)
    assert names == {"row_from_neighbour", "padding_nan_in_last_row", "res_sign", "bias_shifted", "slack_chunk_written", "finite_padding_rows",
                     "ctx_wrote_padding_rows", "hidden_out_off"}


# ---- the six-product census -------------------------------------------------------------------------------------------------------------
def test_census_operands_make_every_kept_product_and_partial_sum_exact():
    census = [c for c in G if c.kind == "census"]
    assert sorted((c.npl, c.tn) for c in census) == sorted(GROUPS)
    assert pk.KEPT == {3: [(2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)], 2: [(1, 0), (0, 1), (0, 0)]}
    for c in census:
        p = pk.gemm_prepared(c)
        assert c.form == "fp32" and not c.bias and c.act == pk.ACT_NONE and not c.post_mul and c.nk == 3
        A, W = p["A_planes"].float(), p["W_planes"].float()
        for q in range(c.npl):
            # plane q: small integers times the fixed power 2^(-4 q), none of them zero
            for t in (A[q], W[q]):
                ints = t * 2.0 ** (pk.CENSUS_SHIFT * q)
                assert (ints == ints.round()).all() and (ints.abs() >= 1).all() and (ints.abs() <= 2).all()
        prods = pk.census_products(p)
        kept, dropped = pk.KEPT[c.npl], pk.DROPPED[c.npl]
        assert sorted(kept + dropped) == sorted(prods) and all((prods[k] != 0).any() for k in dropped)
        # sum |terms| < 2^20 x the smallest unit among the kept terms
        unit = min(2.0 ** (-pk.CENSUS_SHIFT * (i + j)) for i, j in kept)
        mass = sum(A[j].abs().double() @ W[i].abs().double().t() for i, j in kept)
        assert mass.max().item() < 2 ** 20 * unit
        # hence exact in fp32 in any order: fp64 and three fp32 orders agree bit for bit
        want = sum(prods[k] for k in kept)
        K = A.shape[2]
        orders = [list(range(K)), list(range(K - 1, -1, -1)), [k for s in range(4) for k in range(s, K, 4)]]
        for n, order in enumerate(orders):
            acc = torch.zeros(c.M, c.w_rows, dtype=torch.float32)
            for (i, j) in (kept if n != 1 else kept[::-1]):
                for k in order:
                    acc = acc + A[j][:, k, None] * W[i][None, :, k]
            assert torch.equal(acc.double(), want), (pk.gemm_case_id(c), n)
        assert torch.equal(p["ref64"]["C"], want[:, : c.n_out]) and pk.gemm_exact_cols(c) == slice(0, c.n_out)
