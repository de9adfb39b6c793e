"""tests/coupling_kernel_cases.py held to account without a GPU: the table reaches every instantiation and edge it claims, every
case names the kernel family the library would launch (usf_coupling_variant, host-only), the checker accepts the fp32 torch-CPU
evaluation of every case and reports each of five planted defects, and the argument checks that belong to the two MFMA kernels
refuse before any launch.  The library calls here launch nothing and read no pointer; without the built library they cannot run
(as in tests/test_abi.py, the library is built first when it is missing)."""
import ctypes
import types

import pytest
import torch

import coupling_kernel_cases as ck


@pytest.fixture(scope="module")
def ext():
    from usflows_amd import _ext
    if not _ext.lib_exists():
        import __graft_entry__
        __graft_entry__.build()
    _ext.load()
    return _ext


def test_table_reaches_every_instantiation_mode_and_edge():
    cases = ck.CASES
    assert 60 <= len(cases) <= 150 and len(set(cases)) == len(cases)
    assert all(c.M <= 1153 for c in cases)
    inst = {ck.instantiation(c) for c in cases}
    assert inst == {("f32", nh, hp) for nh in (1, 2, 3) for hp in (64, 128, 256)} | {("bf16x3", nh, 256) for nh in (1, 2, 3)}
    # all four modes of every bf16x3 instantiation; the exact-f32 kernel has the plain and the context form only
    assert {(len(c.hidden), c.mode) for c in cases if c.family == "bf16x3"} == {(nh, m) for nh in (1, 2, 3) for m in ck.B3_MODES}
    assert {c.mode for c in cases if c.family == "f32"} == {"plain", "ctx"}
    for nh in (1, 2, 3):
        for hp in (64, 128, 256):
            assert {c.mode for c in cases if ck.instantiation(c) == ("f32", nh, hp)} == {"plain", "ctx"}, (nh, hp)
    f32 = [c for c in cases if c.family == "f32"]
    b3 = [c for c in cases if c.family == "bf16x3"]
    assert {c.M for c in f32} == {1, 15, 16, 17, 63, 64, 65, 257, 300}
    assert {c.M for c in b3} == {1024, 1025, 1151, 1153}
    assert {c.hidden for c in f32} >= {(64,), (1,), (40, 24), (65, 128), (128, 7), (7, 130, 256), (256, 256, 256), (129,)}
    assert {c.hidden for c in b3} == {(129,), (256,), (200, 256), (256, 160), (136, 256, 130)}
    for fam in (f32, b3):
        assert {c.n_pass for c in fam} == {4, 16, 20, 32, 36, 52, 100}
        assert {c.n_trans for c in fam} == {1, 3, 4, 30, 32, 33, 37, 65}
        assert {c.n_pass % 32 for c in fam} == {4, 16, 20, 0} and {c.n_trans % 4 for c in fam} == {0, 1, 2, 3}
        assert {c.off_pass < c.off_trans for c in fam} == {True, False}
        assert {c.sign for c in fam} == {1.0, -1.0}
        assert {(c.act, c.slope) for c in fam if c.mode != "gate"} == {(ck.ACT_LEAKY_RELU, 0.01), (ck.ACT_LEAKY_RELU, 0.0), (ck.ACT_NONE, 0.0)}
    assert all((c.act == ck.ACT_GATE) == (c.mode == "gate") for c in cases)
    for c in cases:
        # what the MFMA kernels ask of a descriptor, and slack columns between and behind the segments
        nt4 = ck.ceil_to(c.n_trans, 4)
        assert c.n_pass % 4 == 0 and c.off_pass % 4 == 0 and c.off_trans % 4 == 0 and c.ldz % 4 == 0, c
        lo, hi = sorted([(c.off_pass, c.off_pass + c.n_pass), (c.off_trans, c.off_trans + nt4)])
        assert lo[1] < hi[0] and hi[1] < c.ldz, c
        assert all(1 <= h <= 256 for h in c.hidden) and 1 <= len(c.hidden) <= 3
        if c.family == "bf16x3":
            assert 128 < max(c.hidden) <= 256 and c.M >= 1024
    # each distinct weight set is shared: fewer sets than cases
    assert len({(c.n_pass, c.hidden, c.n_trans) for c in cases}) <= len(cases)


def test_every_case_names_the_kernel_the_library_would_launch(ext):
    lib = ext.load()
    with ck.tiny_kernel_off():
        for c in ck.CASES:
            assert ck.variant(c, lib, ext.CouplingDesc) == ck.VARIANT[c.family], ck.case_id(c)
    # the knob matters: with it on, the small exact-f32 cases are the tiny-layer kernel's
    from usflows_amd.config import config
    if config.get_lib("coupling_tiny", 1):
        assert any(ck.variant(c, lib, ext.CouplingDesc) == 3 for c in ck.CASES if c.family == "f32")
    # without its split planes a bf16x3 case is the exact-f32 kernel's
    c = next(c for c in ck.CASES if c.family == "bf16x3")
    d = ck.descriptor(c, ck.fake_ptr, ext.CouplingDesc)
    d.split_out = None
    assert lib.usf_coupling_variant(ctypes.byref(d)) == 1


def test_hand_built_images_follow_the_padding_contract():
    """shapes, zero padding, planes that sum to the image, and the K permutation read back against the header's sentence"""
    c = next(c for c in ck.CASES if c.family == "bf16x3" and c.hidden == (136, 256, 130))
    im, w = ck.case_images(c), ck.weights(c.n_pass, c.hidden, c.n_trans)
    Kp, Np = ck.ceil_to(c.n_pass, 32), ck.ceil_to(c.n_trans, 32)
    assert im["Hp"] == 256 and im["W_in"].shape == (256, Kp) and im["W_out"].shape == (Np, 256)
    assert [tuple(W.shape) for W in im["W_hid"]] == [(256, 256)] * 2 and im["b_in"].shape == (256,) and im["b_out"].shape == (Np,)
    assert torch.equal(im["W_in"][:136, : c.n_pass], w["Ws"][0]) and im["W_in"][136:].abs().sum() == 0 and im["W_in"][:, c.n_pass:].abs().sum() == 0
    assert torch.equal(im["W_hid"][1][:130, :256], w["Ws"][2]) and im["W_hid"][1][130:].abs().sum() == 0
    assert torch.equal(im["W_out"][: c.n_trans, :130], w["Ws"][3]) and im["W_out"][:, 130:].abs().sum() == 0
    assert im["split_in"].shape == (3, 256, Kp) and im["split_in"].dtype == torch.bfloat16
    assert torch.equal(im["split_in"].float().sum(0), im["W_in"])
    # position 8 g + j of a block of 32 holds unit 4 g + j (j < 4) or 16 + 4 g + (j - 4) (j >= 4)
    s = im["split_hid"][0].float().sum(0)
    for pos, unit in [(0, 0), (3, 3), (4, 16), (7, 19), (8, 4), (12, 20), (31, 31), (32 + 9, 32 + 5), (224 + 21, 224 + 25)]:
        assert torch.equal(s[:, pos], im["W_hid"][0][:, unit]), (pos, unit)
    assert sorted(ck.k_permutation(256).tolist()) == list(range(256))
    assert torch.equal(im["split_out"].float().sum(0), im["W_out"][:, ck.k_permutation(256)])


def test_checker_accepts_the_fp32_evaluation_of_every_case():
    for c in ck.CASES:
        z, hidden = ck.fp32_result(c)
        assert ck.check(z, hidden, c) == [], ck.case_id(c)
        m = ck.measure(z, hidden, c)
        assert m["err"] == m["err32"] <= m["bound"]


def _pick(pred):
    found = [c for c in ck.CASES if pred(c)]
    assert found
    return found[0]


DEFECT_CASES = [
    _pick(lambda c: c.family == "f32" and c.M >= 17 and c.n_trans % 4 and c.n_pass > 16),
    _pick(lambda c: c.family == "f32" and c.M >= 257 and c.n_pass > 32 and c.mode == "ctx"),
    _pick(lambda c: c.mode == "hidden_out" and c.hidden[0] < 256 and c.n_trans % 4 and c.n_pass > 16),
    _pick(lambda c: c.mode == "gate" and min(c.hidden) < 256 and c.n_pass > 16),
]


@pytest.mark.parametrize("c", DEFECT_CASES, ids=ck.case_id)
def test_checker_reports_each_planted_defect(c):
    p = ck.prepared(c)
    tr = slice(c.off_trans, c.off_trans + c.n_trans)
    clean_z, clean_h = ck.fp32_result(c)
    assert ck.check(clean_z, clean_h, c) == []
    clone_h = lambda: None if clean_h is None else [h.clone() for h in clean_h]      # noqa: E731

    # the last transformed column left at its input
    z = clean_z.clone()
    z[: c.M, c.off_trans + c.n_trans - 1] = p["z"][: c.M, c.off_trans + c.n_trans - 1]
    bad = ck.check(z, clone_h(), c)
    assert len(bad) == 1 and f"transformed column {c.n_trans - 1}" in bad[0], bad

    # the last 16-k step of W_in dropped
    z, h = ck.fp32_result(c, drop_last_kstep=True)
    bad = ck.check(z, h, c)
    assert any("transformed columns: error" in b for b in bad), bad
    if h is not None:
        assert any("hidden_out[0]: error" in b for b in bad), bad

    # row M - 1 computed from row M - 2
    z = clean_z.clone()
    z[c.M - 1, tr] = p["z"][c.M - 1, tr] + (clean_z[c.M - 2, tr] - p["z"][c.M - 2, tr])
    bad = ck.check(z, clone_h(), c)
    assert len(bad) == 1 and f"at row {c.M - 1}," in bad[0], bad

    # one slack column overwritten: the columns [n_trans, ceil4(n_trans)) where there are any, the row's last column, a row >= M
    cols = [c.ldz - 1] + ([c.off_trans + c.n_trans] if c.n_trans % 4 else [])
    for row, col in [(0, col) for col in cols] + [(c.M, c.off_trans)]:
        z = clean_z.clone()
        z[row, col] = 0.0
        bad = ck.check(z, clone_h(), c)
        assert len(bad) == 1 and f"the first at row {row}, column {col}" in bad[0], bad
    # ... or rewritten with another NaN
    z = clean_z.clone()
    z[0, c.ldz - 1] = float("nan")
    assert (ck._bits(z) != ck._bits(clean_z)).sum() == 1
    assert len(ck.check(z, clone_h(), c)) == 1

    if clean_h is not None:
        # one padded hidden unit given a non-zero bias: its activation shows in the padded columns of hidden_out (the next
        # layer's weights are zero there, so the transformed columns do not change)
        l = next(l for l, w in enumerate(c.hidden) if w < p["Hp"])
        h = clone_h()
        h[l][: c.M, c.hidden[l]] = 0.25
        bad = ck.check(clean_z.clone(), h, c)
        assert len(bad) == 1 and f"hidden_out[{l}]: the padded units' columns" in bad[0], bad
        # sentinel regions
        h = clone_h()
        h[0][0, p["Hp"]] = 0.0
        assert any("columns >= 256 written" in b for b in ck.check(clean_z.clone(), h, c))
        h = clone_h()
        h[-1][c.M, 0] = 0.0
        assert any("rows >= M written" in b for b in ck.check(clean_z.clone(), h, c))
        assert any("missing" in b for b in ck.check(clean_z.clone(), None, c))


def _rc(ext, d):
    lib = ext.load()
    rc = lib.usf_coupling_additive_f32(ctypes.byref(d), None)
    return rc, lib.usf_last_error()


@pytest.mark.parametrize("family", ["f32", "bf16x3"])
def test_segments_outside_the_rows_or_overlapping_are_refused_before_any_launch(ext, family):
    """usf_coupling_dispatch checked off_trans + ceil4(n_trans) <= ldz only; the tiny-layer dispatch has checks of its own"""
    c = next(c for c in ck.CASES if c.family == family and c.M > 256 and c.off_pass > c.off_trans and c.n_pass >= 8)
    mk = lambda: ck.descriptor(c, ck.fake_ptr, ext.CouplingDesc)      # noqa: E731
    # the conditioning segment sticks out of the rows
    d = mk()
    d.off_pass = c.ldz - c.n_pass + 4
    rc, msg = _rc(ext, d)
    assert rc == -2 and b"column segments outside the rows" in msg
    d = mk()
    d.off_pass = -4
    assert _rc(ext, d)[0] == -2
    # the segments overlap: by one group of four columns, entirely, and with the transformed segment inside the other
    for off_pass, off_trans in [(c.off_trans + ck.ceil_to(c.n_trans, 4) - 4, c.off_trans), (c.off_trans, c.off_trans), (0, 4)]:
        d = mk()
        d.off_pass, d.off_trans = off_pass, off_trans
        if off_pass + c.n_pass > c.ldz or off_trans + ck.ceil_to(c.n_trans, 4) > c.ldz:
            d.ldz = d.ldo = c.ldz + 128
        rc, msg = _rc(ext, d)
        assert rc == -2 and b"overlap" in msg, (off_pass, off_trans, rc, msg)
    # adjacent segments are fine for the check (the variant call shows the descriptor is otherwise the same kernel's)
    d = mk()
    assert ext.load().usf_coupling_variant(ctypes.byref(d)) == ck.VARIANT[family]


def test_bf16x3_kernel_is_not_eligible_where_its_32_bit_offsets_would_wrap(ext):
    """the bf16x3 kernel forms row * ldz + offset in 32 bits: a row buffer of 2^32 elements or more goes to the exact-f32 kernel
    (64-bit offsets), and the engine's save_fused_hidden -- hidden_out is the bf16x3 kernel's alone -- restates the limit"""
    from usflows_amd.engine import FlowEngine
    lib = ext.load()
    c = next(c for c in ck.CASES if c.family == "bf16x3" and c.mode == "plain")
    for ldz, m_at in [(4096, 1 << 20), (3072, 1398102), (c.ldz + (-c.ldz) % 4, -(-(1 << 32) // (c.ldz + (-c.ldz) % 4)))]:
        assert (m_at - 1) * ldz < (1 << 32) <= m_at * ldz
        d = ck.descriptor(c, ck.fake_ptr, ext.CouplingDesc)
        d.ldz = d.ldo = ldz
        d.M = m_at
        assert lib.usf_coupling_variant(ctypes.byref(d)) == 1, (ldz, m_at)
        d.M = m_at - 1
        assert lib.usf_coupling_variant(ctypes.byref(d)) == 2, (ldz, m_at)
        eng = types.SimpleNamespace(gemm_mode="bf16x3", LD=ldz, LDn=ldz - 4, hmax=256)
        cp = dict(hidden=[256, 256], tr_n=32, tr_off=0)
        assert FlowEngine.save_fused_hidden(eng, cp, m_at - 1) and not FlowEngine.save_fused_hidden(eng, cp, m_at)
        eng.LD, eng.LDn = ldz - 4, ldz                                  # the backward launch's rows may be the wider ones
        assert FlowEngine.save_fused_hidden(eng, cp, m_at - 1) and not FlowEngine.save_fused_hidden(eng, cp, m_at)
    # with hidden_out such a descriptor is an error, not a silent wrap: the exact-f32 kernel does not store activations
    d = ck.descriptor(next(c for c in ck.CASES if c.mode == "hidden_out"), ck.fake_ptr, ext.CouplingDesc)
    d.ldz = d.ldo = 4096
    d.M = 1 << 20
    rc = lib.usf_coupling_additive_f32(ctypes.byref(d), None)
    assert rc == -2 and b"hidden_out / USF_ACT_GATE are served by" in lib.usf_last_error()
