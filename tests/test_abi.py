"""The C-ABI library loads on a CPU-only box and exports every symbol include/usflows_hip.h (public) and
include/usflows_hip_internal.h declare (no compute calls here: there is no GPU)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "usflows_hip.h")
INTERNAL_HEADER = os.path.join(ROOT, "include", "usflows_hip_internal.h")


def _declared_functions(*headers):
    """the functions the given headers declare (default: both)"""
    names = set()
    for h in headers or (HEADER, INTERNAL_HEADER):
        src = re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
        names |= set(re.findall(r"\b(usf_[a-z0-9_]+)\s*\(", src))
    return sorted(names)


def _define(header, name):
    return int(re.search(rf"^#define {name} (\d+)\b", open(header).read(), flags=re.M).group(1))


def test_header_declares_expected_entry_points():
    names = _declared_functions()
    for must in ("usf_linear_f32", "usf_coupling_additive_f32", "usf_base_logprob_f32", "usf_base_sample_f32",
                 "usf_scale_f32", "usf_gather_cols_f32", "usf_run_ops", "usf_abi_version", "usf_last_error"):
        assert must in names


def test_library_exports_every_symbol_either_header_declares():
    """every function the public or the internal header declares is exported, and the binding's SYMBOLS are exactly these"""
    from usflows_amd import _ext
    if not _ext.lib_exists():
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_ext.LIB_PATH)
    for name in _declared_functions():
        assert hasattr(lib, name), f"{name} declared in a header but not exported"
    # and the python binding knows every one of them
    assert set(_declared_functions()) == set(_ext.SYMBOLS)


def test_public_and_internal_headers_split_the_exports():
    """include/usflows_hip.h is the stable boundary, include/usflows_hip_internal.h the rest: every export is declared in
    exactly one of them, the binding's PUBLIC_SYMBOLS are the public header's, and the public header does not even name an
    internal entry point"""
    from usflows_amd import _ext
    public, internal = set(_declared_functions(HEADER)), set(_declared_functions(INTERNAL_HEADER))
    assert public | internal == set(_ext.SYMBOLS)
    assert not public & internal
    assert public == set(_ext.PUBLIC_SYMBOLS)
    assert internal == set(_ext.INTERNAL_SYMBOLS)
    text = open(HEADER).read()
    assert not [n for n in sorted(internal) if re.search(rf"\b{n}\b", text)]
    assert '#include "usflows_hip.h"' in open(INTERNAL_HEADER).read()
    # INTEGRATION.md section B tabulates the public entry points only
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rows = [ln for ln in md[md.index("## B."):].split("\n") if ln.startswith("| `")]
    tabulated = {n for ln in rows for n in re.findall(r"`(usf_[a-z0-9_]+)", ln.split(" | ")[0])} & set(_ext.SYMBOLS)
    assert rows and tabulated <= public


def _c_compiler():
    for cc in ("gcc", "cc", "clang", "/opt/rocm/llvm/bin/clang"):
        if shutil.which(cc):
            return cc
    pytest.fail("no C compiler on PATH (the library's build needs one)")


@pytest.mark.parametrize("header", [HEADER, INTERNAL_HEADER], ids=["public", "internal"])
@pytest.mark.parametrize("lang", ["c", "c++"])
def test_header_compiles_on_its_own(header, lang):
    cc = _c_compiler()
    std = ["-std=c99"] if lang == "c" else []
    r = subprocess.run([cc, "-fsyntax-only", "-Wall", "-Werror", *std, "-x", lang, header], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_both_versions_are_checked_on_load(monkeypatch):
    """USF_ABI_VERSION (public header) and USF_INTERNAL_VERSION (internal header): the headers, the binding and the library
    agree, and load() refuses a library whose either number differs from the binding's"""
    from usflows_amd import _ext
    lib = _ext.load()
    assert lib.usf_abi_version() == _ext.USF_ABI_VERSION == _define(HEADER, "USF_ABI_VERSION") == 36
    assert lib.usf_internal_version() == _ext.USF_INTERNAL_VERSION == _define(INTERNAL_HEADER, "USF_INTERNAL_VERSION")
    for name in ("USF_ABI_VERSION", "USF_INTERNAL_VERSION"):
        with monkeypatch.context() as m:
            m.setattr(_ext, "_lib", None)
            m.setattr(_ext, name, getattr(_ext, name) + 1)
            with pytest.raises(RuntimeError, match="ABI mismatch"):
                _ext.load()
    assert _ext.load() is lib


def test_binding_struct_layout_matches_c():
    from usflows_amd import _ext
    lib = _ext.load()          # load() itself cross-checks sizeof() of every descriptor
    assert lib.usf_abi_version() == _ext.USF_ABI_VERSION
    assert lib.usf_sizeof_desc(_ext.OP_LINEAR) == ctypes.sizeof(_ext.LinearDesc)
    assert lib.usf_sizeof_desc(_ext.OP_COUPLING) == ctypes.sizeof(_ext.CouplingDesc)
    # the kind table load() walks covers EVERY struct the binding declares: one added later cannot stay unchecked
    from usflows_amd import _abi
    structs = {v for v in vars(_abi).values() if isinstance(v, type) and issubclass(v, ctypes.Structure) and v is not ctypes.Structure}
    assert len(structs) >= 17 and set(_abi.SIZEOF_KINDS.values()) == structs and len(_abi.SIZEOF_KINDS) == len(structs)
    for kind, st in _abi.SIZEOF_KINDS.items():
        assert lib.usf_sizeof_desc(kind) == ctypes.sizeof(st), st.__name__
    assert lib.usf_coupling_max_width() == 256
    assert [lib.usf_coupling_padded_width(h) for h in (1, 64, 65, 128, 200, 256, 257)] == [64, 64, 128, 128, 256, 256, -1]


def test_argument_errors_are_reported_without_a_gpu():
    """descriptor validation runs before any launch: bad arguments -> negative rc + message"""
    from usflows_amd import _ext
    lib = _ext.load()
    d = _ext.LinearDesc()
    d.M, d.N, d.K = 4, 4, 6            # K % 4 != 0
    d.A = d.W = d.C = 16
    d.lda = d.ldw = 8
    d.ldc = 4
    rc = lib.usf_linear_f32(ctypes.byref(d), None)
    assert rc < 0 and b"multiples of 4" in lib.usf_last_error()
    assert lib.usf_run_ops(None, 3, None) < 0


def test_integration_md_ctypes_stub_matches_the_c_structs():
    """the stub in INTEGRATION.md was shorter than usf_linear_desc (UB for whoever pastes it).  The stub is
    executed here as written (library path substituted); its own asserts compare sizeof with the library."""
    from usflows_amd import _ext
    _ext.load()
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = re.findall(r"```python\n(.*?)```", md, flags=re.S)
    stub = [b for b in blocks if "class LinearDesc" in b]
    assert len(stub) == 1
    code = stub[0].split("def block_affine_backward")[0].replace('"libusflows_hip.so"', repr(_ext.LIB_PATH))
    ns = {}
    exec(code, ns)
    assert ctypes.sizeof(ns["LinearDesc"]) == ctypes.sizeof(_ext.LinearDesc)
    assert [f[0] for f in ns["LinearDesc"]._fields_] == [f[0] for f in _ext.LinearDesc._fields_]


def test_tiny_coupling_rule_of_the_engine_is_the_librarys():
    """FlowEngine.tiny_coupling restates usf_coupling_tiny.hip's eligibility rule (a plan that sets hidden_out on a descriptor the
    library then serves with another kernel is rejected at run time): the two agree over a sweep of shapes, for the forward
    descriptor and for the backward one (segments swapped, hidden layers reversed).  Host-only: usf_coupling_variant launches
    nothing and reads no pointer."""
    import itertools
    from usflows_amd import _ext
    from usflows_amd.engine import FlowEngine
    _ext.load()
    n_checked = n_tiny = 0
    for B, n_pass, n_trans, hidden in itertools.product([1, 32, 256, 257, 4096], [4, 8, 52, 64, 68], [4, 5, 48, 64, 100],
                                                        [[32], [32, 32], [64, 64], [64, 64, 64], [7, 5], [65], [48, 32, 40]]):
        cp = dict(hidden=hidden, pass_n=n_pass, tr_n=n_trans)
        py = FlowEngine.tiny_coupling(None, cp, B)
        both = _coupling_variant(B, n_pass, hidden, n_trans) == 3 and _coupling_variant(B, n_trans, hidden[::-1], n_pass) == 3
        assert py == both, (B, n_pass, n_trans, hidden, py, both)
        n_checked += 1
        n_tiny += int(py)
    assert n_checked > 800 and 20 < n_tiny < n_checked


def _coupling_variant(B, n_pass, hidden, n_trans):
    """usf_coupling_variant of a forward coupling descriptor with the engine's weight strides (pointers never read)"""
    from usflows_amd import _ext
    d = _ext.CouplingDesc()
    d.z = d.out = 0x10000
    d.ldz = d.ldo = 512
    d.M, d.off_pass, d.n_pass, d.off_trans, d.n_trans = B, 0, n_pass, 256, n_trans
    d.n_hidden = len(hidden)
    r32 = lambda v: (v + 31) // 32 * 32
    for i, h in enumerate(hidden):
        d.hidden[i] = h
    d.W_in, d.ldw_in, d.b_in = 0x20000, r32(n_pass), 0x30000
    for i in range(1, len(hidden)):
        d.W_hid[i - 1], d.ldw_hid[i - 1], d.b_hid[i - 1] = 0x40000 + 0x10000 * i, 64, 0x30000
    d.W_out, d.ldw_out, d.b_out = 0x80000, 64, 0x30000
    d.sign, d.slope, d.act = 1.0, 0.01, _ext.ACT_LEAKY_RELU
    return _ext.load().usf_coupling_variant(d)


def test_tiny_coupling_decision_of_the_engine_follows_the_library_knob():
    """usf_set_tuning("coupling_tiny", 0) switches the tiny-layer kernel off in the library: the engine must not emit the fused
    coupling op (with hidden_out / GATE, which only that kernel serves) for such layers any more, and the knob's value is part of
    the plan-cache key (tests/test_training_emulated.py builds the plans)"""
    from usflows_amd.config import config
    from usflows_amd.engine import FlowEngine
    shapes = [(32, 1, [32, 32], 1), (32, 5, [32, 32], 5), (256, 50, [32, 32], 50), (1, 17, [32], 17)]
    old = config.get_lib("coupling_tiny", 1)
    try:
        config.set_lib("coupling_tiny", 1)
        for B, n_pass, hidden, n_trans in shapes:
            assert FlowEngine.tiny_coupling(None, dict(hidden=hidden, pass_n=n_pass, tr_n=n_trans), B)
            assert _coupling_variant(B, n_pass, hidden, n_trans) == 3
        config.set_lib("coupling_tiny", 0)
        for B, n_pass, hidden, n_trans in shapes:
            assert _coupling_variant(B, n_pass, hidden, n_trans) != 3
            assert not FlowEngine.tiny_coupling(None, dict(hidden=hidden, pass_n=n_pass, tr_n=n_trans), B)
    finally:
        config.set_lib("coupling_tiny", old)
