"""Seeded radial sampling without a GPU: the library exports usf_radial_sample_norm_f32 as an internal entry point, and the numpy
emulator of its radius draw (tests/emulator_radial_sample.py) is split-invariant and has the distribution it claims."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import emulator_radial_sample as emu
from radial_sample_cases import CASE_NAMES, M_DRAW, SEED, cases, ks_distance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "usf_radial_sample_norm_f32"


def test_library_exports_the_sampler_as_an_internal_entry_point():
    from usflows_amd import _ext
    if not _ext.lib_exists():
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_ext.LIB_PATH)
    assert hasattr(lib, NAME)
    assert NAME in _ext.INTERNAL_SYMBOLS and NAME not in _ext.PUBLIC_SYMBOLS
    assert re.search(rf"\b{NAME}\s*\(", open(os.path.join(ROOT, "include", "usflows_hip_internal.h")).read())
    assert NAME not in open(os.path.join(ROOT, "include", "usflows_hip.h")).read()
    # the unfused direction kernel keeps its place in the public ABI
    assert "usf_radial_sample_f32" in _ext.PUBLIC_SYMBOLS and hasattr(lib, "usf_radial_sample_f32")


def test_argument_errors_come_back_without_a_launch():
    """validation runs on the host before anything is launched: no GPU needed"""
    from usflows_amd import _ext
    lib = _ext.load()
    fn = getattr(lib, NAME)
    p = 0x1000                                       # never dereferenced
    assert fn(None, 0, 8, 0, 0, None, _ext.NORM_GAMMA, 65, p, p, p, p, 1, 0, 0, None) == -2
    assert b"K = 65" in lib.usf_last_error()
    assert fn(None, 0, 8, 0, 0, None, _ext.NORM_GAMMA, 1, p, p, None, None, 1, 0, 0, None) == -1
    assert b"null pointer" in lib.usf_last_error()
    assert fn(p, 8, 8, 8, 7, p, _ext.NORM_GAMMA, 1, p, p, None, p, 1, 0, 0, None) == -2
    assert b"not an Lp-radial id" in lib.usf_last_error()
    assert fn(None, 0, 8, 0, 0, None, _ext.NORM_CHI, 1, p, p, None, p, 1, 0, 0, None) == -2          # Chi: raw only
    assert fn(None, 0, 8, 0, 0, None, _ext.NORM_GAMMA, 2, p, p, None, p, 1, 0, 0, None) == -1        # K > 1 needs logits
    assert fn(None, 0, 0, 0, 0, None, _ext.NORM_HALFNORMAL, 1, p, None, None, p, 1, 0, 0, None) == 0      # empty draw: nothing to do


def test_philox_known_answer():
    """Random123's published known-answer vectors for philox4x32_10 (counter and key all zeros / all ones): the emulator's
    generator is the standard one"""
    w = emu.philox4x32_10(np.zeros(1, dtype=np.uint64), 0, 0)
    assert [int(x[0]) for x in w] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    full = 0xFFFFFFFFFFFFFFFF
    w = emu.philox4x32_10(np.full(1, full, dtype=np.uint64), full, full)
    assert [int(x[0]) for x in w] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("row_offset", [0, 2 ** 33 + 5])
def test_emulator_is_split_invariant(name, row_offset):
    kind, a, b, l = cases()[name]
    M = 2048
    full = emu.radii(kind, a, b, l, M=M, seed=SEED, offset=3, row_offset=row_offset)
    tail = emu.radii(kind, a, b, l, M=M // 2, seed=SEED, offset=3, row_offset=row_offset + M // 2)
    assert np.array_equal(full[M // 2:], tail)
    assert np.isfinite(full).all() and (full > 0).all()
    assert not np.array_equal(full[: M // 2], tail)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_emulator_distribution(name):
    """KS distance to the analytic (mixture) CDF < 1.7 / sqrt(M): the bound the Laplace and Normal heads are held to
    (tests/test_kernels_gpu.py)"""
    kind, a, b, l = cases()[name]
    stats = {}
    r = emu.radii(kind, a, b, l, M=M_DRAW, seed=SEED, offset=0, stats=stats)
    ks = ks_distance(kind, a, b, l, r)
    print(f"{name}: KS * sqrt(M) = {ks * math.sqrt(M_DRAW):.3f} {stats}")
    assert ks < 1.7 / math.sqrt(M_DRAW)
    if kind in ("gamma", "chi"):
        assert stats["capped"] == 0 and stats["max_attempts"] <= 8
