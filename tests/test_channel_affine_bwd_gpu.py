"""usf_channel_affine_bwd_f32 on the device: one launch per case of channel_affine_bwd_cases.py, EVERY element of dx, dW and db
against fp64 with test_wide_wgrad_gpu.py's bound (2e-6 of max|ref|; the numpy fp32 statement of the same summation order stays
under 1.5e-7 on these cases, test_channel_affine_bwd_cpu.py), the same call twice and the deferred sum against the immediate one
bit for bit, refusals that write nothing.  profiles/channel_affine_bwd_parity.md has the worst figures (from this file's output
under -s)."""
import ctypes as C

import pytest
import torch

from usflows_amd import _ext
from usflows_amd.config import config
from channel_affine_bwd_cases import CASES, MULTI_TRIP_C1, REFUSED, aligned, case_id, check, emulate, inputs, ref64, wants

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class _cap:
    """the tuning aid channel_affine_bwd_blocks for the length of a block"""

    def __init__(self, cap):
        self.cap = cap

    def __enter__(self):
        self.old = config.get_lib("channel_affine_bwd_blocks", 0)
        config.set_lib("channel_affine_bwd_blocks", self.cap)

    def __exit__(self, *exc):
        config.set_lib("channel_affine_bwd_blocks", self.old)
        return False


def _call(case, x, dy, W, ps):
    _, want_dx, want_db = wants(case)
    return _ext.channel_affine_bwd(x, dy, W, pre_sub=ps, want_dx=want_dx, want_bias=want_db)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_element_against_fp64_and_twice_the_same_bits(case):
    B, Cc, P, form, cap = case
    x, dy, W, ps = inputs(case, DEV)
    _, want_dx, want_db = wants(case)
    assert (x.data_ptr() % 16 == 0) == aligned(case) and (dy.data_ptr() % 16 == 0) == aligned(case)
    with _cap(cap):
        v = _ext.channel_affine_bwd_variant(B, Cc, P, aligned=aligned(case), want_bias=want_db)
        assert v["served"] == 1 and v["vec"] == int(aligned(case) and P % 4 == 0) and v["blocks"] == (min(cap, v["blocks"]) if cap else v["blocks"])
        r1 = _call(case, x, dy, W, ps)
        r2 = _call(case, x, dy, W, ps)
    assert r1 is not None
    dx, dW, db = r1
    rx, rW, rb = ref64(x, dy, W, ps)
    name = case_id(case)
    check(dW, rW, f"{name} dW")
    assert dW.shape == (Cc, Cc)
    if want_db:
        check(db, rb, f"{name} db")
    else:
        assert db is None
    if want_dx:
        check(dx, rx, f"{name} dx")
        assert dx.shape == x.shape
    else:
        assert dx is None
    for a, b in zip(r1, r2):
        assert (a is None and b is None) or torch.equal(a, b)
    # beside the bound: the distance to the numpy fp32 statement of the same order (printed, not held: fmaf through fp64 rounds twice)
    eW, eb = emulate(x, dy, ps, dict(v, slot_floats=Cc * Cc + Cc))
    print(f"{name}: dW differs from the numpy statement by {float((dW.cpu() - torch.from_numpy(eW)).abs().max()):.2e}")


def _raw(x, dy, dx, W, ps, dpar, Cc, ws, ws_n, job=None, want_db=True):
    B, P = x.shape[0], x.shape[2] * x.shape[3]
    return _ext.load().usf_channel_affine_bwd_f32(
        x.data_ptr(), dy.data_ptr(), _ext.ptr(dx), B, Cc, P, W.data_ptr(), _ext.ptr(ps), dpar.data_ptr(),
        dpar.data_ptr() + 4 * Cc * Cc if want_db else None, ws.data_ptr(), ws_n,
        C.cast(job, C.c_void_p) if job is not None else None, _ext.current_stream(x.device))


@pytest.mark.parametrize("case", [MULTI_TRIP_C1, (33, 12, 196, "presub", 0), (33, 5, 49, "plain", 0), (400, 3, 49, "plain", 0)], ids=case_id)
def test_the_deferred_sum_gives_the_bits_of_the_immediate_one(case):
    """job != NULL: the entry point stops in front of its last sum and describes it; run through usf_partial_sum_jobs_f32 (as a
    backward pass's queue does) it writes the same bits -- one round and two"""
    B, Cc, P, form, cap = case
    x, dy, W, ps = inputs(case, DEV)
    lib = _ext.load()
    ws_n = lib.usf_channel_affine_bwd_workspace(B, Cc, P)
    ws = torch.empty(ws_n, device=DEV)
    now = torch.full((Cc * Cc + Cc,), 7.0, device=DEV)
    later = torch.full((Cc * Cc + Cc,), 7.0, device=DEV)
    dx1, dx2 = torch.empty_like(x), torch.empty_like(x)
    assert _raw(x, dy, dx1, W, ps, now, Cc, ws, ws_n) == 0
    torch.cuda.synchronize()
    ws2 = torch.empty(ws_n, device=DEV)
    job2 = (_ext.PsumJob * 2)()
    assert _raw(x, dy, dx2, W, ps, later, Cc, ws2, ws_n, job2) == 0
    torch.cuda.synchronize()
    assert (later == 7.0).all(), "the deferred call wrote its sums"
    two = _ext.channel_affine_bwd_variant(B, Cc, P)["rounds"] == 2
    assert (job2[0].nparts > 0) == two and job2[1].nparts > 0
    st = _ext.current_stream(torch.device(DEV))
    for stage in (0, 1):
        if job2[stage].nparts > 0:
            raw, off, n = _ext._job_table([job2[stage]], lambda j: ((j.n + 255) // 256 if j.vec4 else (j.n + 63) // 64) * j.rows)
            t = torch.frombuffer(raw, dtype=torch.uint8).to(DEV)
            assert lib.usf_partial_sum_jobs_f32(t.data_ptr(), t.data_ptr() + off, n, st) == 0
            torch.cuda.synchronize()
    assert torch.equal(now, later) and torch.equal(dx1, dx2) and not (now == 7.0).any()


def test_refusals_and_errors_write_nothing():
    lib = _ext.load()
    canary = 12345.0
    for B, Cc, P in REFUSED:
        n = max(B * max(Cc, 1) * max(P, 1), 1)
        x, dy, dx = (torch.full((n,), canary, device=DEV).view(B, -1, 1, 1) for _ in range(3))
        dpar = torch.full((max(Cc, 1) ** 2 + max(Cc, 1),), canary, device=DEV)
        ws = torch.full((1 << 14,), canary, device=DEV)
        W = torch.ones(max(Cc, 1) ** 2, device=DEV)
        rc = lib.usf_channel_affine_bwd_f32(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), B, Cc, P, W.data_ptr(), None, dpar.data_ptr(),
                                            dpar.data_ptr() + 4 * Cc * Cc, ws.data_ptr(), ws.numel(), None,
                                            _ext.current_stream(x.device))
        assert rc == 1, (B, Cc, P)
        torch.cuda.synchronize()
        assert (dx == canary).all() and (dpar == canary).all() and (ws == canary).all()
    assert _ext.channel_affine_bwd(torch.randn(4, 13, 7, 7, device=DEV), torch.randn(4, 13, 7, 7, device=DEV),
                                   torch.randn(13, 13, device=DEV)) is None
    # an empty batch: a no-op that returns 0
    e = torch.empty(0, 4, 14, 14, device=DEV)
    dpar = torch.full((20,), canary, device=DEV)
    ws = torch.full((4096,), canary, device=DEV)
    assert _raw(e, e, None, torch.ones(16, device=DEV), None, dpar, 4, ws, ws.numel()) == 0
    torch.cuda.synchronize()
    assert (dpar == canary).all() and (ws == canary).all()
    dx, dW, db = _ext.channel_affine_bwd(e, e, torch.ones(4, 4, device=DEV))
    assert dx.shape == e.shape and not dW.any() and not db.any()
    # a workspace one float short, db apart from dW, in-place: errors, nothing launched
    case = (3, 4, 196, "plain", 0)
    x, dy, W, ps = inputs(case, DEV)
    need = lib.usf_channel_affine_bwd_workspace(3, 4, 196)
    dx = torch.full_like(x, canary)
    dpar = torch.full((20 + 8,), canary, device=DEV)
    ws = torch.full((need,), canary, device=DEV)
    assert _raw(x, dy, dx, W, ps, dpar, 4, ws, need - 1) < 0 and b"workspace too small" in lib.usf_last_error()
    rc = lib.usf_channel_affine_bwd_f32(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), 3, 4, 196, W.data_ptr(), None, dpar.data_ptr(),
                                        dpar.data_ptr() + 4 * 20, ws.data_ptr(), need, None, _ext.current_stream(x.device))
    assert rc < 0 and b"db must follow dW" in lib.usf_last_error()
    assert _raw(x, dy, x, W, ps, dpar, 4, ws, need) < 0 and b"in-place" in lib.usf_last_error()
    torch.cuda.synchronize()
    assert (dx == canary).all() and (dpar == canary).all() and (ws == canary).all()
    assert _raw(x, dy, dx, W, ps, dpar, 4, ws, need) == 0
    torch.cuda.synchronize()
    assert not (dx == canary).any() and not (dpar[:20] == canary).any() and (dpar[20:] == canary).all()
