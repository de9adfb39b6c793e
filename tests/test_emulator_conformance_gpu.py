"""The CPU emulation (tests/emulator.py, emulator_ctx.py, emulator_vctx.py) held to the kernels, op by op, on a real MI355X.

The `-m "not gpu"` suite checks the host code (engine.py, engine_planes.py, training.py) against the emulation; this module checks
the emulation against the library:

A. plans in lockstep -- the same flow built on the CPU and on the device gives the same op array (every field; pointers as
   (owner tensor, byte offset)); then every launch of the plan runs on the device and in the emulator from identical bits, and
   every workspace tensor is compared in full, padding included: what the emulator leaves alone the device leaves alone, what
   the emulator writes the device writes within the kernel tests' bounds (bit-equal where the step is exact);
B. the direct-call emulations install_training_emulation / install_prep_emulation patch in, entry point by entry point;
C. the argument sets the library's own "rejects" tests hand to it: the emulation refuses them too.
"""
import contextlib
import ctypes as C
import math

import pytest
import torch

import emulator
import emulator_ctx
import emulator_vctx
import vctx_cases
from golden_util import load_case
from model_util import build_flow
from oracle import usflows_oracle as orc
from usflows_amd import _ext
from usflows_amd.engine import FlowEngine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# ---- every region left out of a comparison ---------------------------------------------------------------------------------
# (buffer, region, the header sentence that makes the region unspecified).  Nothing else is skipped; an entry may not cover an
# element a later step of the same plan reads into a logical result.
EXCLUSIONS = [
    ("every planes buffer (ws/pz*, ws/pH*, the planes arguments of part B)", "rows [M, 16 ceil(M / 16)) of the last 16-row panel",
     "include/usflows_hip.h: \"Rows >= M of the last panel are padding (any value).\"  The GEMM kernels compute them like any row "
     "(bias included), the emulator writes zeros.  Row m of every op's output depends on row m of its inputs only, and the ops "
     "that leave the planes format store rows < M only -- user_out, nat2 and bpart are compared in full -- so no logical result "
     "reads them.  (usf_wgrad_blocked_f32 sums over them: its header asks for zeros there and says which producers give them.)"),
    ("the workspace of a queued usf_wgrad_blocked_plan_f32 call (ws= of _ext.wgrad_blocked, part B)", "all of it",
     "include/usflows_hip_internal.h: \"G / colsum_out stay unwritten and the workspace stays in use until a "
     "usf_wgrad_reduce_jobs_f32 launch containing the job has run\" -- partial sums in the kernel's own layout; nothing reads "
     "them but that launch, whose outputs G and colsum are compared in full."),
    ("planes_out of _ext.linear where the bf16x3 kernel serves the product (W_split, more than 768 rows; part B)",
     "columns [K, ceil32(K)) of rows [0, M)",
     "include/usflows_hip_internal.h: \"columns [K, ceil32(K)) receive finite padding\".  The test asserts that they are finite; "
     "usf_wgrad_planes_f32 reads columns [a_off, a_off + K) of the operand only."),
]

ROWS = (1, 37)              # one row; two full 16-row panels + five ragged rows
_MEMBER = {_ext.OP_LINEAR: "linear", _ext.OP_COUPLING: "coupling", _ext.OP_PACK_PLANES: "pack_planes",
           _ext.OP_GEMM_PLANES: "gemm_planes", _ext.OP_COUPLING_PLANES: "coupling_planes", _ext.OP_GATED_NORM: "gated_norm",
           _ext.OP_CALL: "call"}
_PREFIX_ENTRY = {_ext.FN_COUPLING_PLANES_CTX: "usf_coupling_planes_ctx", _ext.FN_COUPLING_VCTX: "usf_coupling_additive_vctx_f32"}


@contextlib.contextmanager
def _cpu_prep():
    """the parameter prep of a CPU engine runs on the emulation; the device engine built afterwards sees the real binding"""
    with pytest.MonkeyPatch.context() as mp:
        emulator.install_prep_emulation(mp)
        yield


@pytest.fixture(scope="module", autouse=True)
def _prefix_ops():
    """the two context prefix ops in the interpreter; and few torch threads: the emulator's tensors are tiny, a pool as wide as
    the machine spends its time waking up"""
    threads = torch.get_num_threads()
    torch.set_num_threads(min(threads, 4))
    with pytest.MonkeyPatch.context() as mp:
        emulator_ctx.register(mp)
        emulator_vctx.register(mp)
        yield
    torch.set_num_threads(threads)


# ---- naming every tensor a plan can point into (PtrMap run backwards) -------------------------------------------------------
def _walk(obj, path, out, seen):
    if torch.is_tensor(obj):
        if obj.numel() > 0:
            out.append((path, obj))
    elif isinstance(obj, dict):
        if id(obj) in seen:
            return
        seen.add(id(obj))
        for n, (k, v) in enumerate(obj.items()):
            _walk(v, f"{path}/{k if isinstance(k, str) else '#%d' % n}", out, seen)     # (keys may carry id()s: by position)
    elif isinstance(obj, (list, tuple)):
        if id(obj) in seen:
            return
        seen.add(id(obj))
        for n, v in enumerate(obj):
            _walk(v, f"{path}/{n}", out, seen)


def _named_tensors(eng, plan, x, out):
    """[(name, tensor)] in a device-independent order: workspace, the caller's tensors, index vectors, the pack"""
    named, seen = [], set()
    for n, t in plan["ws"].items():
        if torch.is_tensor(t) and t.numel() > 0:
            named.append((f"ws/{n}", t))
    named.append(("user_in", x))
    if out is not None:
        named.append(("user_out", out))
    _walk(eng.__dict__.get("_idx_cache", {}), "eng/idx", named, seen)
    _walk(eng.__dict__.get("_gidx", {}), "eng/gidx", named, seen)
    _walk(plan["pk"], "pk", named, seen)
    return named


def _span(t):
    return (sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1) * t.element_size()


def _resolve(named, ptr):
    for name, t in named:
        lo = t.data_ptr()
        if lo <= ptr < lo + _span(t):
            return name, ptr - lo
    return None


def _ptr_map(named):
    pm = emulator.PtrMap()
    for _, t in sorted(named, key=lambda nt: -_span(nt[1])):          # (an alias resolves to the largest tensor that holds it)
        if t.is_contiguous():
            pm.add(t)
    return pm


# ---- A.1: the same plan ------------------------------------------------------------------------------------------------------
def _flat_fields(st):
    """(name, is a pointer, value) of every field of a ctypes descriptor, arrays element by element"""
    if isinstance(st, _ext.CallDesc):
        entry = _PREFIX_ENTRY.get(int(st.fn)) or {v: k for k, v in _ext.CALL_FNS.items()}[int(st.fn)]
        types = _ext.SYMBOLS[entry][1][:-1]
        if int(st.fn) in _PREFIX_ENTRY:
            types = types[1:]                                            # (the descriptor is the op behind the prefix)
        yield "fn", False, int(st.fn)
        yield "n_args", False, int(st.n_args)
        for j in range(int(st.n_args)):
            yield f"a[{j}]", types[j] is C.c_void_p, int(st.a[j])
        return
    for name, ct in st._fields_:
        v = getattr(st, name)
        if isinstance(v, C.Array):
            for j in range(len(v)):
                yield f"{name}[{j}]", ct._type_ is C.c_void_p, v[j]
        else:
            yield name, ct is C.c_void_p, v


def _same_plan(plan_c, named_c, plan_g, named_g):
    diffs = []
    if plan_c["n"] != plan_g["n"]:
        return [f"op arrays differ in length: cpu {plan_c['n']}, device {plan_g['n']}"]
    for key in ("side", "final_gather", "patch_in", "patch_out", "out_buf", "n_part"):
        a, b = plan_c.get(key), plan_g.get(key)
        strip = lambda v: [tuple(e for e in g if not torch.is_tensor(e)) for g in v] if key == "side" else v    # noqa: E731
        if strip(a) != strip(b):
            diffs.append(f"plan[{key!r}] differs: cpu {strip(a)}, device {strip(b)}")
    for j in range(plan_c["n"]):
        oc, og = plan_c["arr"][j], plan_g["arr"][j]
        if oc.kind != og.kind:
            diffs.append(f"op {j}: kind cpu {oc.kind}, device {og.kind}")
            continue
        member = _MEMBER[int(oc.kind)]
        for (name, is_ptr, vc), (_, _, vg) in zip(_flat_fields(getattr(oc.u, member)), _flat_fields(getattr(og.u, member))):
            if not is_ptr:
                if vc != vg:
                    diffs.append(f"op {j} ({member}).{name}: cpu {vc}, device {vg}")
                continue
            vc, vg = int(vc or 0), int(vg or 0)
            if (vc == 0) != (vg == 0):
                diffs.append(f"op {j} ({member}).{name}: null on one side only (cpu {vc:#x}, device {vg:#x})")
            elif vc:
                rc, rg = _resolve(named_c, vc), _resolve(named_g, vg)
                if rc is None or rg is None or rc != rg:
                    diffs.append(f"op {j} ({member}).{name}: cpu -> {rc}, device -> {rg}")
    return diffs


# ---- A.2 / A.3: the same ops ---------------------------------------------------------------------------------------------------
def _steps(plan):
    """the launches of FlowEngine._execute_plain, one at a time"""
    arr, steps, pos = plan["arr"], [], 0

    def until(end):
        nonlocal pos
        while pos < end:
            n = 2 if _ext.is_ctx_prefix(arr[pos]) else 1
            steps.append(("ops", pos, n))
            pos += n
    for g in plan["side"]:
        until(g[1])
        steps.append(("side", g))
    until(plan["n"])
    if plan["final_gather"] is not None:
        steps.append(("final", plan["final_gather"]))
    return steps


def _describe(plan, step):
    """(label for the statistics and the coverage, rule, K): rule in exact / gemm / gated_norm / base_part"""
    if step[0] == "side":
        return ("side/scale", "gemm", 1) if step[1][0] == "scale" else ("side/gather", "exact", 0)
    if step[0] == "final":
        return "final_gather", "exact", 0
    op = plan["arr"][step[1]]
    if op.kind == _ext.OP_CALL:
        nxt = plan["arr"][step[1] + 1]
        if op.u.call.fn == _ext.FN_COUPLING_PLANES_CTX:
            return "call/coupling_planes_ctx", "gemm", max(32 * nxt.u.coupling_planes.nk_p, nxt.u.coupling_planes.hidden_padded)
        d = nxt.u.coupling
        return "call/coupling_vctx", "gemm", max([d.n_pass] + [d.hidden[j] for j in range(d.n_hidden)])
    if op.kind == _ext.OP_LINEAR:
        return ("linear+W_split" if op.u.linear.W_split else "linear"), "gemm", op.u.linear.K
    if op.kind == _ext.OP_COUPLING:
        d = op.u.coupling
        variant = {1: "exact-f32", 2: "bf16x3", 3: "tiny"}[_ext.load().usf_coupling_variant(C.byref(d))]
        return f"coupling/{variant}", "gemm", max([d.n_pass] + [d.hidden[j] for j in range(d.n_hidden)])
    if op.kind == _ext.OP_PACK_PLANES:
        d = op.u.pack_planes
        return ("pack_planes+prologue", "gemm", 1) if (d.pre_div or d.pre_sub) else ("pack_planes", "exact", 0)
    if op.kind == _ext.OP_GEMM_PLANES:
        d = op.u.gemm_planes
        if d.base_part:
            return "gemm_planes->base_part", "base_part", 32 * d.nk
        return ("gemm_planes->f32" if d.C_f32 else "gemm_planes->planes"), "gemm", 32 * d.nk
    if op.kind == _ext.OP_COUPLING_PLANES:
        d = op.u.coupling_planes
        return "coupling_planes", "gemm", max(32 * d.nk_p, d.hidden_padded)
    if op.kind == _ext.OP_GATED_NORM:
        return ("gated_norm+ln" if op.u.gated_norm.gamma else "gated_norm"), "gated_norm", 0
    raise AssertionError(f"op kind {op.kind}")


def _device_step(eng, plan, step, x, out):
    B, dev, ws = x.shape[0], x.device, plan["ws"]
    if step[0] == "ops":
        sub = C.cast(C.byref(plan["arr"], step[1] * C.sizeof(_ext.Op)), C.POINTER(_ext.Op))
        _ext.check(_ext.load().usf_run_ops(sub, step[2], _ext.current_stream(dev)), "usf_run_ops")
    elif step[0] == "side" and step[1][0] == "scale":
        _, _, buf, ld, sc, divide, ncols = step[1]
        _ext.scale(ws[buf], ld, ws[buf], ld, B, ncols, sc, divide)
    elif step[0] == "side":
        _, _, src, dst_name, dst_layout = step[1]
        src_t, dst_t = (x if src[0] == "user_in" else ws[src[0]]), ws[dst_name]
        _ext.gather_cols(src_t, src[2], dst_t, dst_t.shape[1], B, dst_t.shape[1], eng._gather_index(src[1], dst_layout, dev))
    else:
        src, dst_name = step[1]
        if dst_name == "user_out":
            _ext.gather_cols(ws[src[0]], src[2], out, eng.D, B, eng.D, eng._gather_index(src[1], "user", dev))
        else:
            _ext.gather_cols(ws[src[0]], src[2], ws[dst_name], eng.LDn, B, eng.LDn, eng._gather_index(src[1], "nat", dev))


def _emu_step(eng, plan, step, x, out, pm, dtype):
    if step[0] == "ops":
        took = emulator.emulate_launch(plan["arr"], step[1], plan["n"], pm, dtype)
        assert took == step[2], (took, step)
    elif step[0] == "side":
        emulator.emulate_side(eng, plan, step[1], x, dtype)
    else:
        emulator.emulate_final_gather(eng, plan, x, out)


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def _where(mask):
    idx = mask.flatten().nonzero().flatten()
    return f"elements [{int(idx[0])} .. {int(idx[-1])}] ({idx.numel()} of {mask.numel()})"


class _Acc:
    """what one step wrote, over all of its buffers: the largest entry, the device's and the fp32 emulator's worst error"""

    def __init__(self):
        self.wmax, self.err, self.err32, self.at = 0.0, 0.0, 0.0, ""
        self.rel_elem = 0.0            # the device's worst element-wise relative error, denominators clamped at 1e-3


def _cmp_values(label, pre, e64, e32, dev, exact, acc, fails):
    """the three rules of the comparison, element by element, on one buffer"""
    if not pre.is_floating_point():
        if not torch.equal(dev, e64):
            fails.append(f"{label}: {_where(dev != e64)} differ from the emulator (integer buffer)")
        return
    pb, rb, db = _bits(pre), _bits(e64), _bits(dev)
    keep = (pb == rb) | (torch.isnan(e64) & ~torch.isnan(pre))        # unchanged, or marked "never written"
    bad = keep & (db != pb)
    if bad.any():
        fails.append(f"{label}: {_where(bad)} changed on the device, the emulator leaves them alone")
    wrote = ~keep
    if not wrote.any():
        return
    if exact:
        bad = wrote & (db != rb)
        if bad.any():
            fails.append(f"{label}: {_where(bad)} not bit-equal to the emulator in an exact step")
        return
    fin = wrote & torch.isfinite(e64)
    odd = wrote & ~torch.isfinite(e64) & (db != rb)
    if odd.any():
        fails.append(f"{label}: {_where(odd)} the emulator wrote a non-finite value the device does not hold")
    if fin.any():
        zero = torch.zeros((), dtype=torch.float64)
        r = torch.where(fin, e64.double(), zero)                       # (elsewhere e64 may hold NaN: NaN * 0 is NaN)
        d = (dev.double() - r).abs()
        d = torch.where(fin, torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d), zero)
        acc.wmax = max(acc.wmax, float(r.abs().max()))
        if float(d.max()) > acc.err:
            acc.err, acc.at = float(d.max()), f"{label} element {int(d.flatten().argmax())}"
        d32 = torch.where(fin, (e32.double() - r).abs(), zero)
        acc.err32 = max(acc.err32, float(torch.where(torch.isnan(d32), torch.full_like(d32, float("inf")), d32).max()))
        acc.rel_elem = max(acc.rel_elem, float((d / r.abs().clamp_min(1e-3)).max()))


_PLANES_FIELDS = {_ext.OP_PACK_PLANES: (("planes", "nkb"),), _ext.OP_GEMM_PLANES: (("A", "a_nkb"), ("C_planes", "c_nkb")),
                  _ext.OP_COUPLING_PLANES: (("z", "z_nkb"),)}


def _planes_nkb(plan, named):
    """buffer name -> blocks per panel, as the plan's own descriptors give it for the buffers they point to (a workspace buffer
    may be larger than panels x blocks: engine_planes.planes_buf keeps a larger one of the same name)"""
    nkb = {}
    for j in range(plan["n"]):
        op = plan["arr"][j]
        d = getattr(op.u, _MEMBER[int(op.kind)])
        for ptr_f, nkb_f in _PLANES_FIELDS.get(int(op.kind), ()):
            hit = _resolve(named, int(getattr(d, ptr_f) or 0)) if getattr(d, ptr_f) else None
            if hit is not None and hit[1] == 0:
                assert nkb.setdefault(hit[0], int(getattr(d, nkb_f))) == int(getattr(d, nkb_f)), f"{hit[0]}: two block counts"
    return nkb


def _cmp_buffer(name, fmt, pre, e64, e32, dev, exact, acc, fails, rows=None, nkb=None):
    if pre.dtype != torch.uint8:
        return _cmp_values(name, pre, e64, e32, dev, exact, acc, fails)
    # a planes buffer: through planes_decode (every panel, every block: padding rows included), and raw per 1 KiB chunk
    npl, dt = (2, torch.float16) if fmt == 1 else (3, torch.bfloat16)
    used = pre.numel() if fmt == 0 else pre.numel() * 2 // 3               # (sized for either format: engine_planes.planes_buf)
    dec = lambda raw: emulator.planes_decode(raw[:used].view(dt).view(-1, 1, npl, 64, 8), used // (npl * 1024) * 16)   # noqa: E731
    dp, d64, d32, dd = dec(pre), dec(e64), dec(e32), dec(dev)
    if rows is not None and rows % 16:
        # EXCLUSIONS: the padding rows of the last panel (its blocks are the buffer's last nkb; 16 decoded rows per block)
        npan = -(-rows // 16)
        nblk = dp.shape[0] // 16
        nkb = nblk // npan if nkb is None else nkb                  # (the op descriptor's, where one names the buffer)
        blk, j = torch.arange(dp.shape[0]) // 16, torch.arange(dp.shape[0]) % 16
        pad = ((blk >= (npan - 1) * nkb) & (blk < npan * nkb) & (j >= rows - 16 * (npan - 1)))[:, None].expand_as(dp)
        d64, d32, dd = torch.where(pad, dp, d64), torch.where(pad, dp, d32), torch.where(pad, dp, dd)
    _cmp_values(f"{name} (decoded, [rows of 16-row panels x blocks, 32])", dp, d64, d32, dd, exact, acc, fails)
    te, td = (e64 != pre).view(-1, 1024).any(1), (dev != pre).view(-1, 1024).any(1)
    if (te != td).any():
        fails.append(f"{name}: 1 KiB chunks touched by the device only {(td & ~te).nonzero().flatten().tolist()[:8]}, "
                     f"by the emulator only {(te & ~td).nonzero().flatten().tolist()[:8]}")


def _bound(rule, K, acc, gamma=False):
    """the relative bound of a step (against the largest entry it wrote); no new tolerance:
    gemm        max(4 err32, 6e-8 sqrt(K))                    tests/test_kernels_gpu.py:147, tests/test_planes_gpu.py:221
    gated_norm  2e-6 max(1, |r|max) (x 4 with a layer norm)   tests/test_kernels_gpu.py:402
    base_part   2e-6, element-wise relative (_Acc.rel_elem)   tests/test_planes_gpu.py:323"""
    scale = acc.wmax if acc.wmax > 0 else 1.0
    if rule == "gemm":
        return max(4 * acc.err32 / scale, 6e-8 * math.sqrt(max(K, 1)))
    if rule == "gated_norm":
        return 2e-6 * max(1.0, scale) * (4 if gamma else 1) / scale
    if rule == "base_part":
        return 2e-6
    raise AssertionError(rule)


def _lockstep(tag, eng_c, plan_c, x_c, out_c, eng_g, plan_g, x_g, out_g, stats, visited):
    """every step of the plan on the device and in the emulator from identical bits; returns the failures"""
    named_c, named_g = _named_tensors(eng_c, plan_c, x_c, out_c), _named_tensors(eng_g, plan_g, x_g, out_g)
    fails = []
    if [n for n, _ in named_c] != [n for n, _ in named_g]:
        only = set(n for n, _ in named_c) ^ set(n for n, _ in named_g)
        return [f"{tag}: the two sides own different tensors: {sorted(only)[:10]}"]
    state = []                                                      # (name, cpu twin, device tensor): compared after every step
    for (n, tc), (_, tg) in zip(named_c, named_g):
        if tc.shape != tg.shape or tc.dtype != tg.dtype:
            fails.append(f"{tag}: {n} is {tuple(tc.shape)} {tc.dtype} on the cpu, {tuple(tg.shape)} {tg.dtype} on the device")
            continue
        if n.startswith("ws/") or n == "user_out":
            if tc.dtype == torch.uint8:                             # torch.empty planes buffers: zero-filled once on both sides
                tc.zero_(), tg.zero_()
            state.append((n, tc, tg))
        elif n != "user_in" and not torch.equal(tc, tg.cpu()):
            # the pack, the index vectors: the device's bits on both sides (what is equal already -- the parameters themselves --
            # is left alone: a write would bump the parameter's version and with it the CPU engine's pack)
            tc.copy_(tg)
    if fails:
        return fails
    fails += [f"{tag}: {d}" for d in _same_plan(plan_c, named_c, plan_g, named_g)]
    if fails:
        return fails
    pm = _ptr_map(named_c)
    fmt = plan_g.get("planes_fmt", 0)
    nkb_of = _planes_nkb(plan_g, named_g)
    for k, step in enumerate(_steps(plan_g)):
        label, rule, K = _describe(plan_g, step)
        visited.add(label)
        where = f"{tag} step {k} ({label}" + (f", op {step[1]}" if step[0] == "ops" else "") + ")"
        torch.cuda.synchronize()
        pre = {n: tg.detach().cpu().clone() for n, _, tg in state}
        for n, tc, _ in state:
            tc.copy_(pre[n])
        _device_step(eng_g, plan_g, step, x_g, out_g)
        torch.cuda.synchronize()
        post_g = {n: tg.detach().cpu() for n, _, tg in state}
        _emu_step(eng_c, plan_c, step, x_c, out_c, pm, torch.float64)
        post64 = {n: tc.clone() for n, tc, _ in state}
        for n, tc, _ in state:
            tc.copy_(pre[n])
        _emu_step(eng_c, plan_c, step, x_c, out_c, pm, torch.float32)
        acc, sfails = _Acc(), []
        for n, tc, _ in state:
            _cmp_buffer(f"buffer {n}", fmt, pre[n], post64[n], tc, post_g[n], rule == "exact", acc, sfails, rows=x_g.shape[0],
                        nkb=nkb_of.get(n))
        if rule != "exact" and acc.wmax > 0:
            gamma = step[0] == "ops" and plan_g["arr"][step[1]].kind == _ext.OP_GATED_NORM and bool(plan_g["arr"][step[1]].u.gated_norm.gamma)
            scale = acc.wmax
            bound = _bound(rule, K, acc, gamma)
            err = acc.rel_elem if rule == "base_part" else acc.err / scale
            stats[label] = max(stats.get(label, 0.0), err / bound)
            if not err < bound:
                sfails.append(f"error {err:.3e} (fp32 emulator {acc.err32 / scale:.3e}) not below {bound:.3e}, worst at {acc.at}")
        elif rule == "exact":
            stats.setdefault(label, 0.0)
        fails += [f"{where}: {f}" for f in sfails]
    return fails


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def _golden(name):
    spec, sd, a = load_case(name)
    return spec, sd, a["x"], a["zin"], a.get("context")


def _vctx(name):
    x, zin, ctx = vctx_cases.inputs(name)
    return vctx_cases.spec_of(name), vctx_cases.state_dict_of(name), x, zin, ctx


def _wide(dim, hidden):
    """no golden case has a hidden width in (128, 256]: the shape the fused bf16x3 coupling kernel needs (with >= 1024 rows).
    The nearest stand-in: the documented synthetic generator at the smallest such flow"""
    spec = orc.FlowSpec(dim, 1, hidden, householder=0)
    g = torch.Generator().manual_seed(dim)
    return spec, orc.synth_state_dict(spec, seed=3), torch.rand(48, dim, generator=g), torch.randn(48, dim, generator=g), None


# id -> (loader, loader argument, fused, planes, base density in the epilogue too, rows, directions)
BOTH = ("backward", "forward")
CASES = {
    "d7_conj-unfused": (_golden, "synth_d7_k3_hh1_conj_normal", False, False, False, ROWS, BOTH),
    "d7_conj-fused": (_golden, "synth_d7_k3_hh1_conj_normal", True, False, False, ROWS, BOTH),
    "d33-unfused": (_golden, "synth_d33_k3_lu2_hh1", False, False, False, ROWS, BOTH),
    "d33-fused": (_golden, "synth_d33_k3_lu2_hh1", True, False, False, ROWS, BOTH),
    "d33-planes-bf16x3-unfused": (_golden, "synth_d33_k3_lu2_hh1", False, "bf16x3", True, ROWS, BOTH),
    "d33-planes-bf16x3-fused": (_golden, "synth_d33_k3_lu2_hh1", True, "bf16x3", True, ROWS, BOTH),
    "d33-planes-f16x2-unfused": (_golden, "synth_d33_k3_lu2_hh1", False, "f16x2", True, ROWS, BOTH),
    "d33-planes-f16x2-fused": (_golden, "synth_d33_k3_lu2_hh1", True, "f16x2", True, ROWS, BOTH),
    "d16_gated_ln": (_golden, "synth_d16_k3_convnet_gated_ln", False, False, False, ROWS, BOTH),
    "d7_soft_ctx-fused": (_golden, "synth_d7_k3_soft_ctx", True, False, False, ROWS, BOTH),
    "d7_soft_ctx-unfused": (_golden, "synth_d7_k3_soft_ctx", False, False, False, ROWS, BOTH),
    "d7_soft_ctx-planes-bf16x3": (_golden, "synth_d7_k3_soft_ctx", True, "bf16x3", True, ROWS, BOTH),
    "d7_soft_ctx-planes-f16x2": (_golden, "synth_d7_k3_soft_ctx", True, "f16x2", True, ROWS, BOTH),
    "vctx_d7_k3-fused": (_vctx, "d7_k3", True, False, False, ROWS, BOTH),
    "vctx_d7_k3-unfused": (_vctx, "d7_k3", False, False, False, ROWS, BOTH),
    "vctx_d33_k2-fused": (_vctx, "d33_k2", True, False, False, ROWS, BOTH),
    # the op kinds the cases above do not reach at 37 rows (one direction, one row count each):
    "d64_k6-fused": (_golden, "synth_d64_k6_hh0_laplace", True, False, False, (37,), ("backward",)),      # exact-f32 coupling kernel
    "d64_k6-unfused": (_golden, "synth_d64_k6_hh0_laplace", False, False, False, (37,), ("backward",)),   # usf_linear_f32 with W_split
    "wide160-fused": (_wide, (33, [160]), True, False, False, (1029,), ("backward",)),                    # bf16x3 coupling kernel
}
REQUIRED = {"linear", "linear+W_split", "coupling/exact-f32", "coupling/bf16x3", "coupling/tiny", "pack_planes",
            "gemm_planes->planes", "gemm_planes->f32", "gemm_planes->base_part", "coupling_planes", "gated_norm", "gated_norm+ln",
            "call/coupling_planes_ctx", "call/coupling_vctx"}
_RESULTS = {}          # case id -> (failures, worst ratio per step label, labels visited, log lines)


def _switches(eng, fused, planes):
    """as emulator.engine_transform sets them (the library's own _fused_ok stays: it answers the same on both sides)"""
    eng.use_fused_coupling, eng.fused_min_rows = fused, 0
    eng.use_planes, eng.planes_min_rows = bool(planes), 0
    if planes:
        eng.gemm_mode = planes


def _tile(t, B, shift=0):
    return None if t is None else t[(torch.arange(B) + shift) % t.shape[0]].contiguous()


def _result_tensors(plan, out):
    ws = plan["ws"]
    res = [out] if out is not None else [ws["bpart"][:, : plan["n_part"]]]
    return res + ([ws["pflag"]] if "pflag" in ws else [])


def _run_case(cid):
    if cid in _RESULTS:
        return _RESULTS[cid]
    loader, arg, fused, planes, with_base, rows, directions = CASES[cid]
    spec, sd, x0, zin0, ctx0 = loader(*arg) if isinstance(arg, tuple) else loader(arg)
    fails, stats, visited, log = [], {}, set(), []
    with _cpu_prep():
        flow_c = build_flow(spec, sd)
        eng_c = FlowEngine(flow_c.layers)
    flow_g = build_flow(spec, sd, device=DEV)
    eng_g = FlowEngine(flow_g.layers)
    eng_f = [FlowEngine(flow_g.layers), FlowEngine(flow_g.layers)]            # a fresh plan per batch for the reuse check
    for e in [eng_c, eng_g] + eng_f:
        _switches(e, fused, planes)
    info = flow_c._base_info(torch.device("cpu")) if with_base else None
    forms = [(d, "user") for d in directions]
    if info is not None and info[0] in ("laplace", "normal"):
        forms.append(("backward", "base%d" % (_ext.BASE_LAPLACE if info[0] == "laplace" else _ext.BASE_NORMAL)))
    for B in rows:
        for direction, final in forms:
            tag = f"{cid} {direction} B={B} final={final}"
            src = x0 if direction == "backward" else zin0
            batches = [(_tile(src, B, s), _tile(ctx0, B, s)) for s in (0, 5)]
            has_ctx = ctx0 is not None
            with _cpu_prep():
                plan_c = eng_c._plan(direction, B, torch.device("cpu"), has_ctx, final)
            plan_g = eng_g._plan(direction, B, torch.device(DEV), has_ctx, final)
            plan_f = [e._plan(direction, B, torch.device(DEV), has_ctx, final) for e in eng_f]
            g = torch.Generator().manual_seed(B)
            out_c = torch.randn(B, eng_c.D, generator=g) if final == "user" else None
            out_g = out_c.to(DEV) if out_c is not None else None
            if final.startswith("base"):
                loc, scale = info[1].to(DEV), info[2].to(DEV)
                for p in [plan_g] + plan_f:
                    _ext.base_tables(int(final[4:]), loc, scale, eng_g.D, p["ws"]["btab"], p["ws"]["btab"].numel() // 3)
            # the first whole-plan run of each batch, on a fresh plan of its own: what a reused plan has to reproduce bit for bit
            fresh = []
            for (xb, cb), ef, pf in zip(batches, eng_f, plan_f):
                o = torch.empty(B, ef.D, device=DEV) if final == "user" else None
                ef._execute_plain(pf, xb.to(DEV), o, None if cb is None else cb.to(DEV))
                torch.cuda.synchronize()
                fresh.append([t.clone() for t in _result_tensors(pf, o)])
            x_c, c_c = batches[0]
            x_g = x_c.to(DEV)
            emulator.patch_user_pointers(plan_c, x_c, out_c)
            emulator.patch_user_pointers(plan_g, x_g, out_g)
            if has_ctx:
                eng_g._fill_context(plan_g, c_c.to(DEV), B)
            f = _lockstep(tag, eng_c, plan_c, x_c, out_c, eng_g, plan_g, x_g, out_g, stats, visited)
            fails += f
            # reuse: the stepped plan runs another batch, then the first one again
            for which in (1, 0):
                xb, cb = batches[which]
                eng_g._execute_plain(plan_g, xb.to(DEV), out_g, None if cb is None else cb.to(DEV))
                torch.cuda.synchronize()
                for got, want in zip(_result_tensors(plan_g, out_g), fresh[which]):
                    if not torch.equal(got, want):
                        fails.append(f"{tag}: a reused plan gives other bits than a fresh one for batch {which}: {_where(got != want)}")
            log.append(f"{tag}: {len(_steps(plan_g))} steps, {len(f)} failures")
    _RESULTS[cid] = (fails, stats, visited, log)
    return _RESULTS[cid]


def _report(stats):
    return "\n".join(f"    {k:28s} worst error / bound {v:.3f}" for k, v in sorted(stats.items()))


@pytest.mark.parametrize("cid", list(CASES))
def test_plan_in_lockstep(cid):
    """A: the case's plans are the same on both sides, every step agrees with the emulator under the three rules and the
    kernel tests' bounds, and a reused plan reproduces a fresh one bit for bit"""
    fails, stats, _, log = _run_case(cid)
    print("\n".join(log))
    print(_report(stats))
    assert not fails, f"{len(fails)} disagreements:\n" + "\n".join(fails[:40])


def test_every_op_kind_the_engine_emits_was_stepped():
    """A.5: the union of the steps visited over all cases holds every kind of launch the engine can put into a plan"""
    visited, stats = set(), {}
    for cid in CASES:
        _, s, v, _ = _run_case(cid)
        visited |= v
        for k, r in s.items():
            stats[k] = max(stats.get(k, 0.0), r)
    print("worst observed error / bound per kind of step, all cases:\n" + _report(stats))
    assert REQUIRED <= visited, f"never stepped: {sorted(REQUIRED - visited)}"


# ---- C: refusals ---------------------------------------------------------------------------------------------------------------
def _refused(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except Exception:
        return True
    return False


def test_the_emulator_refuses_what_the_library_refuses():
    """the argument sets of test_linear_rejects_bad_args, test_gated_norm_rows_rejects_bad_args, test_gemm_planes_rejects_bad_args
    and test_planes_entry_points_reject_what_they_cannot_serve (those with an emulated counterpart), handed to both sides: host-side
    validation refuses them before any launch, and so does the emulation"""
    sets = []
    A, W, Cm = torch.zeros(4, 6), torch.zeros(4, 6), torch.zeros(4, 4)
    sets.append(("linear: K % 4 != 0", "linear", (A, W, Cm), dict(M=4, N=4, K=6, lda=6, ldw=6, ldc=4)))
    x = torch.zeros(4, 8)
    sets.append(("gated_norm_rows: no output", "gated_norm_rows", (x,), dict(M=4, C_cols=8, ld_skip=8)))
    sets.append(("gated_norm_rows: stride shorter than the row", "gated_norm_rows", (x,), dict(M=4, C_cols=8, ld_skip=4, out=x, ld_out=8)))
    sets.append(("gated_norm_rows: gamma without beta", "gated_norm_rows", (x,), dict(M=4, C_cols=8, ld_skip=8, out=x, ld_out=8, gamma=x)))
    sets.append(("gated_norm_rows: C > 4096", "gated_norm_rows", (x,), dict(M=4, C_cols=5000, c_pad=5000, ld_skip=5000, out=x, ld_out=5000)))
    Ap = torch.zeros(_ext.planes_bytes(64, 2), dtype=torch.uint8)
    Wp = torch.zeros(3, 32, 64, dtype=torch.bfloat16)
    sets.append(("gemm_planes: K range past the buffer", "gemm_planes", (Ap, Wp), dict(M=64, a_nkb=2, a_kb0=1, nk=2, C_planes=Ap, c_nkb=2, c_kbn=1)))
    sets.append(("gemm_planes: no output", "gemm_planes", (Ap, Wp), dict(M=64, a_nkb=2, nk=2)))
    N = K = 256
    A32, Y32, G = torch.zeros(4096, K), torch.zeros(4096, N), torch.zeros(N, K)
    sets.append(("wgrad: column sums where no instantiation carries them", "wgrad", (Y32, A32, G),
                 dict(M=1024, N=N, K=K, ldy=N, lda=K, ldg=K, mode=1, colsum=torch.zeros(N))))
    emu = dict(linear=emulator._emu_linear, gated_norm_rows=emulator._emu_gated_norm_rows, gemm_planes=emulator._emu_gemm_planes_call,
               wgrad=emulator._emu_wgrad)
    dev = lambda v: v.to(DEV) if torch.is_tensor(v) else v      # noqa: E731
    lenient = []
    for what, name, args, kw in sets:
        with pytest.raises((RuntimeError, ValueError)):
            getattr(_ext, name)(*[dev(a) for a in args], **{k: dev(v) for k, v in kw.items()})
        if not _refused(emu[name], *args, **kw):
            lenient.append(what)
    assert not lenient, f"the emulator accepts what the library refuses: {lenient}"


# ---- B: the direct-call emulations ---------------------------------------------------------------------------------------------
def _map(obj, fn, memo):
    """obj with every tensor replaced by fn(tensor); one tensor object maps to one copy (aliases stay aliases)"""
    if torch.is_tensor(obj):
        if id(obj) not in memo:
            memo[id(obj)] = fn(obj)
        return memo[id(obj)]
    if isinstance(obj, (list, tuple)):
        return type(obj)(_map(v, fn, memo) for v in obj)
    if isinstance(obj, dict):
        return {k: _map(v, fn, memo) for k, v in obj.items()}
    return obj


def _direct(what, name, emu, args, kw, rule="gemm", K=1, tol=None, dtype_kw=True, batch=False, rows=None, call=None, emu_call=None,
            scratch=(), unspecified=(), gamma=False):
    """_ext.<name> on device copies of the arguments, the emulation on CPU clones (dtype=fp64: the reference; fp32: the yardstick),
    then EVERY tensor argument compared in full under the rules of part A -- inputs and gaps must come back untouched.
    rule: exact | gemm (K: the inner dimension) | gated_norm (_bound) | rel (tol x the largest entry written) | elem (tol,
    element-wise relative with the denominator clamped at 1e-3) | abs (tol).  dtype_kw: the emulation takes dtype= (the fp32
    entry points; the fp64 and the exact ones have one precision).  batch: inside a batch_jobs(defer_grads=True) block, flushed
    by the binding's own flush / the emulation's.  call / emu_call: what to run in place of the plain call (a queue and its
    flush).  gamma: the gated_norm rule with a layer norm.  rows: M of the planes buffers among the arguments.  scratch: tensors left out; unspecified: (tensor, mask) left out
    where the mask holds, and finite on the device there -- both only for what EXCLUSIONS lists."""
    mg, m64, m32 = {}, {}, {}
    ag, kg = _map(args, lambda t: t.to(DEV), mg), _map(kw, lambda t: t.to(DEV), mg)
    a64, k64 = _map(args, lambda t: t.clone(), m64), _map(kw, lambda t: t.clone(), m64)
    a32, k32 = _map(args, lambda t: t.clone(), m32), _map(kw, lambda t: t.clone(), m32)
    pre = [t.clone() for t in m64.values()]
    dev_fn = call or getattr(_ext, name)
    if batch:
        with _ext.batch_jobs(torch.device(DEV), defer_grads=True):
            dev_fn(*ag, **kg)
    else:
        dev_fn(*ag, **kg)
    torch.cuda.synchronize()
    emu_fn = emu_call or emu
    for dt, a, k in ((torch.float64, a64, k64), (torch.float32, a32, k32)):
        extra = dict(dtype=dt) if dtype_kw else {}
        if batch:
            with _ext.batch_jobs(torch.device("cpu"), defer_grads=True) as bj:
                emu_fn(*a, **k, **extra)
                assert bj.grad_jobs or bj.jobs, f"{what}: the emulation did not queue the job"
                emulator._emu_flush(bj)
        else:
            emu_fn(*a, **k, **extra)
    skip = {id(t) for t in scratch}
    masks = {id(t): m for t, m in unspecified}
    acc, fails = _Acc(), []
    for i, (key, p, t64, t32, tg) in enumerate(zip(m64, pre, m64.values(), m32.values(), mg.values())):
        if key in skip:
            continue
        got = tg.cpu()
        if key in masks:
            m = masks[key]
            if not torch.isfinite(got[m].float()).all():
                fails.append(f"tensor argument {i}: non-finite values in the region the header leaves open")
            got, t64, t32 = torch.where(m, p, got), torch.where(m, p, t64), torch.where(m, p, t32)
        _cmp_buffer(f"tensor argument {i} {tuple(p.shape)} {p.dtype}", 0, p, t64, t32, got, rule == "exact", acc, fails, rows=rows)
    if rule != "exact" and acc.wmax > 0:
        scale = acc.wmax
        if rule in ("gemm", "gated_norm"):
            err, bound = acc.err / scale, _bound(rule, K, acc, gamma)
        elif rule == "rel":
            err, bound = acc.err / scale, tol
        elif rule == "elem":
            err, bound = acc.rel_elem, tol
        else:
            err, bound = acc.err, tol
        _STATS_B[name] = max(_STATS_B.get(name, 0.0), err / bound)
        print(f"{what}: error {err:.3e}, bound {bound:.3e} (fp32 emulation {acc.err32 / scale:.3e})")
        if not err < bound:
            fails.append(f"error {err:.3e} not below {bound:.3e}, worst at {acc.at}")
    assert not fails, f"{what}:\n" + "\n".join(fails)


_STATS_B = {}
MS = (1, 37)


def _rnd(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


@pytest.mark.parametrize("M", MS)
def test_direct_linear(M):
    """_ext.linear as the training path calls it: padded strides and element offsets, every epilogue, the gate epilogue
    (usf_act_grad_f32 of the plain product) and the input's planes as a side output"""
    g = torch.Generator().manual_seed(M)
    N, K, lda, ldw, ldc, ldr = 20, 24, 32, 28, 28, 24
    A, W, Cm, R = _rnd(g, M + 1, lda), _rnd(g, N, ldw, scale=0.3), _rnd(g, M + 1, ldc), _rnd(g, M + 1, ldr)
    vec = lambda n: 0.5 + torch.rand(n, generator=g)      # noqa: E731
    dims = dict(M=M, N=N, K=K, lda=lda, ldw=ldw, ldc=ldc)
    _direct("bias + LeakyReLU, offsets", "linear", emulator._emu_linear, (A, W, Cm),
            dict(dims, bias=vec(N), act=_ext.ACT_LEAKY_RELU, slope=0.01, a_off=4, c_off=8), K=K)
    _direct("prologue + residual + post_mul", "linear", emulator._emu_linear, (A, W, Cm),
            dict(dims, pre_div=vec(K), pre_sub=vec(K), bias=vec(N), residual=R, ldr=ldr, r_off=4, res_sign=-1.0, post_mul=vec(N)),
            K=K)
    _direct("addend", "linear", emulator._emu_linear, (A, W, Cm), dict(dims, bias=vec(N), addend=R, ldadd=ldr, act=_ext.ACT_LEAKY_RELU,
                                                                      slope=0.2), K=K)
    _direct("gate epilogue", "linear", emulator._emu_linear, (A, W, Cm), dict(dims, addend=R, ldadd=ldr, act=_ext.ACT_GATE, slope=0.01),
            K=K)
    P = _rnd(g, 3, -(-M // 32) * 32, 32).to(torch.bfloat16)
    _direct("planes_out", "linear", emulator._emu_linear, (A, W, Cm), dict(dims, bias=vec(N), planes_out=P), K=K)


@pytest.mark.parametrize("M", MS)
def test_direct_weight_gradients_and_column_sums(M):
    """usf_wgrad_f32 / usf_colsum_f32: alpha and beta both at work, offsets, padded strides; launched directly and as queued jobs
    of one usf_grad_jobs_f32 launch; inner dimension M"""
    g = torch.Generator().manual_seed(10 + M)
    N, K, ldy, lda, ldg = 12, 20, 16, 24, 28
    Y, A, G = _rnd(g, M + 1, ldy), _rnd(g, M + 1, lda), _rnd(g, N + 1, ldg)
    kw = dict(M=M, N=N, K=K, ldy=ldy, lda=lda, ldg=ldg, y_off=4, a_off=4, g_off=ldg, alpha=0.5, beta=-1.5)
    for mode in (0, 1):
        _direct(f"wgrad mode {mode}", "wgrad", emulator._emu_wgrad, (Y, A, G), dict(kw, mode=mode, defer=False), K=M)
    _direct("wgrad beta = 0", "wgrad", emulator._emu_wgrad, (Y, A, G), dict(kw, beta=0.0, defer=False), K=M)
    _direct("wgrad queued", "wgrad", emulator._emu_wgrad, (Y, A, G), kw, K=M, batch=True)
    out = _rnd(g, N + 3)
    ck = dict(M=M, N=N, ldy=ldy, y_off=4, alpha=-0.5, beta=2.5)
    _direct("colsum", "colsum", emulator._emu_colsum, (Y, out), ck, K=M)
    _direct("colsum beta = 0", "colsum", emulator._emu_colsum, (Y, out), dict(ck, beta=0.0), K=M)
    _direct("colsum queued", "colsum", emulator._emu_colsum, (Y, out), ck, K=M, batch=True)


@pytest.mark.parametrize("M", MS)
def test_direct_elementwise(M):
    """usf_act_grad_f32 and add_rows (usf_masked_residual_f32 with a mask of ones): exact.  _ext.add_rows(x, t, ones) takes dense
    [M, ld] buffers and nothing else -- the row stride IS the width, there is no offset, alpha or beta: no gap to leave alone"""
    g = torch.Generator().manual_seed(20 + M)
    d, h = _rnd(g, M, 28), _rnd(g, M, 24)
    _direct("act_grad", "act_grad", emulator._emu_act_grad, (d, h), dict(M=M, H=18, ldd=28, ldh=24, act=_ext.ACT_LEAKY_RELU, slope=0.01),
            rule="exact", dtype_kw=False)
    _direct("act_grad, no activation", "act_grad", emulator._emu_act_grad, (d, h), dict(M=M, H=18, ldd=28, ldh=24, act=_ext.ACT_NONE, slope=0.0),
            rule="exact", dtype_kw=False)
    _direct("add_rows", "add_rows", emulator._emu_add_rows, (_rnd(g, M, 24), _rnd(g, M, 24), torch.ones(24)), {}, rule="exact", dtype_kw=False)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("gated,norm", [(True, True), (False, True), (True, False)])
def test_direct_gated_norm_rows(M, gated, norm):
    """usf_gated_norm_rows_f32 (bound: tests/test_kernels_gpu.py:402) and its backward twin (tests/test_train_kernels_gpu.py:388:
    2e-5 of the largest entry), C no multiple of 4, strides beyond c_pad"""
    g = torch.Generator().manual_seed(30 + M)
    Cn, cp = 18, 20
    ld, ldv = cp + 8, 2 * cp + 12
    skip, vg, dy = _rnd(g, M, ld), (_rnd(g, M, ldv) if gated else None), _rnd(g, M, ld)
    gamma, beta = ((0.5 + torch.rand(Cn, generator=g), _rnd(g, Cn)) if norm else (None, None))
    out, out_act = _rnd(g, M, ld), _rnd(g, M, ld)
    _direct("gated_norm_rows", "gated_norm_rows", emulator._emu_gated_norm_rows, (skip,),
            dict(M=M, C_cols=Cn, c_pad=cp, ld_skip=ld, vg=vg, ld_vg=ldv, gate_off=cp, gamma=gamma, beta=beta, eps=1e-5, out=out, ld_out=ld,
                 out_act=out_act, ld_act=ld, act=_ext.ACT_LEAKY_RELU, slope=0.01), rule="gated_norm",
            gamma=norm)
    d_skip, d_vg, dy_xh = _rnd(g, M, ld), (_rnd(g, M, ldv) if gated else None), (_rnd(g, M, ld) if norm else None)
    _direct("gated_norm_rows_bwd", "gated_norm_rows_bwd", emulator._emu_gated_norm_rows_bwd, (skip, dy, d_skip),
            dict(M=M, C_cols=Cn, c_pad=cp, ld_skip=ld, ld_dy=ld, ld_d_skip=ld, vg=vg, ld_vg=ldv, gate_off=cp, d_vg=d_vg, ld_d_vg=ldv, gamma=gamma,
                 eps=1e-5, dy_xh=dy_xh, ld_dy_xh=ld), rule="rel", tol=2e-5)


@pytest.mark.parametrize("M", MS)
def test_direct_base_density(M):
    """usf_base_logprob_f32 for every base id (bound: tests/test_kernels_gpu.py:230, 2e-6 element-wise) with and without the
    fp64 accumulators and the device log-det; the tables, the gradient (tests/test_train_kernels_gpu.py:134: 1e-6 of the
    largest entry) and the parameter gradient (a sum over M rows: the column sums' bound)"""
    g = torch.Generator().manual_seed(40 + M)
    D, ldz = 33, 36
    z, loc, sc = _rnd(g, M, ldz, scale=2.0), _rnd(g, D), 0.5 + torch.rand(D, generator=g)
    out = _rnd(g, M + 2)
    for base in (_ext.BASE_LAPLACE, _ext.BASE_NORMAL, _ext.BASE_LPNORM1, _ext.BASE_LPNORM2, _ext.BASE_LPNORMINF, _ext.BASE_ROWSUM):
        lp = base in (_ext.BASE_LPNORM1, _ext.BASE_LPNORM2, _ext.BASE_LPNORMINF)
        row = base == _ext.BASE_ROWSUM
        a = (z, ldz, M, D if not row else 5, base, None if row else loc, None if (row or lp) else sc, -3.25, out)
        _direct(f"base_logprob {base}", "base_logprob", emulator._emu_base_logprob, a, {}, rule="elem", tol=2e-6)
        # (every id with the accumulators and the device scalar: the LPNORM* kernels add no constant, device scalar included)
        _direct(f"base_logprob {base} + sums + device log-det", "base_logprob", emulator._emu_base_logprob, a,
                dict(sum_out=torch.tensor([1.5, 2.0], dtype=torch.float64), logdet_dev=torch.tensor(0.75, dtype=torch.float64)),
                rule="elem", tol=2e-6)
    for base in (_ext.BASE_LAPLACE, _ext.BASE_NORMAL):
        _direct(f"base_tables {base}", "base_tables", emulator._emu_base_tables, (base, loc, sc, D, _rnd(g, 3 * ldz), ldz), {},
                rule="elem", tol=2e-6, dtype_kw=False)
        _direct(f"base_param_grad {base}", "base_param_grad", emulator._emu_base_param_grad,
                (z, ldz, _rnd(g, M), M, D, base, loc, sc, _rnd(g, 2, D)), {}, K=M)
    g_lp = _rnd(g, M)
    for base in (_ext.BASE_LAPLACE, _ext.BASE_NORMAL, _ext.BASE_LPNORM1, _ext.BASE_LPNORM2, _ext.BASE_LPNORMINF):
        # (the LPNORM* ids take the rows' radii in `scale`, as the forward kernel leaves them: include/usflows_hip_internal.h)
        p = {_ext.BASE_LPNORM1: 1.0, _ext.BASE_LPNORM2: 2.0, _ext.BASE_LPNORMINF: float("inf")}.get(base)
        s_arg = sc if p is None else (z[:, :D] - loc).norm(p=p, dim=1)
        _direct(f"base_logprob_grad {base}", "base_logprob_grad", emulator._emu_base_logprob_grad,
                (z, ldz, g_lp, M, D, base, loc, s_arg, _rnd(g, M, ldz), ldz), {}, rule="rel", tol=1e-6)


@pytest.mark.parametrize("M", MS)
def test_direct_fp64_products(M):
    """usf_gemm_f64 with transposes, a batch, strides, offsets, alpha and beta (bound: tests/test_prep_gpu.py:98), matmul_f64,
    usf_matvec_f64 (:235: 1e-13, the fp32 copy the rounded fp64 one), usf_householder_f64 (:144: 1e-13)"""
    g = torch.Generator().manual_seed(50 + M)
    N, K, nb = 9, 13, 3
    f64 = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    for tA, tB in ((False, False), (True, False), (False, True), (True, True)):
        lda, ldb, ldc = (M if tA else K) + 3, (K if tB else N) + 2, N + 5
        sa, sb, sc_ = (K if tA else M) * lda + 7, (N if tB else K) * ldb + 5, M * ldc + 3
        A, B, Cm = f64(nb * sa + 4), f64(nb * sb + 4), f64(nb * sc_ + 4)
        _direct(f"gemm_f64 transA={tA} transB={tB}", "gemm_f64", emulator._emu_gemm_f64, (A, B, Cm),
                dict(M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, transA=tA, transB=tB, batch=nb, strideA=sa, strideB=sb, strideC=sc_,
                     alpha=0.5, beta=-1.5, a_off=2, b_off=3, c_off=1), rule="abs", tol=1e-12 * max(1.0, K), dtype_kw=False)
        _direct(f"gemm_f64 beta = 0 transA={tA} transB={tB}", "gemm_f64", emulator._emu_gemm_f64, (A, B, Cm),
                dict(M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, transA=tA, transB=tB, alpha=1.0, beta=0.0), rule="abs", tol=1e-12 * max(1.0, K), dtype_kw=False)
    for tA, tB in ((False, False), (True, True)):
        A, B = (f64(K, M) if tA else f64(M, K)), (f64(N, K) if tB else f64(K, N))
        got = _ext.matmul_f64(A.to(DEV), B.to(DEV), transA=tA, transB=tB).cpu()
        ref = emulator._emu_matmul_f64(A, B, transA=tA, transB=tB)
        assert got.shape == ref.shape and (got - ref).abs().max().item() <= 1e-12 * max(1.0, K)
    src, b, idx = f64(M + 2, K), f64(K), torch.tensor(([M, -1, 0] + list(range(M)))[: M + 1], dtype=torch.int32)
    _direct("matvec_f64", "matvec_f64", emulator._emu_matvec_f64, (src, b),
            dict(idx=idx, n_out=M + 1, alpha=-0.5, out32=_rnd(g, M + 1), out64=f64(M + 1)), rule="abs", tol=1e-13, dtype_kw=False)
    D = 7
    _direct("householder", "householder", emulator._emu_householder, (f64(D, D).float(), f64(2, D).float()), dict(out=f64(D, D)),
            rule="abs", tol=1e-13, dtype_kw=False)


def test_direct_lu_prepare_and_gradient_finish():
    """usf_lu_prepare_f64 (bounds: tests/test_prep_gpu.py:45-51) and usf_lu_grad_finish_f64 (:301: the torch formulation, bit-equal)"""
    g = torch.Generator().manual_seed(60)
    n, D = 3, 9
    Ls = [torch.eye(D) + 0.3 * _rnd(g, D, D).tril(-1) for _ in range(n)]
    Us = [(torch.eye(D) * (0.5 + torch.rand(D, generator=g)) + 0.3 * _rnd(g, D, D).triu(1)).contiguous() for _ in range(n)]
    got = _ext.lu_prepare([t.to(DEV) for t in Ls], [t.to(DEV) for t in Us], keep_factors=True)
    ref = emulator._emu_lu_prepare(Ls, Us, keep_factors=True)
    assert set(got) == set(ref)
    for key, tol in (("M", 1e-12), ("Minv", 1e-10), ("ladj", 1e-11 * D), ("tri", 0.0), ("tri_inv", 1e-10)):
        a, b = got[key].cpu(), ref[key]
        assert a.shape == b.shape and a.dtype == b.dtype, key
        assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item()), key
    f64 = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    for with_t in (True, False):
        dL, dU, TL, TU, c, tri = f64(n, D, D), f64(n, D, D), (f64(n, D, D) if with_t else None), (f64(n, D, D) if with_t else None), f64(n), ref["tri"]
        _direct("lu_grad_finish", "lu_grad_finish", emulator._emu_lu_grad_finish, (dL, dU, TL, TU, c, tri, n, D, _rnd(g, n * D * D + 4), _rnd(g, n * D * D + 4)),
                {}, rule="exact", dtype_kw=False)


@pytest.mark.parametrize("M", MS)
def test_direct_planes_entry_points(M):
    """the planes entry points the planes training step calls directly: usf_pack_planes_f32 with the base gradient on the way in,
    usf_gemm_planes_bf16x3 in the subset the emulation accepts (a K sub-range, an output sub-range), usf_wgrad_blocked_f32 with
    alpha and beta, with the column sums (cs_alpha, cs_beta) accumulated and overwritten, and with its reduction queued and
    flushed (inner dimension M)"""
    g = torch.Generator().manual_seed(70 + M)
    D, nkb = 40, 2
    idx = torch.full((32 * nkb,), -1, dtype=torch.int32)
    idx[:D] = torch.randperm(D, generator=g).to(torch.int32)
    src, w = _rnd(g, M, D + 4), _rnd(g, M)
    loc, sc = _rnd(g, D), 0.5 + torch.rand(D, generator=g)
    planes = torch.randint(0, 255, (_ext.planes_bytes(M, nkb),), generator=g, dtype=torch.uint8)
    for base in (_ext.BASE_LAPLACE, _ext.BASE_NORMAL):
        _direct(f"pack_planes grad base {base}", "pack_planes", emulator._emu_pack_planes_call, (src, planes),
                dict(M=M, nkb=nkb, idx=idx, ld=D + 4, src_cols=D, grad=(base, w, loc, sc)), K=1, rows=M, dtype_kw=False)
    _direct("pack_planes plain", "pack_planes", emulator._emu_pack_planes_call, (src, planes), dict(M=M, nkb=nkb, idx=idx, ld=D + 4, src_cols=D),
            rule="exact", rows=M, dtype_kw=False)
    # a GEMM on planes: K range blocks 1 .. 2 of 3, output blocks 1 .. 1 of 3
    a_nkb, c_nkb = 3, 3
    Abuf = torch.zeros(_ext.planes_bytes(M, a_nkb), dtype=torch.uint8)
    emulator.planes_encode(emulator._tensor_planes_view(Abuf, M, a_nkb), _rnd(g, M, 32 * a_nkb), 0)
    Cbuf = torch.zeros(_ext.planes_bytes(M, c_nkb), dtype=torch.uint8)
    emulator.planes_encode(emulator._tensor_planes_view(Cbuf, M, c_nkb), _rnd(g, M, 32 * c_nkb), 0)
    Wl = torch.zeros(32, 64)
    Wl[:20] = _rnd(g, 20, 64, scale=0.2)
    slot = torch.tensor([32 * (c // 32) + emulator._slot_feature(c % 32) for c in range(64)])
    Wp = torch.stack(emulator._bf16_planes(Wl[:, slot])).contiguous()
    bias = torch.zeros(32)
    bias[:20] = _rnd(g, 20)
    _direct("gemm_planes", "gemm_planes", emulator._emu_gemm_planes_call, (Abuf, Wp),
            dict(M=M, a_nkb=a_nkb, a_kb0=1, nk=2, bias=bias, C_planes=Cbuf, c_nkb=c_nkb, c_kb0=1, c_kbn=1, act=_ext.ACT_LEAKY_RELU, slope=0.01), K=64, rows=M)
    N, K = 20, 40
    G, cs = _rnd(g, N + 1, K + 4), _rnd(g, N + 2)
    ops = (Cbuf, c_nkb, 1, Abuf, a_nkb, 1, G)
    _direct("wgrad_blocked", "wgrad_blocked", emulator._emu_wgrad_blocked, ops,
            dict(M=M, N=N, K=K, ldg=K + 4, g_off=K + 4, alpha=0.5, beta=-1.5), K=M, rows=M)
    _direct("wgrad_blocked beta = 0", "wgrad_blocked", emulator._emu_wgrad_blocked, ops,
            dict(M=M, N=N, K=K, ldg=K + 4, g_off=K + 4, alpha=1.0, beta=0.0), K=M, rows=M)
    # the column sums ride along from K = 64 on (usf_wgrad_planes_colsum_ok): the form every call of training.py has
    K = 64
    G = _rnd(g, N + 1, K + 4)
    ops = (Cbuf, c_nkb, 1, Abuf, a_nkb, 1, G)
    kw = dict(M=M, N=N, K=K, ldg=K + 4, g_off=K + 4, alpha=0.5, beta=-1.5, colsum=cs)
    _direct("wgrad_blocked + column sums", "wgrad_blocked", emulator._emu_wgrad_blocked, ops, dict(kw, cs_alpha=-0.5, cs_beta=2.5), K=M, rows=M)
    _direct("wgrad_blocked + column sums, overwritten", "wgrad_blocked", emulator._emu_wgrad_blocked, ops,
            dict(kw, beta=0.0, cs_alpha=-1.0, cs_beta=0.0), K=M, rows=M)
    # the reduction queued (usf_wgrad_blocked_plan_f32) and flushed by the binding's own flush / the emulation's
    ws = torch.zeros(_ext.wgrad_blocked_workspace(M, N, K))

    def queued(fn, flush, device):
        def run(*a, **k):
            q = []
            fn(*a, queue=q, **k)
            assert len(q) == 1, "the reduction was not queued"
            flush(q, device)
            assert not q
        return run
    _direct("wgrad_blocked queued", "wgrad_blocked", emulator._emu_wgrad_blocked, ops, dict(kw, cs_alpha=-0.5, cs_beta=2.5, ws=ws), K=M, rows=M,
            call=queued(_ext.wgrad_blocked, _ext.wgrad_reduce_flush, torch.device(DEV)),
            emu_call=queued(emulator._emu_wgrad_blocked, emulator._emu_wgrad_reduce_flush, torch.device("cpu")), scratch=(ws,))


def test_direct_products_on_the_split_precision_kernels():
    """the two forms that exist only from hundreds of rows on, at the smallest ragged row counts that reach them:
    usf_wgrad_bias_f32 (mode 1, M >= 2048, K >= 64: usf_wgrad_bias_ok) -- the weight gradient with the column sums from the same
    pass, alpha / beta / cs_alpha / cs_beta all at work, offsets and padded strides; and usf_linear_f32 on its bf16x3 kernel
    (W_split, more than 768 rows) with the input's planes as a side output: rows >= M and columns >= ceil32(K) of the planes
    stay as they were, columns [K, ceil32(K)) hold finite padding (EXCLUSIONS)"""
    g = torch.Generator().manual_seed(80)
    M, N, K, ldy, lda, ldg = 2048 + 37, 20, 68, 24, 76, 72
    assert _ext.wgrad_bias_ok(M, N, K, ldy, lda, 1)
    Y, A, G, cs = _rnd(g, M + 1, ldy), _rnd(g, M + 1, lda), _rnd(g, N + 1, ldg), _rnd(g, N + 2)
    kw = dict(M=M, N=N, K=K, ldy=ldy, lda=lda, ldg=ldg, y_off=4, a_off=4, g_off=ldg, alpha=0.5, beta=-1.5, mode=1, colsum=cs)
    _direct("wgrad + column sums", "wgrad", emulator._emu_wgrad, (Y, A, G), dict(kw, cs_alpha=-0.5, cs_beta=2.5), K=M)
    _direct("wgrad + column sums, overwritten", "wgrad", emulator._emu_wgrad, (Y, A, G), dict(kw, beta=0.0, cs_alpha=-1.0, cs_beta=0.0), K=M)
    M, N, K, lda, ldw, ldc = 768 + 37, 68, 24, 32, 28, 72
    A, W, Cm = _rnd(g, M + 1, lda), _rnd(g, N, ldw, scale=0.3), _rnd(g, M + 1, ldc)
    Ws = torch.zeros(3, N, 32, dtype=torch.bfloat16)
    for q, pl in enumerate(emulator._bf16_planes(W[:, :K].contiguous())):
        Ws[q, :, :K] = pl
    P = _rnd(g, 3, -(-M // 32) * 32, 40).to(torch.bfloat16)
    open_cols = torch.zeros(P.shape, dtype=torch.bool)
    open_cols[:, :M, K:32] = True
    dims = dict(M=M, N=N, K=K, lda=lda, ldw=ldw, ldc=ldc, W_split=Ws)
    _direct("linear bf16x3 + planes_out", "linear", emulator._emu_linear, (A, W, Cm),
            dict(dims, bias=0.5 + torch.rand(N, generator=g), a_off=4, c_off=8, act=_ext.ACT_LEAKY_RELU, slope=0.01, planes_out=P), K=K,
            unspecified=((P, open_cols),))
