"""Canonical dumps of what the host side of the flat-flow path hands to the library, for comparing two checkouts on the CPU.

    python tools/plan_dump.py plans  > plans.txt     # one record per plan of a fixed list of configurations (--only NAME...: a part)
    python tools/plan_dump.py trace  > trace.txt     # the call sequence of one log_prob_with_grad + backward per configuration,
                                                     # and the gradient arena's hash after it and after a second pass

Both run without a GPU under tests/emulator.py's emulation of the entry points (the library is loaded for its host-only
answers).  Every pointer is written as (tensor it falls in, byte offset): a workspace tensor by its ``ws`` key, every other
tensor by shape, dtype and a hash of its contents -- workspace contents never enter the output (planes buffers are
``torch.empty``).  Run it in two checkouts (``--root`` names the tree whose ``usflows_amd`` and ``tests`` are used) and compare
the outputs byte for byte; ``sha1`` and the record count go to stderr.

The planes couplings' valid widths ``n_p`` / ``n_t`` are printed with every coupling ``meta`` entry: the carried values where
the plan has them, else derived from ``feat_p`` / ``feat_t`` -- so a checkout that carries them compares equal to one that
derives them exactly when the two agree."""
import argparse
import ctypes as C
import hashlib
import os
import sys


def _setup(root):
    root = os.path.abspath(root)
    for p in (os.path.join(root, "tests"), root):
        if p not in sys.path:
            sys.path.insert(0, p)


class Patch:
    """the part of pytest's monkeypatch the emulator's install functions use"""

    def __init__(self):
        self.done, self.items = [], []

    def setattr(self, obj, name, value):
        self.done.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def setitem(self, mapping, key, value):
        self.items.append((mapping, key, key in mapping, mapping.get(key)))
        mapping[key] = value

    def undo(self):
        for obj, name, old in reversed(self.done):
            setattr(obj, name, old)
        for mapping, key, had, old in reversed(self.items):
            if had:
                mapping[key] = old
            else:
                mapping.pop(key, None)
        self.done, self.items = [], []


# ---- naming tensors ----------------------------------------------------------------------------------------------------
class Names:
    """(tensor, byte offset) of a raw address.  ``ws``: the plan's workspace; ``roots``: containers walked for every other tensor"""

    def __init__(self, ws, roots, named=()):
        import torch
        self.torch = torch
        self.entries = []                      # (base, nbytes, rank, label-or-tensor)
        for key, t in ws.items():
            if torch.is_tensor(t) and t.numel() > 0:
                self._add(t, 0, f"ws:{key}")
        for label, t in named:
            if torch.is_tensor(t) and t.numel() > 0:
                self._add(t, 1, label)
        seen = set()
        for r in roots:
            self._walk(r, seen, 0)
        self._ids = {}

    def _add(self, t, rank, label):
        st = t.untyped_storage()
        self.entries.append((t.data_ptr(), t.numel() * t.element_size(), rank, label, st.data_ptr(), st.nbytes()))

    def _walk(self, o, seen, depth):
        torch = self.torch
        if torch.is_tensor(o):
            if o.numel() > 0 and id(o) not in seen:
                seen.add(id(o))
                self._add(o, 2, o)
            return
        if id(o) in seen or depth > 8:
            return
        if isinstance(o, dict):
            seen.add(id(o))
            for k, v in o.items():
                if k not in ("ws", "_ws", "_plans", "arr", "grad_arena"):
                    self._walk(v, seen, depth + 1)
        elif isinstance(o, (list, tuple, set)):
            seen.add(id(o))
            for v in o:
                self._walk(v, seen, depth + 1)
        elif hasattr(o, "__dict__") and type(o).__module__.startswith("usflows_amd") and not isinstance(o, torch.nn.Module):
            seen.add(id(o))
            self._walk(vars(o), seen, depth + 1)
        elif hasattr(o, "__slots__") and type(o).__module__.startswith("usflows_amd"):
            seen.add(id(o))
            for s in o.__slots__:
                self._walk(getattr(o, s, None), seen, depth + 1)

    def _label(self, lab):
        if isinstance(lab, str):
            return lab
        k = id(lab)
        if k not in self._ids:
            t = lab.detach()
            if not t.is_contiguous():
                t = t.contiguous()
            raw = t.reshape(-1).view(self.torch.uint8).numpy().tobytes()
            self._ids[k] = f"pack:{list(lab.shape)}:{str(lab.dtype)[6:]}:{hashlib.sha1(raw).hexdigest()[:16]}"
        return self._ids[k]

    def of_ptr(self, ptr, strict=True):
        if not ptr:
            return "null"
        best = None
        for base, nbytes, rank, lab, _sb, _sn in self.entries:
            if base <= ptr < base + nbytes:
                cand = (rank, nbytes, self._label(lab), ptr - base)
                if best is None or cand < best:
                    best = cand
        if best is None:
            if strict:
                raise KeyError(f"pointer {ptr:#x} falls in no known tensor")
            return "unknown"
        return f"{best[2]}+{best[3]}"

    def of_tensor(self, t):
        """a tensor argument: the known tensor it is (a view of), shape, strides; tensors of the call's own by shape and dtype"""
        if t.numel() == 0:
            return f"empty:{list(t.shape)}:{str(t.dtype)[6:]}"
        where = self.of_ptr(t.data_ptr(), strict=False)
        if where == "unknown":
            return f"other:{list(t.shape)}:{str(t.dtype)[6:]}"
        return f"{where}:{list(t.shape)}:{list(t.stride())}"


# ---- ops and meta ------------------------------------------------------------------------------------------------------
def _field(v, t, names, _ext):
    if t is _ext._fp:
        return names.of_ptr(v or 0)
    if isinstance(t, type) and issubclass(t, C.Array):
        return [_field(x, t._type_, names, _ext) for x in v]
    if t in (C.c_float, C.c_double):
        return repr(float(v))
    return int(v)


def op_record(op, names, _ext):
    members = {_ext.OP_LINEAR: "linear", _ext.OP_COUPLING: "coupling", _ext.OP_PACK_PLANES: "pack_planes",
               _ext.OP_GEMM_PLANES: "gemm_planes", _ext.OP_COUPLING_PLANES: "coupling_planes", _ext.OP_GATED_NORM: "gated_norm",
               _ext.OP_CALL: "call"}
    member = members[op.kind]
    d = getattr(op.u, member)
    if member == "call":
        a = [int(d.a[j]) for j in range(d.n_args)]
        if d.fn == _ext.FN_COUPLING_VCTX:          # ctx, ld_ctx, ctx_dim, W_ctx_t, ldw_ctx, b_ctx
            a = [names.of_ptr(a[0]), a[1], a[2], names.of_ptr(a[3]), a[4], names.of_ptr(a[5])]
        elif _ext.is_ctx_prefix(op):               # ctx, ctx_stride, w_ctx, b_ctx
            a = [names.of_ptr(a[0]), a[1], names.of_ptr(a[2]), names.of_ptr(a[3])]
        elif _ext.is_side_prefix(op):              # side, then block numbers
            a = [names.of_ptr(a[0])] + a[1:]
        return f"call fn={d.fn} n_args={d.n_args} a={a}"
    parts = [f"{name}={_field(getattr(d, name), t, names, _ext)}" for name, t in d._fields_]
    return member + " " + " ".join(parts)


def canon(v, eng):
    import torch
    if torch.is_tensor(v):
        return f"tensor:{str(v.dtype)[6:]}:{list(v.shape)}:{v.tolist()}"
    if isinstance(v, torch.nn.Module) or type(v).__name__ == "_MergedAffine":
        for j, s in enumerate(list(eng.steps) + list(getattr(eng, "_virtual", []))):
            if s.module is v:
                return f"module:step{j}"
        return f"module:{type(v).__name__}"
    if isinstance(v, dict):
        return "{" + ", ".join(f"{k}: {canon(v[k], eng)}" for k in sorted(v)) + "}"
    if isinstance(v, (list, tuple)):
        return "[" + ", ".join(canon(x, eng) for x in v) + "]"
    if isinstance(v, float):
        return repr(v)
    if isinstance(v, (bool, int, str)) or v is None:
        return repr(v)
    return f"<{type(v).__name__}>"


def meta_record(m, eng):
    m = dict(m)
    if m.get("kind") == "coupling" and "feat_p" in m:
        for w, feat, kb0 in (("n_p", m["feat_p"], m["kb_p0"]), ("n_t", m["feat_t"], m["kb_t0"])):
            if w not in m:
                m[w] = int((feat >= 0).nonzero().max().item()) + 1 - 32 * kb0
    return canon(m, eng)


def plan_record(title, eng, plan, _ext, extra_roots=()):
    names = Names(plan["ws"], [plan["pk"], {k: v for k, v in vars(eng).items() if k not in ("_ws", "_plans")}] + list(extra_roots))
    out = [f"== {title}"]
    for j in range(plan["n"]):
        out.append(f"op{j} {op_record(plan['arr'][j], names, _ext)}")
    side = []
    for g in plan["side"]:
        import torch
        side.append([names.of_tensor(x) if torch.is_tensor(x) else x for x in g])
    out.append(f"side {canon(side, eng)}")
    for key in ("final_gather", "patch_in", "patch_out", "out_buf"):
        out.append(f"{key} {canon(plan[key], eng)}")
    out.append(f"n_part {plan.get('n_part', 0)} planes {plan.get('planes', False)} planes_fmt {plan.get('planes_fmt')} "
               f"planes_train {plan.get('planes_train', False)} has_ctx {plan.get('has_ctx', False)}")
    for j, m in enumerate(plan["meta"]):
        out.append(f"meta{j} {meta_record(m, eng)}")
    return out


# ---- the configurations ------------------------------------------------------------------------------------------------
VARIANTS = [("f32", False, False), ("f32_fused", True, False), ("bf16x3", False, "bf16x3"), ("bf16x3_fused", True, "bf16x3"),
            ("f16x2", False, "f16x2"), ("f16x2_fused", True, "f16x2")]
CTX_CASES = ("synth_d7_k3_soft_ctx", "synth_d7_k3_soft_noctx")
TRAIN_F32 = ("synth_d16_k3_densenn_relu", "synth_d16_k4_hh2_conj_laplace", "synth_d7_k3_soft_ctx")
PLANES_TRAIN = [(160, 2, [96, 64], False, 0), (136, 3, [72], False, 0), (160, 2, [64, 64], True, 1)]


def _switches(eng, fused, planes):
    """the engine switches as tests/emulator.py's engine_transform sets them"""
    eng.use_fused_coupling = fused
    eng.fused_min_rows = 0
    eng.use_planes, eng.planes_min_rows = bool(planes), 0
    if planes:
        eng.gemm_mode = planes
    if fused:
        eng._fused_ok = lambda cp: len(cp["hidden"]) <= 3


def _planes_train_flow(D, K, hidden, conj, hh, base="laplace"):
    from model_util import build_flow
    from oracle.synth import ModelSpec, synth_state_dict
    spec = ModelSpec(dim=D, coupling_blocks=K, hidden_dims=hidden, householder=hh, affine_conjugation=conj, base=base)
    flow = build_flow(spec, synth_state_dict(spec, seed=3))
    eng = flow.engine()
    eng.use_planes, eng.planes_min_rows, eng.fused_min_rows, eng.train_planes_min_rows = True, 0, 0, 0
    return flow, eng


def _planes_train_ctx_flow():
    from model_util import build_flow
    from oracle import usflows_oracle as orc
    spec = orc.FlowSpec(160, 2, [64, 48], soft_training=True, negative_slope=1.0, base="normal")
    flow = build_flow(spec, orc.synth_state_dict(spec, seed=9))
    eng = flow.engine()
    eng.use_planes, eng.planes_min_rows, eng.fused_min_rows, eng.train_planes_min_rows = True, 0, 0, 0
    eng.train_ctx_planes_min_rows = 0
    return flow, eng


def _single_layer_plans(one, name, dev):
    """every layer of a flow as an engine of its own, as layer.forward / layer.backward dispatch: the one place a stand-alone
    scale launch and the gather in front of a coupling occur"""
    from golden_util import load_case
    from model_util import build_flow
    from usflows_amd.engine import FlowEngine
    spec, sd, _a = load_case(name)
    for j, layer in enumerate(build_flow(spec, sd).layers):
        eng = FlowEngine([layer])
        _switches(eng, False, False)
        for direction in ("forward", "backward"):
            one(f"single {name} layer{j} {type(layer).__name__} B=37 {direction} user", eng, direction, 37, dev, False, "user")


def _flat_branch_plans(one, want, dev):
    """the branches of the fp32-row builder the golden list never enters: the tiny-layer kernel, vector contexts, a general
    conditioner in training, A_planes_out, hidden activations saved by the fused kernel, one-layer engines"""
    import vctx_cases
    from golden_util import load_case
    from model_util import build_flow
    for name in ("init_d10_k10_gmlive", "init_d2_k10_gmlive"):               # engine defaults: every coupling is "tiny"
        if want(f"tiny:{name}"):
            spec, sd, _a = load_case(name)
            for train in (False, True):
                eng = build_flow(spec, sd).engine()
                eng.keep_factors = True
                one(f"tiny {name} defaults B=32 train={train}", eng, "backward", 32, dev, False, "nat", train=train)
    for name in ("d7_k3", "d16_k3", "d33_k2", "d64_k2_c10"):
        if want(f"vctx:{name}"):
            B = vctx_cases.CASES[name][2]
            for train in (False, True):
                eng = vctx_cases.build(name).engine()
                eng.keep_factors = True
                if name == "d64_k2_c10":
                    eng.gemm_mode = "bf16x3"
                one(f"vctx {name} B={B} mode={eng.gemm_mode} train={train}", eng, "backward", B, dev, True, "nat", train=train)
    for name in ("synth_d16_k3_convnet_gated_ln", "synth_d33_k2_convnet_gated_conj"):
        if want(f"general-train:{name}"):
            spec, sd, _a = load_case(name)
            eng = build_flow(spec, sd).engine()
            eng.keep_factors = True
            one(f"general-train {name} B=37", eng, "backward", 37, dev, False, "nat", train=True)
    # fp32 rows in bf16x3 mode: (the planes flow, rows, fused override) -- A_planes_out needs usf_wgrad_planes_ok's 8192+ rows,
    # the fused kernel's saved hidden activations hmax >= 256 and >= 1024 rows
    for tag, cfg, B, fused in (("A_planes_out", (160, 2, [96, 64], False, 0), 40960, False),
                               ("fused_hidden", (64, 2, [200, 256], False, 1), 1100, True)):
        if want(f"rows-train:{tag}"):
            _flow, eng = _planes_train_flow(*cfg)
            eng.use_train_planes, eng.use_planes, eng.gemm_mode, eng.keep_factors = False, False, "bf16x3", True
            if fused:
                eng.use_fused_coupling = True
                eng._fused_ok = lambda cp: len(cp["hidden"]) <= 3
            one(f"rows-train {tag} {cfg} bf16x3 B={B}", eng, "backward", B, dev, False, "nat", train=True)
    if want("single:synth_d7_k3_hh1_conj_normal"):
        _single_layer_plans(one, "synth_d7_k3_hh1_conj_normal", dev)


def dump_plans(emit, only=None):
    """only: the case names to dump (a golden case's name, or a ``group:name`` of the lists below); None = all of them"""
    import torch
    from golden_util import case_names, load_case
    from model_util import build_flow
    from usflows_amd import _ext
    from usflows_amd.engine import FlowEngine
    import emulator
    patch = Patch()
    emulator.install_prep_emulation(patch)
    dev = torch.device("cpu")
    n = 0
    want = lambda case: only is None or case in only      # noqa: E731

    def one(title, eng, *args, **kw):
        nonlocal n
        try:
            plan = eng._plan(*args, **kw)
        except Exception as e:                       # a configuration the engine does not accept: part of the record
            emit([f"== {title}", f"rejected {type(e).__name__}: {e}"])
        else:
            emit(plan_record(title, eng, plan, _ext))
        n += 1

    try:
        for name in case_names(small_only=True):
            if not want(name):
                continue
            spec, sd, a = load_case(name)
            natural = a.get("context") is not None or bool(spec.soft_training)
            rows = (37, 32, 300) if name.endswith("_gmlive") else (37,)
            for vname, fused, planes in VARIANTS:
                for has_ctx in ((True, False) if name in CTX_CASES else (natural,)):
                    for B in rows:
                        eng = FlowEngine(build_flow(spec, sd).layers)
                        _switches(eng, fused, planes)
                        for direction in ("backward", "forward"):
                            for final in ("user", "nat", "base0"):
                                one(f"{name} {vname} ctx={has_ctx} B={B} {direction} {final}", eng, direction, B, dev, has_ctx, final)
        for name in TRAIN_F32:
            if not want(f"train:{name}"):
                continue
            spec, sd, a = load_case(name)
            has_ctx = a.get("context") is not None or bool(spec.soft_training)
            for fused in (False, True):
                eng = build_flow(spec, sd).engine()
                _switches(eng, fused, False)
                eng.keep_factors = True
                one(f"{name} train f32 fused={fused} B=37", eng, "backward", 37, dev, has_ctx, "nat", train=True)
        if want("planes-train"):
            for cfg in PLANES_TRAIN:
                flow, eng = _planes_train_flow(*cfg)
                eng.keep_factors = True
                one(f"planes-train {cfg} B=37", eng, "backward", 37, dev, False, "nat", train=True)
            flow, eng = _planes_train_ctx_flow()
            eng.keep_factors = True
            one("planes-train ctx B=600", eng, "backward", 600, dev, True, "nat", train=True)
        _flat_branch_plans(one, want, dev)
    finally:
        patch.undo()
    return n


# ---- the training call trace -------------------------------------------------------------------------------------------
class _Index:
    def __init__(self, t, sha):
        self.t, self.sha = t, sha


class Trace:
    def __init__(self, _ext):
        self._ext = _ext
        self.calls = []            # (name, args, kwargs) with tensors / ops kept for naming at the end

    def wrap(self, name, fn):
        def logged(*args, **kw):
            self.calls.append((name, [self._keep(v) for v in args], {k: self._keep(v) for k, v in kw.items()}))
            return fn(*args, **kw)
        return logged

    def _keep(self, v):
        import torch
        if isinstance(v, self._ext.Op):
            return self._ext.Op.from_buffer_copy(bytes(v))
        if torch.is_tensor(v) and not v.dtype.is_floating_point and 0 < v.numel() <= 1 << 16:
            # an index table, maybe a temporary of the caller: its contents are part of the call
            return _Index(v, hashlib.sha1(v.detach().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()[:16])
        if isinstance(v, (list, tuple)):
            return [self._keep(x) for x in v]
        return v

    def _show(self, v, names):
        import torch
        if isinstance(v, _Index):
            shown = names.of_tensor(v.t)
            return shown if not shown.startswith("other:") else f"index:{list(v.t.shape)}:{str(v.t.dtype)[6:]}:{v.sha}"
        if torch.is_tensor(v):
            return names.of_tensor(v)
        if isinstance(v, self._ext.Op):
            return "op(" + op_record(v, names, self._ext) + ")"
        if isinstance(v, list):
            return "[" + ", ".join(self._show(x, names) for x in v) + "]"
        if isinstance(v, float):
            return repr(v)
        if isinstance(v, (bool, int, str)) or v is None:
            return repr(v)
        if isinstance(v, torch.device):
            return str(v)
        return f"<{type(v).__name__}>"

    def lines(self, names):
        out = []
        for name, args, kw in self.calls:
            shown = [self._show(v, names) for v in args] + [f"{k}={self._show(kw[k], names)}" for k in sorted(kw)]
            out.append(f"{name}({', '.join(shown)})")
        return out


def _sha(t):
    import torch
    return hashlib.sha1(t.detach().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def trace_one(title, flow, eng, x, ctx, g_lp, emit, defer=True, fused=None, vctx=False, want_dx=False):
    """one record: the calls of the first log_prob_with_grad + backward, then the gradient arena's hash after that pass and
    after a second pass on the same path and input (want_dx: the input requires grad; its gradient is hashed as well)"""
    import emulator
    import emulator_ctx
    import emulator_vctx
    from usflows_amd import _ext, training
    from usflows_amd.training import TrainPath
    patch = Patch()
    emulator.install_training_emulation(patch)
    emulator_ctx.install(patch)
    if vctx:
        emulator_vctx.install(patch)
    tr = Trace(_ext)
    wrapped = set()
    for obj, name, _old in list(patch.done):
        if (obj is _ext or obj is _ext.batch_jobs) and (obj, name) not in wrapped and callable(getattr(obj, name)):
            wrapped.add((obj, name))
            label = name if obj is _ext else f"batch_jobs.{name}"
            patch.setattr(obj, name, tr.wrap(label, getattr(obj, name)))
    for name in ("host_op", "flush_jobs"):
        patch.setattr(_ext, name, tr.wrap(name, getattr(_ext, name)))
    try:
        path = TrainPath(flow)
        path.defer_small_grads = defer
        if fused is not None:
            eng.use_fused_coupling = fused
        if want_dx:
            x = x.clone().requires_grad_(True)
        assert path.supported(x, ctx)
        hashes = []
        for nth in ("first", "second"):
            x.grad = None
            lp = training.log_prob_with_grad(path, x, ctx)
            (lp * g_lp).sum().backward()
            if nth == "first":
                n_first = len(tr.calls)
                keep = eng.use_train_planes
                if want_dx:                        # (TrainPath.forward: the input's gradient leaves the fp32-row plan)
                    eng.use_train_planes = False
                plan = eng._plan("backward", x.shape[0], x.device, ctx is not None, "nat", train=True)
                eng.use_train_planes = keep
            hashes.append(f"arena after the {nth} backward: sha1 {_sha(plan['grad_arena']['flat'])}"
                          + (f" dx {_sha(x.grad)}" if want_dx else ""))
        hashes[1] += f" calls={len(tr.calls) - n_first}"
        del tr.calls[n_first:]
        named = [(f"param:{k}", p) for k, p in flow.named_parameters()] + [("x", x), ("g_lp", g_lp)]
        if ctx is not None:
            named.append(("ctx", ctx))
        arena = plan.get("grad_arena")
        if arena is not None:
            named.append(("arena", arena["flat"]))
        names = Names(plan["ws"], [plan["pk"], {k: v for k, v in vars(eng).items() if k not in ("_ws", "_plans")},
                                   {k: v for k, v in vars(path).items() if k not in ("flow", "eng", "_cur")}], named)
        flags = sorted({k for m in plan["meta"] for k in ("tiny", "hidden_saved", "hidden_saved_fused") if m.get(k)})
        ps = plan.get("bwd_pass")                  # the recorded backward's pass object (a tree from before it: the path's attribute)
        deferred = ps.defer if ps is not None else getattr(path, "_defer", False)
        head = [f"== {title}: planes_train={bool(plan.get('planes_train'))} deferred={bool(deferred)} "
                f"flags={flags} calls={len(tr.calls)}"]
        emit(head + tr.lines(names) + hashes)
    finally:
        patch.undo()


def dump_trace(emit):
    import torch
    from golden_util import load_case
    from model_util import build_flow
    n = 0
    for cfg in PLANES_TRAIN + [PLANES_TRAIN[1] + ("radial",)]:          # (+ a radial base: the latent's gradient as fp32 rows)
        flow, eng = _planes_train_flow(*cfg)
        g = torch.Generator().manual_seed(7)
        x = torch.rand(37, cfg[0], generator=g)
        trace_one(f"planes-train {cfg} B=37", flow, eng, x, None, torch.randn(37, generator=g), emit)
        n += 1
    for with_ctx in (True, False):
        flow, eng = _planes_train_ctx_flow()
        g = torch.Generator().manual_seed(7)
        x = torch.rand(600, 160, generator=g)
        ctx = torch.rand(600, 1, generator=g) * 2
        g_lp = -(0.5 + torch.rand(600, generator=g)) / 600
        trace_one(f"planes-train soft ctx={with_ctx} B=600", flow, eng, x, ctx if with_ctx else None, g_lp, emit)
        n += 1
    # fp32 rows: queued gradient jobs (B <= GRAD_JOB_MAX_ROWS), launched in place, the fused conditioner backward
    for title, name, defer, rows, fused in (("f32 deferred", "synth_d16_k4_hh2_conj_laplace", True, None, False),
                                            ("f32 not deferred", "synth_d16_k4_hh2_conj_laplace", False, None, False),
                                            ("f32 ctx deferred", "synth_d7_k3_soft_ctx", True, None, None),
                                            ("f32 radial base", "synth_d16_k3_hh1_radial2", True, None, None),
                                            ("f32 fused conditioner backward", "init_d10_k10_gmlive", True, 32, None)):
        spec, sd, a = load_case(name)
        flow = build_flow(spec, sd)
        x, ctx = a["x"], a.get("context")
        if rows is not None:
            x = x[:rows] if x.shape[0] >= rows else x.repeat(-(-rows // x.shape[0]), 1)[:rows]
            ctx = None if ctx is None else ctx[:rows]
        if ctx is None and spec.soft_training:
            ctx = torch.zeros(x.shape[0], 1)
        g_lp = torch.randn(x.shape[0], generator=torch.Generator().manual_seed(1))
        trace_one(f"{title}: {name} B={x.shape[0]}", flow, flow.engine(), x.contiguous(), ctx, g_lp, emit, defer=defer, fused=fused)
        n += 1
    # fp32 rows: a vector context (above the tiny kernel's rows) and a general (gated / layer-norm) conditioner
    import vctx_cases
    x, _zin, ctx = vctx_cases.inputs("d33_k2")
    flow = vctx_cases.build("d33_k2")
    g_lp = torch.randn(x.shape[0], generator=torch.Generator().manual_seed(1))
    trace_one(f"f32 vector ctx: d33_k2 B={x.shape[0]}", flow, flow.engine(), x.contiguous(), ctx, g_lp, emit, vctx=True)
    spec, sd, a = load_case("synth_d16_k3_convnet_gated_ln")
    flow = build_flow(spec, sd)
    g_lp = torch.randn(a["x"].shape[0], generator=torch.Generator().manual_seed(1))
    trace_one(f"f32 general conditioner: synth_d16_k3_convnet_gated_ln B={a['x'].shape[0]}", flow, flow.engine(), a["x"].contiguous(),
              None, g_lp, emit)
    n += 2
    # fp32 rows: an input that requires grad (the first layer's data gradient; one case at a padded dim), a block of two LU
    # factors (the unbatched chain rule through _to_leaves's torch graph), a DenseNN without a context layer
    for title, name, want_dx in (("f32 input gradient", "synth_d7_k3_hh0_laplace", True),
                                 ("f32 input gradient, padded dim", "init_d2_k4_hh0_laplace", True),
                                 ("f32 two LU factors per block", "synth_d33_k3_lu2_hh1", False),
                                 ("f32 DenseNN", "synth_d16_k3_densenn_relu", False)):
        spec, sd, a = load_case(name)
        flow = build_flow(spec, sd)
        g_lp = torch.randn(a["x"].shape[0], generator=torch.Generator().manual_seed(1))
        trace_one(f"{title}: {name} B={a['x'].shape[0]}", flow, flow.engine(), a["x"].contiguous(), None, g_lp, emit, want_dx=want_dx)
        n += 1
    # a trainable Normal / Laplace base (its parameter gradients: one pass over the latent), fp32 rows and planes
    from golden_util import load_trainable_base_case
    for name in ("tbase_d16_k3_hh0_normal_scalar_scale", "tbase_d160_k2_hh0_laplace"):
        spec, sd, x = load_trainable_base_case(name)[:3]
        flow = build_flow(spec, sd)
        eng = flow.engine()
        if spec.dim >= 128:
            eng.use_planes, eng.planes_min_rows, eng.fused_min_rows, eng.train_planes_min_rows = True, 0, 0, 0
        g_lp = torch.full((x.shape[0],), -1.0 / x.shape[0])
        trace_one(f"trainable base: {name} B={x.shape[0]}", flow, eng, x.contiguous(), None, g_lp, emit)
        n += 1
    return n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("mode", choices=["plans", "trace"])
    ap.add_argument("--only", nargs="+", default=None, help="plans: the case names to dump (default: all)")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose usflows_amd / tests are used (default: this file's)")
    args = ap.parse_args()
    _setup(args.root)
    sha = hashlib.sha1()

    def emit(lines):
        text = "\n".join(lines) + "\n"
        sha.update(text.encode())
        sys.stdout.write(text)

    n = dump_plans(emit, args.only) if args.mode == "plans" else dump_trace(emit)
    print(f"{args.mode}: {n} records, sha1 {sha.hexdigest()}", file=sys.stderr)


if __name__ == "__main__":
    main()
