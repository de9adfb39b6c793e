"""Training step on the device: ``Flow.log_prob`` under autograd as ONE autograd node whose
forward is the engine's launch list and whose backward is hand-derived -- what ``Flow.fit`` (flows.py:196-199:
``loss = -log_prob(batch).mean() - log_prior()``) asks autograd to differentiate.

forward   the log_prob launch list (engine_flat.py) with every affine output kept in a buffer of its own (the saved
          activations; couplings update their transformed half in place, and their conditioning half -- all the
          backward needs of them -- is untouched), then the base-density tail.
backward  usf_base_logprob_grad_f32 -> per layer, last to first:
            affine    usf_wgrad_f32 (g^T a), usf_colsum_f32, data gradient = usf_linear_f32 on the transposed image
            coupling  hidden activations recomputed by two usf_linear_f32 launches, then per conditioner layer
                      usf_wgrad_f32 / usf_colsum_f32 / usf_linear_f32 (transposed image) / usf_act_grad_f32;
                      the conditioning half of the gradient is updated in place
          (every layer keeps gradient images of its own; the scatter / un-permute copies into the parameter layout are
          queued and leave as one usf_pack_weights_f32 launch per size class behind the last layer)
          then the parameter-sized chain rule, batched over all LU blocks on the f64 MFMA (usf_gemm_f64; the formulas:
          training_chain.py); longer Sequential chains go through a small torch graph over the prepared fp64 matrices.

Supported here: flat inputs, Laplace / Normal base without trainable parameters or a RadialDistribution base (the
node then returns the Lp radius + log-det and the finishing formula stays in torch), inputs that do not require grad,
ConditionalDenseNN / DenseNN conditioners; anything else keeps using the differentiable composite formulation
(flows.py / transforms.py mirrors) -- same results, torch ops.

Where what lives:
  training.py          this map; ``TrainPath`` (eligibility, forward, backward with its tape, the gradient arena, bound
                       gradients, the all-reduce), the autograd nodes, ``log_prob_with_grad`` / ``log_prob_empty_shard``
  training_pass.py     ``Pass`` -- the state of ONE backward pass, handed to every layer function --, the opening both layer
                       loops share, ``linear_grads`` (the parameter gradients of one Linear layer) and the scatter helpers
  training_rows.py / training_planes.py    the two layer loops: affine and coupling layers on fp32 rows / on gradient planes
  training_chain.py    the parameter-sized fp64 chain rule (LU factors, Householder vectors, ScaleTransform)
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import _ext
from . import training_planes, training_rows
from . import transforms as T
from .config import config
from .engine import FlowEngine
from .networks import ConditionalDenseNN, ConvNet, DenseNN
from .training_pass import Pass, ws_buf


class TrainUnsupported(Exception):
    pass


class TrainPath:
    """forward / backward of ``Flow.log_prob`` for one flow (owned by the Flow; shares the FlowEngine)."""

    defer_small_grads = True      # batches <= _ext.GRAD_JOB_MAX_ROWS: weight / bias gradients as one usf_grad_jobs_f32 launch

    def __init__(self, flow):
        self.flow = flow
        self.eng: FlowEngine = flow.engine()
        self._inv: Dict[tuple, torch.Tensor] = {}         # selectors / constants keyed by layout and device: outlive every pass
        # What else outlives a pass (everything a pass itself knows is a training_pass.Pass):
        self._cur = None        # the current call's x, g_lp, gsum: the tape's host_op closures read them on every replay
        self._dx = None         # (buffer, row stride) the last backward left the input's gradient in (_input_grad reads it)
        # data-parallel training (parallel.data_parallel_training): (process group | None, average?) -- the whole flat
        # gradient arena goes through ONE all-reduce per step (RCCL over xGMI with the "nccl" backend)
        self.grad_allreduce = None

    # ---- eligibility ----------------------------------------------------------------------------------
    def supported(self, x: torch.Tensor, context) -> bool:
        eng = self.eng
        if eng is None or (context is not None and context.requires_grad):
            return False
        # (an input that requires grad -- round 5: the backward also returns d log_prob / dx, see ``_input_grad``)
        info = self.flow._base_info(x.device)
        if info is None:
            return False
        if info[0] == "radial":
            # RadialDistribution (distributions.py:327-549): trainable loc / norm distribution are fine -- the node
            # returns the Lp radius and the finishing formula stays in torch (O(B), differentiable)
            if getattr(self.flow.base_distribution, "n_batch_dims", 1) != 0:
                return False
        elif any(p.requires_grad for p in self._base_params()) and self._locscale_base() is None:
            return False
        for s in eng.steps:
            if s.kind == "coupling" and not isinstance(s.module.conditioner, (ConditionalDenseNN, DenseNN)):
                # the vector ConvNet with GatedMLP / LayerNormVector blocks (networks.py:206-245, 287-308): chain of linear launches
                # + row passes, backward in training_rows.coupling_backward_general
                cond = s.module.conditioner
                if not (isinstance(cond, ConvNet) and cond.is_vector and not cond.is_plain_mlp() and context is None
                        and not getattr(cond, "consumes_context", False)):
                    return False
            if s.kind == "scale" and s.inverted:
                return False
        return True

    def _base_params(self):
        b = self.flow.base_distribution
        return list(b.parameters()) if isinstance(b, torch.nn.Module) else []

    def _locscale_base(self):
        """the base distribution when it is one of the reference's TRAINABLE Laplace / Normal modules (distributions.py:199-238:
        ``loc`` and a softplus-constrained ``scale_unconstrained`` as nn.Parameters, [D] or broadcast over the features): their
        gradients come from usf_base_param_grad_f32"""
        from .distributions import Laplace, Normal
        b = self.flow.base_distribution
        if not isinstance(b, (Laplace, Normal)) or getattr(b, "n_batch_dims", 0) != 0:
            return None
        D = self.eng.D
        for p in (b.loc, b.scale_unconstrained):
            if p.dim() > 1 or (p.dim() == 1 and p.shape[0] not in (1, D)) or p.dtype != torch.float32:
                return None
        return b

    def base_extra_params(self, device=None) -> List[torch.nn.Parameter]:
        """trainable parameters of the base distribution whose gradients the node itself produces (besides the layers')"""
        b = self._locscale_base()
        if b is None:
            return []
        return [p for p in (b.loc, b.scale_unconstrained) if p.requires_grad]

    def _base_tensors(self, ws, info, refill=False):
        """(base id, loc, scale) for the tail / gradient kernels.  A trainable Laplace / Normal module: persistent [D] buffers
        of the workspace, refilled by every forward pass (the recorded backward launches keep reading the same addresses)"""
        base, loc, scale = self._base_ids(info)
        if info[0] != "radial" and self.base_extra_params():
            D = self.eng.D
            lb, sb = ws_buf(ws, "base_loc", 1, D)[0, :D], ws_buf(ws, "base_scale", 1, D)[0, :D]
            if refill:
                lb.copy_(loc)
                sb.copy_(scale)
            return base, lb, sb
        return base, loc, scale

    def params(self) -> List[torch.nn.Parameter]:
        return self.eng._params()

    # ---- forward --------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, context, want_dx: bool = False):
        eng = self.eng
        x = eng._check_input(x)
        B = x.shape[0]
        dev = x.device
        eng.keep_factors = True
        # the input's gradient leaves the fp32-row backward (the planes backward ends in planes of the first layer's weight
        # gradient operand, not in rows)
        keep, eng.use_train_planes = eng.use_train_planes, eng.use_train_planes and not want_dx
        try:
            plan = eng._plan("backward", B, dev, context is not None, "nat", train=True)
        finally:
            eng.use_train_planes = keep
        self._check_plan(plan)
        if want_dx:
            self._check_input_grad(plan)
        eng._run(plan, x, None, context)
        zname, _, ldn = plan["out_buf"]
        info = self.flow._base_info(dev)
        base, loc, scale = self._base_tensors(plan["ws"], info, refill=True)
        # what the backward must find unchanged: the workspace's pass counter (ANY later pass over the same (B, device)
        # workspace -- a training forward or a no_grad log_prob / backward / sample -- overwrites the saved
        # activations, the staged input and the context columns) and the parameter versions
        gen = (plan["ws"]["_gen"], eng._version_key(dev))
        if info[0] == "radial":
            # the radius stays in a plan-owned buffer (the backward's d r / d z needs it); the caller gets a copy
            rbuf = ws_buf(plan["ws"], "radius", 1, B)[0, :B]
            _ext.base_logprob(plan["ws"][zname], ldn, B, eng.D, base, loc, None, 0.0, rbuf, None)
            return rbuf.clone(), plan, x, gen
        lp = torch.empty(B, dtype=torch.float32, device=dev)
        _ext.base_logprob(plan["ws"][zname], ldn, B, eng.D, base, loc, scale, 0.0, lp, None,
                          logdet_dev=plan["pk"]["ladj_total"].neg_dev)
        return lp, plan, x, gen

    def revalidate(self, ctx):
        """called by the autograd nodes' backward: (1) parameters changed since the forward (optimiser step /
        load_state_dict in between): the gradient would be evaluated at other parameters than the returned log_prob
        -> error, as torch does for saved tensors modified in place; (2) another pass used the workspace: run this
        node's forward again (same parameters, same input -> same activations)"""
        ws_gen, vkey = ctx.gen
        if self.eng._version_key(ctx.x.device) != vkey:
            raise RuntimeError("usflows_amd: parameters were modified between Flow.log_prob and its backward pass "
                               "(optimiser step or load_state_dict in between); the device training path keeps "
                               "activations, not parameter copies -- call backward() before changing parameters")
        if ctx.plan["ws"].get("_gen") != ws_gen:
            _, ctx.plan, ctx.x, ctx.gen = self.forward(ctx.x, ctx.context, want_dx=ctx.want_dx)

    @staticmethod
    def _base_ids(info):
        if info[0] == "radial":
            return {1.0: _ext.BASE_LPNORM1, 2.0: _ext.BASE_LPNORM2}.get(info[2], _ext.BASE_LPNORMINF), info[1], None
        return (_ext.BASE_LAPLACE if info[0] == "laplace" else _ext.BASE_NORMAL), info[1], info[2]

    def _check_plan(self, plan):
        if plan["final_gather"] is not None:
            raise TrainUnsupported("layer list does not end in an affine block")
        for g in plan["side"]:
            if g[0] != "gather" or g[1] != 0 or g[2][0] != "user_in":
                raise TrainUnsupported("stand-alone scale layer / mid-flow layout change")
        for m in plan["meta"]:
            if m["kind"] == "affine" and m["post_scale"] is not None:
                raise TrainUnsupported("forward-direction scale fusion")
        # everything the backward relies on is checked HERE, before the autograd node exists, so that an unsupported
        # layer list falls back to the composite formulation in Flow.log_prob instead of failing inside loss.backward()
        if plan.get("train_checked"):
            return
        D = self.eng.D
        for m in plan["meta"]:
            if m["kind"] == "affine":
                blk = m["blk"]
                parts = list(blk.transforms) if isinstance(blk, T.SequentialAffineTransform) else [blk]
                if not all(isinstance(t, (T.LUTransform, T.HouseholderTransform)) for t in parts):
                    raise TrainUnsupported(f"affine part {[type(t).__name__ for t in parts]}")
            elif m["kind"] == "coupling":
                cond = self.eng.steps[m["step"]].module.conditioner
                if isinstance(cond, ConvNet):
                    if not plan["pk"]["coupling"][m["step"]].get("general"):
                        raise TrainUnsupported("ConvNet conditioner without the general (block-wise) pack")
                    continue
                has_ctx = isinstance(cond, ConditionalDenseNN)
                h = [int(v) for v in cond.hidden_dims]
                want = [(h[0], D)] + ([(h[0], self.eng.ctx_dim)] if has_ctx else []) + \
                       [(h[i + 1], h[i]) for i in range(len(h) - 1)] + [(D, h[-1])]
                got = [tuple(l.weight.shape) for l in cond.layers]
                if got != want:
                    raise TrainUnsupported(f"conditioner weight shapes {got} != {want}")
        plan["train_checked"] = True

    # ---- backward -------------------------------------------------------------------------------------
    def _check_input_grad(self, plan) -> None:
        """d log_prob / dx is served when the first layer of the plan is an affine block that reads the caller's tensor in its
        natural order (what every USFlow layer list gives: [ScaleTransform folded,] BlockAffineTransform first)"""
        first = plan["meta"][0] if plan["meta"] else None
        # ("nat": a zero-padded copy of the caller's rows when D is not a multiple of 4 -- same order)
        if first is None or first["kind"] != "affine" or first["in_buf"] not in ("user_in", "nat") or first["in_layout"] != "nat" \
                or plan.get("planes_train"):
            e = TrainUnsupported("input gradient: the layer list does not start with an affine block on the caller's tensor")
            e.input_grad_only = True            # (parameter-only calls of this flow keep the device path: flows.Flow.log_prob)
            raise e

    def _input_grad(self, plan) -> torch.Tensor:
        """d sum_m g_lp[m] log_prob[m] / dx [B, D] from the gradient the last backward pass left at the first layer's input"""
        g, ld = self._dx
        D = self.eng.D
        B = plan["ws"]["zA"].shape[0]
        # the data-gradient GEMM wrote rows of stride ld, which need not be the buffer's width (LD != LDn at D = 2, 10, 100, ...)
        dx = g.reshape(-1)[:B * ld].view(B, ld)[:, :D]
        sm = plan["meta"][0]["pre_scale"]
        if sm is not None:                                             # x' = x / scale in front of the block (ScaleTransform.backward)
            return dx / sm.scale.detach().to(dx.device, torch.float32).reshape(1, D)
        # autograd may keep what we return (x.grad): never hand out the workspace, which the next pass overwrites
        return dx.clone()

    def backward(self, plan, x, g_lp: torch.Tensor, gsum: Optional[torch.Tensor] = None,
                 into_bound: bool = False, want_dx: bool = False) -> Dict[int, torch.Tensor]:
        """gradients of sum_m g_lp[m] * log_prob(x)[m] w.r.t. every trainable parameter: id(param) -> tensor.

        The launch sequence depends only on the plan: it is recorded on the first call (``_ext.Tape``) and replayed
        afterwards; the per-call inputs (x, g_lp) enter through ``host_op`` closures reading ``self._cur``."""
        dev = x.device
        # gsum: gradient at the log-det output (radial bases: log_prob = f(radius) + logdet, the node returns both);
        # None: log_prob = base(z) + logdet came out of the node itself, so it is sum(g_lp)
        self._cur = dict(x=x, g_lp=g_lp.detach().to(torch.float32).contiguous(),
                         gsum=None if gsum is None else gsum.detach())
        pk = plan["pk"]
        arena = self._arena(plan)
        tkey = "bwd_tape_dx" if want_dx else "bwd_tape"              # (the launch sequence differs: the first layer's data gradient)
        tape = plan.get(tkey)
        usable = _ext.TAPES_ENABLED and pk.get("replayable", False)
        with torch.no_grad():
            if usable and tape is not None and tape.stream == _ext.current_stream(dev) and plan.get(tkey + "_pk") is pk:
                _ext.replay(tape)
            else:
                tape = _ext.Tape() if usable else None
                ps = Pass(self, plan, arena, want_dx)
                body = training_planes.backward_body if plan.get("planes_train") else training_rows.backward_body
                with _ext.record(tape):
                    dx = body(ps)
                if tape is not None:
                    tape.stream = _ext.current_stream(dev)
                    tape.dx = dx
                plan[tkey], plan[tkey + "_pk"], plan["bwd_pass"] = tape, pk, ps
            self._dx = dx if tape is None else tape.dx                 # (a replay writes the same buffer)
            self._last_arena = arena
            if into_bound:
                # the node was built over bound gradients (bind_flat_grads; _LogProbFn took no parameter inputs): what
                # autograd's AccumulateGrad would do per parameter (~290 small adds) is one add over the flat buffer
                gf = self._bound_grads(arena)
                if gf is not None:
                    gf.add_(arena["flat"])
                else:               # the binding went away between forward and backward: per parameter, by hand
                    params = self._arena_params()
                    for pid in arena["touched"]:
                        p, g = params[pid], arena["views"][pid]
                        if p.grad is None:
                            p.grad = g.clone()
                        else:
                            p.grad.add_(g)
                return {}
            flat = arena["flat"].clone()          # autograd may keep what we return: never hand out the arena itself
            self.allreduce_gradients(flat, x.shape[0])
        # parameters the path never reaches (a context layer without context) get no gradient, as under autograd
        out = {pid: flat[o: o + n].view(shape) for pid, (o, n, shape) in arena["slots"].items() if pid in arena["touched"]}
        # the LU factors' gradients leave the chain rule with exact zeros outside their triangles (triu / tril in fp64): LUTransform's
        # mask hooks (transforms.py: one product per factor and pass -- 66 launches of the cfg2 model) skip exactly these tensors
        lu_ids = [id(getattr(lu, nm)) for ch in pk["affine_parts"]["__chunks__"] for lu in ch["lus"] for nm in ("L_raw", "U_raw")]
        masked = [out[i] for i in lu_ids if i in out]
        if masked:
            from .image_training import mark_masked
            mark_masked(masked)
        return out

    # ---- gradients accumulated by one launch ----------------------------------------------------------------
    def _arena_params(self) -> Dict[int, torch.nn.Parameter]:
        ps = list(self.params())
        b = self.flow.base_distribution
        if hasattr(b, "loc") and isinstance(getattr(b, "loc", None), torch.nn.Parameter):
            ps.append(b.loc)
        ps += self.base_extra_params()
        return {id(p): p for p in ps}

    def bind_flat_grads(self) -> bool:
        """Make the ``.grad`` of every parameter this path produces a gradient for a VIEW of one flat fp32 buffer laid
        out like the gradient arena (current values kept).  While the views stay in place (``optimizer.zero_grad(
        set_to_none=True)`` or any reassignment undoes it), ``backward`` adds the whole arena with one launch instead of
        handing ~9 tensors per block to autograd's per-parameter accumulation -- at the reference's batch of 32 rows those
        adds are a tenth of the step.  Flow.fit calls this before it captures the step as a hipGraph and sets
        ``use_bound_node`` for the duration of the captured step only: outside that scope ``log_prob`` stays an ordinary
        autograd node over the parameters (which accumulates into the views in place).  Data-parallel runs stay unbound."""
        ar = self.__dict__.get("_last_arena")
        if ar is None or self.grad_allreduce is not None:
            return False
        params = self._arena_params()
        gf = torch.zeros_like(ar["flat"])
        views = {}
        for pid in ar["touched"]:
            p = params.get(pid)
            if p is None or p.dtype != torch.float32 or p.device != gf.device:
                return False
            o, n, shape = ar["slots"][pid]
            views[pid] = (p, gf[o: o + n].view(shape))
        with torch.no_grad():
            for p, v in views.values():
                if p.grad is not None:
                    v.copy_(p.grad)
                p.grad = v
        self._gflat = gf
        # what the autograd node hangs on while the gradients are bound (its own gradient is a constant zero)
        self._anchor = torch.zeros((), dtype=torch.float32, device=gf.device, requires_grad=True)
        self._anchor_zero = torch.zeros((), dtype=torch.float32, device=gf.device)
        self._gflat_views = {pid: (p, v.data_ptr(), ar["slots"][pid][0]) for pid, (p, v) in views.items()}
        return True

    def grads_bound(self) -> bool:
        """are the parameters' .grad still the views bind_flat_grads made?  (checked when the autograd node is built)"""
        views = self.__dict__.get("_gflat_views")
        if not views or self.grad_allreduce is not None:
            return False
        return all(e[0].grad is not None and e[0].grad.data_ptr() == e[1] for e in views.values())

    def _bound_grads(self, arena) -> Optional[torch.Tensor]:
        gf = self.__dict__.get("_gflat")
        if gf is None or self.grad_allreduce is not None or gf.shape != arena["flat"].shape:
            return None
        views = self._gflat_views
        if len(views) != len(arena["touched"]):
            return None
        for pid in arena["touched"]:
            e = views.get(pid)
            if e is None or e[0].grad is None or e[0].grad.data_ptr() != e[1] or arena["slots"][pid][0] != e[2]:
                return None
        return gf

    def allreduce_gradients(self, flat: torch.Tensor, local_rows: int) -> None:
        """data-parallel training: ONE all-reduce over the flat gradient arena (its last element carries this rank's
        row count).  ``average``: every rank's loss is the MEAN over its own shard, so the global-mean gradient is
        sum_r B_r grad_r / sum_r B_r -- shards of unequal size (a short last batch) are weighted by their row counts and
        an empty shard contributes zeros with weight 0.  Otherwise (losses are sums): the plain sum."""
        if self.grad_allreduce is None:
            return
        import torch.distributed as dist
        group, average = self.grad_allreduce
        if not (dist.is_available() and dist.is_initialized() and
                (dist.get_world_size(group) > 1 or getattr(self, "force_collective", False))):
            return
        if average:
            flat[:-1] *= float(local_rows)
        flat[-1] = float(local_rows)
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
        if average:
            flat[:-1] /= flat[-1].clamp_min(1.0)

    def empty_shard_gradients(self, device) -> Dict[int, torch.Tensor]:
        """a rank whose shard of the batch is empty still has to join the step's collective (the others would hang):
        it contributes a zero arena with weight 0 and receives the same global gradient as every other rank"""
        pk = self.eng.pack(device)
        arena = self._arena(dict(pk=pk, ws=None), device)
        with torch.no_grad():
            flat = torch.zeros_like(arena["flat"])
            self.allreduce_gradients(flat, 0)
        return {pid: flat[o: o + n].view(shape) for pid, (o, n, shape) in arena["slots"].items()}

    def _arena(self, plan, dev=None) -> dict:
        """one flat fp32 buffer for all parameter gradients of this plan; the LU factors' gradients lie batched
        ([n,D,D] L_raw | [n,D,D] U_raw | [n,D] bias, in prepare order) so the chain rule writes each with one copy.
        Its layout depends on the parameter pack only (the same on every rank); one extra element at the end carries
        the rank's row count through the data-parallel all-reduce."""
        ar = plan.get("grad_arena")
        if ar is not None and ar["pk"] is plan["pk"]:
            return ar
        pk = plan["pk"]
        if dev is None:
            dev = plan["ws"]["zA"].device
        slots, off = {}, 0
        lu_views = []
        for ch in pk["affine_parts"]["__chunks__"]:
            n, D = len(ch["lus"]), self.eng.D
            base = off
            for name, per in (("L_raw", D * D), ("U_raw", D * D), ("bias_vector", D)):
                for j, lu in enumerate(ch["lus"]):
                    p = getattr(lu, name)
                    slots[id(p)] = (off + j * per, per, tuple(p.shape))
                off += n * per
            lu_views.append((base, n))
        extra = []
        info = self.flow._base_info(dev)
        if info is not None and info[0] == "radial":
            extra.append(self.flow.base_distribution.loc)
        extra += self.base_extra_params()
        for p in list(self.params()) + extra:
            if id(p) not in slots and p.requires_grad:
                slots[id(p)] = (off, p.numel(), tuple(p.shape))
                off += p.numel()
        flat = torch.zeros(max(off, 1) + 1, dtype=torch.float32, device=dev)
        ar = dict(flat=flat, slots=slots, lu_views=lu_views, pk=pk, touched=set(),
                  views={pid: flat[o: o + n].view(shape) for pid, (o, n, shape) in slots.items()})
        plan["grad_arena"] = ar
        return ar


def _node_forward(ctx, path: TrainPath, x, context, params):
    """what both autograd nodes' forward does: the launch list, and what their backward needs on ctx"""
    ctx.want_dx = bool(ctx.needs_input_grad[1])
    out, plan, xc, gen = path.forward(x, context, want_dx=ctx.want_dx)
    ctx.path, ctx.plan, ctx.x, ctx.context, ctx.gen = path, plan, xc, context, gen
    ctx.params = params
    # bound gradients (TrainPath.bind_flat_grads): the only differentiable input is the path's anchor scalar; backward itself
    # adds the whole arena -- a radial base's loc included -- into the bound .grad views with one launch
    ctx.bound = len(params) == 1 and params[0] is path.__dict__.get("_anchor")
    return out


def _node_backward(ctx, g_out, gsum=None):
    """... and both backwards: gradients for (path, x, context, *params)"""
    path: TrainPath = ctx.path
    path.revalidate(ctx)
    grads = path.backward(ctx.plan, ctx.x, g_out, gsum=gsum, into_bound=ctx.bound, want_dx=ctx.want_dx)
    gx = path._input_grad(ctx.plan).reshape(ctx.x.shape) if ctx.want_dx else None
    if ctx.bound:
        return (None, gx, None, path._anchor_zero)
    return (None, gx, None) + tuple(grads.get(id(p)) if p.requires_grad else None for p in ctx.params)


class _LogProbFn(torch.autograd.Function):
    """``Flow.log_prob`` as one autograd node (forward: launch list; backward: TrainPath.backward)."""

    @staticmethod
    def forward(ctx, path: TrainPath, x, context, *params):
        return _node_forward(ctx, path, x, context, params)

    @staticmethod
    def backward(ctx, g_lp):
        return _node_backward(ctx, g_lp)


class _RadiusFn(torch.autograd.Function):
    """Radial bases: the node returns (r = ||f^-1(x) - loc||_p, log-det); ``RadialDistribution.log_prob``'s finishing
    formula norm_dist.log_prob(r) - log dV_p(r) (distributions.py:506-511) is applied outside, in torch, so a trainable
    norm distribution gets its gradients from autograd and this node's backward starts from d/dr."""

    @staticmethod
    def forward(ctx, path: TrainPath, x, context, *params):
        r = _node_forward(ctx, path, x, context, params)
        return r, ctx.plan["pk"]["ladj_total"].neg32(r.device)

    @staticmethod
    def backward(ctx, g_r, g_logdet):
        if g_r is None:
            g_r = torch.zeros(ctx.x.shape[0], dtype=torch.float32, device=ctx.x.device)
        if g_logdet is None:
            g_logdet = torch.zeros((), dtype=torch.float32, device=ctx.x.device)
        return _node_backward(ctx, g_r, g_logdet)


class _EmptyShardFn(torch.autograd.Function):
    """data-parallel training, this rank's shard is empty: log_prob is an empty tensor, but the backward joins the
    gradient all-reduce (weight 0) so the other ranks do not hang and this replica receives the same gradients"""

    @staticmethod
    def forward(ctx, path: TrainPath, x, *params):
        ctx.path, ctx.params, ctx.dev = path, params, x.device
        return torch.empty(0, dtype=torch.float32, device=x.device)

    @staticmethod
    def backward(ctx, g_lp):
        grads = ctx.path.empty_shard_gradients(ctx.dev)
        return (None, None) + tuple(grads.get(id(p)) if p.requires_grad else None for p in ctx.params)


def log_prob_empty_shard(path: TrainPath, x):
    extra = []
    info = path.flow._base_info(x.device)
    if info is not None and info[0] == "radial":
        extra.append(path.flow.base_distribution.loc)
    return _EmptyShardFn.apply(path, x, *(extra + list(path.params())))


def log_prob_with_grad(path: TrainPath, x, context):
    params = list(path.params())
    info = path.flow._base_info(x.device)
    # (the bound node -- no parameter inputs, the whole arena added into the bound .grad views by one launch -- only inside
    # the scope that asked for it: Flow.fit's captured step sets ``use_bound_node``; anywhere else a grad-enabled log_prob
    # is an ordinary autograd node over the parameters, so torch.autograd.grad / hooks / backward(inputs=...) behave as usual
    # even while the .grad views of an earlier fit are still in place)
    bound = path.__dict__.get("use_bound_node", False) and path.grads_bound() and torch.is_grad_enabled()
    if info[0] == "radial":
        base = path.flow.base_distribution
        if bound:
            r, logdet = _RadiusFn.apply(path, x, context, path._anchor)
        else:
            r, logdet = _RadiusFn.apply(path, x, context, base.loc, *params)
        lp = None
        if config.radial:
            from . import radial
            lp = radial.log_prob_from_radius(base, r)      # (one launch each way, no validating distribution object)
        return (base.log_prob_from_radius(r) if lp is None else lp) + logdet
    if bound:
        return _LogProbFn.apply(path, x, context, path._anchor)
    return _LogProbFn.apply(path, x, context, *(params + path.base_extra_params()))
