"""Adam / AdamW and ``clip_grad_norm_`` on the device path -- SURVEY row N2: most of the reference's experiment files name
``torch.optim.Adam`` with a ``weight_decay`` (``HyperoptExperiment._trial`` hands the class to ``Flow.fit``,
explib/hyperopt.py:108-114), and ``gradient_clip`` is an argument of its ``fit`` (flows.py:120, 201-202).

``Adam`` / ``AdamW`` are torch's classes -- constructor, ``param_groups``, per-parameter state (``step`` as a CPU fp32 scalar,
``exp_avg``, ``exp_avg_sq``, ``max_exp_avg_sq``) and ``state_dict()`` are theirs, interchangeable both ways -- whose ``step()``
sends all contiguous fp32 device tensors of a parameter group through ONE launch of ``usf_adam_step_f32`` (a device table
of chunks as SophiaG's; torch's single-tensor operation order; 28 bytes per parameter and step).  What makes the step
replayable as a hipGraph by ``Flow.fit``: the step count t of the bias corrections 1 - beta^t lives in a device counter
that the launch itself advances (torch's non-capturable form turns t into Python floats, which a capture would freeze);
``note_graph_replays`` keeps the host ``state['step']`` equal to it.  Everything else -- CPU tensors, non-contiguous or
non-fp32 tensors, a tensor ``lr``, ``capturable`` / ``differentiable`` / ``fused=True`` / ``foreach=True`` -- is handed to
torch's own arithmetic, so on a CPU the classes ARE torch's.

``GradClip`` is ``torch.nn.utils.clip_grad_norm_(params, max_norm)`` (2-norm, ``error_if_nonfinite=False``) in two
launches over a gradient-only chunk table, without a host synchronisation: any optimiser's step stays capturable behind it.
"""
from typing import List, Optional

import numpy as np
import torch
from torch.optim.adam import adam as _torch_adam

from ._abi import AdamChunk, GradChunk
from ._mt_tables import CHUNK, ChunkTables, chunk_rows, param_capacity


def _is_number(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _group_supported(group) -> bool:
    """the options of a parameter group that the kernel implements (torch's defaults but for foreach=None, which only
    chooses between torch's own implementations)"""
    return (not group.get("capturable") and not group.get("differentiable") and not group.get("fused")
            and not group.get("foreach") and _is_number(group["lr"]) and _is_number(group["eps"])
            and _is_number(group["weight_decay"]) and all(_is_number(b) for b in group["betas"]))


class _KernelAdam(ChunkTables):
    """the device ``step`` of ``Adam`` / ``AdamW`` below (a mixin in front of torch's class)"""

    _chunk_struct = AdamChunk
    _ROW = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("vmax", "<u8"), ("n", "<i4"), ("slot", "<i4")])

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.reset_tables()

    def __setstate__(self, state):
        super().__setstate__(state)
        self.reset_tables()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self.reset_tables()             # (the step counters on the device are copies of the host's: upload them again)

    # ---- which tensors the kernel serves ----
    def _on_hip(self, p, amsgrad: bool) -> bool:
        if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.grad is not None and not p.grad.is_sparse
                and p.grad.dtype == torch.float32 and p.grad.is_contiguous() and p.grad.device == p.device):
            return False
        st = self.state.get(p)
        if not st:
            return True                 # (state not created yet: torch's initialisation gives contiguous fp32 zeros_like)
        names = ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if amsgrad else ())
        return (torch.is_tensor(st.get("step")) and not st["step"].is_cuda
                and all(torch.is_tensor(st.get(k)) and st[k].device == p.device and st[k].dtype == torch.float32
                        and st[k].is_contiguous() for k in names))

    def _split(self, group):
        """the group's parameters with a gradient: (those for the kernel, those for torch's arithmetic)"""
        hip, rest = [], []
        for p in group["params"]:
            if p.grad is not None:
                (hip if self._on_hip(p, group["amsgrad"]) else rest).append(p)
        return hip, rest

    def _init_state(self, group, ps):
        """torch's lazy state initialisation (and its checks) for the parameters ``ps`` of ``group``; the lists of
        torch.optim.adam.adam's positional arguments"""
        lists = [[] for _ in range(6)]
        has_complex = self._init_group({**group, "params": ps}, *lists)
        return lists, has_complex

    # ---- ChunkTables ----
    def _table_key(self, gi: int, ps: List[torch.Tensor]):
        amsgrad = self.param_groups[gi]["amsgrad"]
        bases = [(p.data_ptr(), p.grad.data_ptr(), self.state[p]["exp_avg"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr(),
                  self.state[p]["max_exp_avg_sq"].data_ptr() if amsgrad else 0) for p in ps]

        def build():
            # one device counter per distinct step count: parameters of a group that have taken different numbers of
            # steps (one had no gradient for a while) keep torch's per-parameter bias corrections
            slots, rows = {}, []
            for p, b in zip(ps, bases):
                t = int(self.state[p]["step"].item())
                slot = slots.setdefault(t, len(slots))
                rows += chunk_rows(b, p.numel(), (slot,))
            return np.array(rows, dtype=self._ROW), torch.tensor(list(slots), dtype=torch.int64), None
        return (amsgrad, tuple(bases)), build

    def _table_capacity(self):
        return param_capacity(self.param_groups, lambda rows, tensors: 8 * tensors)

    def _table_members(self):
        out = []
        if all(_group_supported(g) for g in self.param_groups):
            for gi, group in enumerate(self.param_groups):
                hip, _ = self._split(group)
                self._init_state(group, hip)
                out.append((gi, hip))
        return out

    # ---- the step ----
    def step(self, closure=None):
        if not all(_group_supported(g) for g in self.param_groups) or \
                not any(self._split(g)[0] for g in self.param_groups):
            return super().step(closure)          # torch's own step, bit for bit (every CPU model)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        with torch.no_grad():
            self._device_step()
        return loss

    def _device_step(self) -> None:
        from . import _ext
        _ext.load()                               # no silent fallback on a GPU box
        capturing = torch.cuda.is_current_stream_capturing()
        for gi, group in enumerate(self.param_groups):
            beta1, beta2 = group["betas"]
            common = dict(amsgrad=group["amsgrad"], beta1=beta1, beta2=beta2, lr=group["lr"], weight_decay=group["weight_decay"],
                          eps=group["eps"], maximize=group["maximize"])
            hip, rest = self._split(group)
            if rest:
                if capturing:
                    raise RuntimeError("usflows_amd.optim: a parameter that is not a contiguous fp32 device tensor takes torch's "
                                       "Adam arithmetic, whose host-side step count cannot be captured")
                lists, has_complex = self._init_state(group, rest)
                _torch_adam(*lists, foreach=group["foreach"], capturable=False, differentiable=False, fused=group["fused"],
                            has_complex=has_complex, decoupled_weight_decay=group["decoupled_weight_decay"], **common)
            if not hip:
                continue
            self._init_state(group, hip)
            _, dev, n, steps, _ = self._table(gi, hip)
            _ext.adam_step(dev, n, steps, lr=group["lr"], beta1=beta1, beta2=beta2, eps=group["eps"],
                           weight_decay=group["weight_decay"], maximize=group["maximize"], amsgrad=group["amsgrad"],
                           decoupled=group["decoupled_weight_decay"])
            if capturing:
                continue            # nothing ran: the launches were recorded, and every replay is reported to note_graph_replays
            for p in hip:
                self.state[p]["step"] += 1
                torch.autograd.graph.increment_version(p)    # the kernel wrote through raw pointers
        return None


class Adam(_KernelAdam, torch.optim.Adam):
    """``torch.optim.Adam`` whose step runs as one HIP launch per parameter group on a ROCm device (module docstring)"""


class AdamW(_KernelAdam, torch.optim.AdamW):
    """``torch.optim.AdamW`` (decoupled weight decay), likewise"""


def adopt(optim) -> Optional[torch.optim.Optimizer]:
    """The optimiser ``Flow.fit`` steps with in place of ``optim``: ``optim`` itself when it is one of this package's;
    for an instance of exactly ``torch.optim.Adam`` / ``torch.optim.AdamW`` with options the kernel implements, an
    ``Adam`` / ``AdamW`` that SHARES its ``param_groups`` and ``state`` (stepping either moves both); None otherwise."""
    from .sophia import SophiaG
    if isinstance(optim, (_KernelAdam, SophiaG)):
        return optim
    cls = {torch.optim.Adam: Adam, torch.optim.AdamW: AdamW}.get(type(optim))
    if cls is None or not all(_group_supported(g) for g in optim.param_groups):
        return None
    if getattr(optim, "grad_scale", None) is not None or getattr(optim, "found_inf", None) is not None:
        return None
    ours = cls.__new__(cls)
    ours.__dict__.update(optim.__dict__)          # param_groups, state, defaults and hooks: the same objects
    ours._patch_step_function()
    ours.reset_tables()
    return ours


class GradClip(ChunkTables):
    """``torch.nn.utils.clip_grad_norm_(params, max_norm)`` (2-norm, error_if_nonfinite=False), called once per step
    between backward and ``optim.step()``.  Contiguous fp32 device gradients: ``usf_grad_sqnorm_partials_f32`` +
    ``usf_grad_clip_scale_f32`` over one table of all of them; anything else: torch's function."""

    _chunk_struct = GradChunk
    _ROW = np.dtype([("g", "<u8"), ("n", "<i4"), ("r", "<i4")])

    def __init__(self, params, max_norm: float):
        self.params = [p for p in params]
        self.max_norm = float(max_norm)
        self.reset_tables()

    def _grads(self):
        grads = [p.grad for p in self.params if p.grad is not None]
        ok = bool(grads) and all(g.is_cuda and g.dtype == torch.float32 and not g.is_sparse and g.is_contiguous()
                                 and g.device == grads[0].device for g in grads)
        return grads, ok

    def _table_key(self, gi: int, grads):
        bases = [(g.data_ptr(),) for g in grads]

        def build():
            rows = [r for g, b in zip(grads, bases) for r in chunk_rows(b, g.numel(), (0,))]
            return np.array(rows, dtype=self._ROW), torch.zeros(len(rows), dtype=torch.float64), None
        return tuple(bases), build

    def _table_capacity(self):
        ps = [p for p in self.params if p.is_cuda and p.dtype == torch.float32 and p.requires_grad]
        rows = sum((p.numel() + CHUNK - 1) // CHUNK for p in ps)
        return {0: (rows, 8 * rows, ps[0].device)} if rows else {}

    def _table_members(self):
        grads, ok = self._grads()
        return [(0, grads)] if ok else []

    @torch.no_grad()
    def __call__(self) -> None:
        grads, ok = self._grads()
        if not grads:
            return
        if not ok:
            torch.nn.utils.clip_grad_norm_(self.params, self.max_norm)
            return
        from . import _ext
        _ext.load()
        _, dev, n, partials, _ = self._table(0, grads)
        _ext.grad_clip(dev, n, partials, self.max_norm)
