"""Fused AdamW (+ device-side OneCycleLR for captured steps) over flat parameter buffers.

Replaces ``torch.optim.AdamW`` (conf/optimizers/adamw.yaml: lr, weight_decay=1e-4, betas
(0.9,0.999) with beta1 cycled by OneCycleLR, eps 1e-8) wired by
``climsr/core/instantiator.py:48-49`` and ``OneCycleLR`` (conf/schedulers/one_cycle_schedule.yaml,
instantiator.py:51-64).  One kernel updates a whole network's flat fp32 buffer.

``Adam`` is the same for ``torch.optim.Adam`` (conf/optimizers/adam.yaml: coupled L2 weight decay), and ``DeviceStepped``
turns an eager (``AdamW`` | ``Adam``, scheduler or None) pair into the form a captured step replays: counters, schedule
(OneCycleLR, none, or one of five transformers warm-up lambdas: ``climsr_opt_hparams``) and update all on the device.
"""
from __future__ import annotations

from typing import Iterable, List, Optional

import torch

from .. import _lib
from .._lib import ptr
from ..ops import _launch


def _flat_owner(params: List[torch.Tensor]):
    """If params are exactly the views of one flat buffer in order, return (flat, flat_grad_base_check)."""
    if not params:
        return None
    base = params[0]
    st = base.untyped_storage()
    off = base.storage_offset()
    for p in params:
        if p.untyped_storage().data_ptr() != st.data_ptr() or p.storage_offset() != off or p.dtype != torch.float32:
            return None
        off += p.numel()
    if off != st.nbytes() // 4:
        return None
    return torch.empty(0, dtype=torch.float32, device=base.device).set_(st, 0, (off,))


def _gather_flat_grad(own, flat, params):
    """The one flat tensor holding the gradients of ``params`` (the views of ``flat``, in order), or None.  When the
    gradients already are the views of one buffer that buffer is returned as it is.  Gradients delivered through
    autograd as separate tensors (torch DDP; a module called twice sums its nodes' gradients out of place) are gathered
    into the owning module's flat gradient buffer with one multi-tensor copy, which keeps the one-launch update."""
    gflat = _flat_owner([p.grad for p in params])
    if gflat is None and own is not None and getattr(own, "_flat", None) is not None and \
            own._flat.data_ptr() == flat.data_ptr() and own._flat.numel() == flat.numel():
        views = [own._flat_grad[off:off + n].view(p.shape) for p, off, n in own._flat_index]
        torch._foreach_copy_(views, [p.grad for p in params])
        gflat = own._flat_grad
    return gflat


def flat_grad(module) -> torch.Tensor:
    """``module._flat_grad`` holding the module's current gradients: as it stands when every ``param.grad`` views it,
    after one multi-tensor gather otherwise (``_gather_flat_grad``).  Every parameter must have a gradient."""
    params = [p for p, _o, _n in module._flat_index]
    if any(p.grad is None for p in params):
        raise RuntimeError("flat_grad: a parameter has no gradient (run a backward first)")
    gflat = _gather_flat_grad(module, module._flat, params)
    if gflat is None or gflat.data_ptr() != module._flat_grad.data_ptr():
        # views of some other flat buffer (or no flat layout): copy into the module's own
        views = [module._flat_grad[off:off + n].view(p.shape) for p, off, n in module._flat_index]
        torch._foreach_copy_(views, [p.grad for p in params])
    return module._flat_grad


_NORM_KINDS = {"l2": 0, 2: 0, 2.0: 0, "2": 0, "2.0": 0, "inf": 1, float("inf"): 1}


class GradNorm:
    """Per-parameter and total gradient norms of one native module, from one segmented reduction over its flat
    gradient buffer (``climsr_grad_norm``: three launches whatever the parameter count, fp64, deterministic).

    Caches the device offsets table (from ``module._flat_index``), the workspace and the outputs; calling it returns
    ``(per_parameter_norms, total, coefficient, finite)`` as views of those cached device tensors (float64 [nparams],
    float64 0-d, float32 0-d, float32 0-d), valid until the next call -- clone what must outlive it.  No host sync."""

    def __init__(self, module):
        if not hasattr(module, "_flat_index") or not hasattr(module, "_flat_grad"):
            raise TypeError(f"GradNorm needs a native flat-parameter module, got {type(module).__name__}")
        self.module = module
        self._grad_ptr = None

    @classmethod
    def of(cls, module) -> "GradNorm":
        gn = getattr(module, "_grad_norm_cache", None)
        if gn is None:
            gn = cls(module)
            object.__setattr__(module, "_grad_norm_cache", gn)
        return gn

    def _prepare(self, lib):
        g = self.module._flat_grad
        if self._grad_ptr == (g.data_ptr(), g.numel()):
            return
        if not g.is_cuda:
            raise RuntimeError("GradNorm is GPU only: the module's flat gradient buffer is on " + str(g.device))
        offs = [off for _p, off, _n in self.module._flat_index] + [g.numel()]
        self.nseg = len(offs) - 1
        self.seg_off = torch.tensor(offs, dtype=torch.int64).to(g.device)
        self.workspace = torch.empty(lib.climsr_grad_norm_workspace(g.numel(), self.nseg), dtype=torch.uint8, device=g.device)
        self.norms = torch.zeros(self.nseg + 1, dtype=torch.float64, device=g.device)
        self.clip = torch.ones(2, dtype=torch.float32, device=g.device)
        self._grad_ptr = (g.data_ptr(), g.numel())

    def __call__(self, kind=2, max_norm: float = 0.0, gathered: bool = False):
        if kind not in _NORM_KINDS:
            raise ValueError(f"GradNorm: norm kind {kind!r} is not 2 or 'inf'")
        lib = _lib.load()
        self._prepare(lib)
        g = self.module._flat_grad if gathered else flat_grad(self.module)
        _launch("grad_norm", lambda: lib.climsr_grad_norm(ptr(g), g.numel(), ptr(self.seg_off), self.nseg, _NORM_KINDS[kind],
                                                          float(max_norm or 0.0), ptr(self.workspace), ptr(self.norms),
                                                          ptr(self.clip), _lib.stream_ptr()), nbytes=4 * g.numel())
        return self.norms[:self.nseg], self.norms[self.nseg], self.clip[0], self.clip[1]


def clip_grad_norm_(module, max_norm: float) -> torch.Tensor:
    """``torch.nn.utils.clip_grad_norm_`` (L2) for a native module: one norm pass over the flat gradient buffer, then
    one in-place scale of it by the device-side coefficient min(1, max_norm / (total + 1e-6)).  Afterwards every
    ``param.grad`` is the clipped gradient (a view of the flat buffer).  Returns the total norm before clipping as a
    0-d float64 device tensor; no host sync."""
    if not max_norm > 0:
        raise ValueError(f"clip_grad_norm_: max_norm must be positive, got {max_norm!r}")
    _per, total, coef, _finite = GradNorm.of(module)(2, max_norm)
    total = total.clone()
    scale_grad_(module, coef)
    return total


def scale_grad_(module, coef: torch.Tensor) -> None:
    """The module's flat gradient buffer times a float32 device scalar, in place (``climsr_scale_f32``); afterwards every
    ``param.grad`` views that buffer.  Call after ``GradNorm`` / ``flat_grad`` (the buffer holds the gradients)."""
    lib = _lib.load()
    g = module._flat_grad
    _launch("grad_scale", lambda: lib.climsr_scale_f32(ptr(g), g.numel(), ptr(coef), _lib.stream_ptr()), nbytes=8 * g.numel())
    module.grads_as_views()  # gathered gradients: .grad now reads the clipped buffer


class AdamW(torch.optim.Optimizer):
    """Drop-in for torch.optim.AdamW (amsgrad=False) whose update runs in libclimsr_hip.

    Hyper-parameters are read from ``param_groups`` at every step, so torch's own
    ``OneCycleLR`` (which cycles lr and betas[0]) drives it unchanged.  When the params are the
    views of one flat buffer (climsr_amd modules) the whole group is one launch; the module's
    bf16 weight layouts are refreshed through ``owner.repack_weights()`` when given.
    """

    # torch.optim.AdamW options this fused update does not implement: accepted only at their default value
    _UNSUPPORTED = {"maximize": False, "foreach": None, "fused": None, "capturable": False, "differentiable": False}
    _COUPLED = False  # True (Adam): the weight decay is an L2 term added to the gradient, not a decay of the weights

    def __init__(self, params: Iterable, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 amsgrad: bool = False, owner=None, **kwargs):
        if amsgrad:
            raise ValueError("amsgrad is not supported")
        for k, v in kwargs.items():
            if k not in self._UNSUPPORTED:
                raise TypeError(f"{type(self).__name__} got an unexpected keyword argument {k!r}")
            if v != self._UNSUPPORTED[k]:
                raise ValueError(f"{type(self).__name__} option {k}={v!r} is not supported by the fused update (only {self._UNSUPPORTED[k]!r})")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.owner = owner
        self._hp = None

    def load_state_dict(self, state_dict) -> None:
        """``torch.optim.Optimizer.load_state_dict`` copies the flat update's state (string keys ``"group%d"``: step, m,
        v) as it is, on whatever device the file was read to -- and the kernel takes raw pointers.  So every group's m
        and v are checked against the group's flat parameter buffer (shape, dtype, contiguity: ``ValueError``) and moved
        to its device here, before any step."""
        super().load_state_dict(state_dict)
        for gi, group in enumerate(self.param_groups):
            st = self.state.get("group%d" % gi)
            if not st or ("m" not in st and "v" not in st):
                continue
            flat = _flat_owner(group["params"])
            if flat is None:
                raise ValueError(f"{type(self).__name__}.load_state_dict: group {gi} carries flat-buffer moments but its parameters are "
                                 "not the views of one flat buffer")
            if not isinstance(st.get("step"), int) or st["step"] < 1:
                raise ValueError(f"{type(self).__name__}.load_state_dict: group {gi} has moments but step={st.get('step')!r}")
            for k in ("m", "v"):
                t = st.get(k)
                if not isinstance(t, torch.Tensor) or t.shape != flat.shape or t.dtype != flat.dtype or not t.is_contiguous():
                    got = f"{tuple(t.shape)} {t.dtype} contiguous={t.is_contiguous()}" if isinstance(t, torch.Tensor) else repr(t)
                    raise ValueError(f"{type(self).__name__}.load_state_dict: group {gi} moment {k!r} is {got}; the flat parameter buffer "
                                     f"is {tuple(flat.shape)} {flat.dtype}")
                st[k] = t.to(flat.device, copy=True)  # never the caller's tensor: the update writes it in place

    def _hparams(self, group, step: int, device) -> torch.Tensor:
        """The kernel's scalars {lr, beta1, beta2, eps, wd, lr / bc1, sqrt(bc2), 0} for this group's ``step``-th update."""
        lr = group["lr"]
        b1, b2 = group["betas"]
        bc1 = 1 - b1 ** step
        bc2 = 1 - b2 ** step
        return torch.tensor([lr, b1, b2, group["eps"], group["weight_decay"], lr / bc1, bc2 ** 0.5, 0.0],
                            dtype=torch.float32).to(device, non_blocking=True)

    @torch.no_grad()
    def step(self, closure=None, grad_scale: Optional[torch.Tensor] = None):
        """``grad_scale``: a float32 device scalar (the clip coefficient) the update multiplies every gradient by while
        it reads it -- no extra pass over the gradients, which are left as they are.  None: the plain update."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        mirrored = False
        for group in self.param_groups:
            params = [p for p in group["params"] if p.grad is not None]
            if not params:
                continue
            st = self.state.setdefault("group%d" % self.param_groups.index(group), {})
            step = st.get("step", 0) + 1
            st["step"] = step
            hp = self._hparams(group, step, params[0].device)
            flat = _flat_owner(group["params"]) if len(params) == len(group["params"]) else None
            if flat is not None:
                gflat = _gather_flat_grad(self.owner, flat, group["params"])
                if gflat is None:
                    flat = None
            if flat is not None:
                if "m" not in st:
                    st["m"] = torch.zeros_like(flat)
                    st["v"] = torch.zeros_like(flat)
                _adamw_flat(lib, self.owner, flat, gflat, st["m"], st["v"], hp, _lib.stream_ptr(), grad_scale, self._COUPLED)
                mirrored = True
            else:
                for p in params:
                    ps = self.state[p]
                    if "m" not in ps:
                        ps["m"] = torch.zeros_like(p)
                        ps["v"] = torch.zeros_like(p)
                    # with grad_scale the scaled entry only reads the gradient: .grad stays unclipped
                    _adamw_flat(lib, None, p, p.grad.contiguous(), ps["m"], ps["v"], hp, _lib.stream_ptr(), grad_scale, self._COUPLED)
        if self.owner is not None:
            _repack_after(self.owner, mirrored)
        return loss


def _mirror_of(module):
    """(offset, numel, bf16 buffer) of a weight the module reads as a bf16 copy of its flat buffer, or None."""
    fn = getattr(module, "bf16_mirror", None)
    return fn() if fn is not None else None


def _repack_after(module, mirrored: bool = True) -> None:
    """Re-pack ``module``'s bf16 weight layouts after an update; ``mirrored``: ``_adamw_flat`` wrote its bf16 mirror."""
    if mirrored and _mirror_of(module) is not None:
        module.repack_weights(mirror_done=True)
    else:
        module.repack_weights()


def _adamw_flat(lib, module, p, g, m, v, hp, stream, grad_scale=None, coupled=False):
    """One fused update launch over ``p`` (a network's flat buffer, or one parameter with ``module`` None); when
    ``module`` mirrors part of the buffer in bf16 (``bf16_mirror()``), the same pass writes that copy.  ``grad_scale``
    (device scalar): the update reads gradient * grad_scale and leaves the gradient as it is.  ``coupled``: the Adam
    update (L2 term in the gradient) instead of AdamW's.  The only caller of the library's ``climsr_*_step*`` entries."""
    mir = _mirror_of(module) if module is not None else None
    lo, mn, buf = mir if mir is not None else (0, 0, None)
    n = p.numel()
    args = (n, ptr(p), ptr(g), ptr(m), ptr(v), ptr(hp))
    window = (lo, mn, ptr(buf), stream)
    if grad_scale is not None:
        label, fn = ("adam_scaled", lib.climsr_adam_step_scaled) if coupled else ("adamw_scaled", lib.climsr_adamw_step_scaled)
        args += (ptr(grad_scale),) + window
    elif coupled:
        label, fn, args = "adam", lib.climsr_adam_step, args + window
    elif mir is not None:
        label, fn, args = "adamw", lib.climsr_adamw_step_mirror, args + window
    else:
        label, fn, args = "adamw", lib.climsr_adamw_step, args + (stream,)
    _launch(label, lambda: fn(*args), nbytes=28 * n + 2 * mn)


class _DeviceStep:
    """An optimizer step with every scalar on the device, so that a captured hipGraph replays it: what ``GraphedAdamW``
    and ``DeviceStepped`` share.  ``step()`` launches the schedule kernel (``_launch_schedule``: lr, betas and bias
    corrections from the device counters ``state``, which it advances, into the ``hp`` row), with ``max_grad_norm`` the
    L2 norm of the flat gradient (``_grads``) giving the device clip coefficient, the fused update reading it, and the
    bf16 re-pack.  It returns that coefficient (or None), allocates nothing and reads nothing back."""

    def __init__(self, module, m, v, state, coupled: bool, max_grad_norm: Optional[float], grad_norm: Optional[GradNorm]):
        self.module, self.m, self.v, self.state, self.coupled = module, m, v, state, coupled
        self.hp = torch.zeros(8, dtype=torch.float32, device=module._flat.device)
        self.max_grad_norm, self.grad_norm = max_grad_norm, grad_norm

    @staticmethod
    def _clip_norm(module, max_grad_norm, gn_of) -> Optional[GradNorm]:
        """The ``GradNorm`` (``gn_of(module)``) a step clipping at ``max_grad_norm`` needs; None without clipping."""
        if max_grad_norm is None:
            return None
        if not max_grad_norm > 0:
            raise ValueError(f"max_grad_norm must be positive, got {max_grad_norm!r}")
        gn = gn_of(module)
        if module._flat.is_cuda:
            gn._prepare(_lib.load())  # offsets table and workspace now: step() may run inside a capture
        return gn

    # subclasses: _launch_schedule(lib, stream) launches the schedule kernel on self.state / self.hp; _grads() returns
    # (the flat gradient tensor, whether it is module._flat_grad already holding the gradients)

    def step(self):
        lib = _lib.load()
        s = _lib.stream_ptr()
        self._launch_schedule(lib, s)
        gflat, gathered = self._grads()
        coef = None
        if self.grad_norm is not None:  # L2 norm of the flat gradient -> clip coefficient, kept on the device
            coef = self.grad_norm(2, self.max_grad_norm, gathered=gathered)[2]
        _adamw_flat(lib, self.module, self.module._flat, gflat, self.m, self.v, self.hp, s, coef, self.coupled)
        _repack_after(self.module)
        return coef


class GraphedAdamW(_DeviceStep):
    """AdamW + OneCycleLR with all scalars on the device, for hipGraph-captured training steps (``bench.py``'s step).

    ``step()`` is ``_DeviceStep``'s with ``climsr_adamw_hparams`` as the schedule kernel and ``module._flat_grad`` taken
    as it stands (no per-step host work).  Semantics: torch AdamW stepped before OneCycleLR.step() each iteration."""

    def __init__(self, module, lr: float = 1e-4, total_steps: int = 1000, weight_decay: float = 1e-4, pct_start: float = 0.05,
                 div_factor: float = 2.0, final_div_factor: float = 100.0, betas=(0.9, 0.999), eps: float = 1e-8,
                 max_grad_norm: Optional[float] = None):
        flat = module._flat
        super().__init__(module, torch.zeros_like(flat), torch.zeros_like(flat), torch.zeros(2, dtype=torch.float64, device=flat.device),
                         False, max_grad_norm, self._clip_norm(module, max_grad_norm, GradNorm))
        self.cfg = (int(total_steps), float(lr), float(pct_start), float(div_factor), float(final_div_factor), float(betas[1]),
                    float(eps), float(weight_decay))

    def _launch_schedule(self, lib, stream) -> None:
        ts, lr, pct, div, fdiv, b2, eps, wd = self.cfg
        _launch("adamw_hparams", lambda: lib.climsr_adamw_hparams(ptr(self.state), ts, lr, pct, div, fdiv, b2, eps, wd, ptr(self.hp),
                                                                  stream))

    def _grads(self):
        return self.module._flat_grad, True


class Adam(AdamW):
    """Drop-in for torch.optim.Adam (amsgrad=False; conf/optimizers/adam.yaml: coupled L2 ``weight_decay``) whose update
    runs in libclimsr_hip (``climsr_adam_step`` / ``climsr_adam_step_scaled``).  Everything else is ``AdamW``'s:
    ``param_groups`` read at every step, flat m / v in ``state["group%d"]``, ``step(grad_scale=)``, the re-pack."""

    _COUPLED = True

    def __init__(self, params: Iterable, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 amsgrad: bool = False, owner=None, **kwargs):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, owner=owner, **kwargs)


# ---------------------------------------------------------------------------------------------------------------------
# Schedules the device can step (climsr_opt_hparams), restated in float64 Python.  ``lr_lambda`` is transformers' own
# formula per kind; ``onecycle_lr_beta1`` is torch's OneCycleLR (cos annealing, two phases, beta1 cycled).
# ---------------------------------------------------------------------------------------------------------------------
SCHED_ONECYCLE, SCHED_NONE, SCHED_CONSTANT, SCHED_CONSTANT_WARMUP, SCHED_LINEAR_WARMUP, SCHED_COSINE_WARMUP, \
    SCHED_COSINE_RESTARTS_WARMUP = range(7)

_TRANSFORMERS_LAMBDAS = {  # the lambda's function name (transformers >= 4.30) / its factory's name (older closures)
    "_get_constant_lambda": SCHED_CONSTANT, "get_constant_schedule": SCHED_CONSTANT,
    "_get_constant_schedule_with_warmup_lr_lambda": SCHED_CONSTANT_WARMUP, "get_constant_schedule_with_warmup": SCHED_CONSTANT_WARMUP,
    "_get_linear_schedule_with_warmup_lr_lambda": SCHED_LINEAR_WARMUP, "get_linear_schedule_with_warmup": SCHED_LINEAR_WARMUP,
    "_get_cosine_schedule_with_warmup_lr_lambda": SCHED_COSINE_WARMUP, "get_cosine_schedule_with_warmup": SCHED_COSINE_WARMUP,
    "_get_cosine_with_hard_restarts_schedule_with_warmup_lr_lambda": SCHED_COSINE_RESTARTS_WARMUP,
    "get_cosine_with_hard_restarts_schedule_with_warmup": SCHED_COSINE_RESTARTS_WARMUP,
}


def lr_lambda(kind: int, step: int, warmup: float = 0.0, total: float = 0.0, cycles: float = 0.5) -> float:
    """lambda(step) of a ``SCHED_*`` kind other than OneCycleLR, in float64, as transformers/optimization.py writes it
    (``warmup`` may be fractional: the host lambdas use the task's un-rounded warm-up product as it is)."""
    import math

    if kind in (SCHED_NONE, SCHED_CONSTANT):
        return 1.0
    if step < warmup:
        return float(step) / float(max(1.0, warmup))
    if kind == SCHED_CONSTANT_WARMUP:
        return 1.0
    if kind == SCHED_LINEAR_WARMUP:
        return max(0.0, float(total - step) / float(max(1.0, total - warmup)))
    progress = float(step - warmup) / float(max(1.0, total - warmup))
    if kind == SCHED_COSINE_WARMUP:
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * float(cycles) * 2.0 * progress)))
    if kind == SCHED_COSINE_RESTARTS_WARMUP:
        if progress >= 1.0:
            return 0.0
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * ((float(cycles) * progress) % 1.0))))
    raise ValueError(f"lr_lambda: unknown schedule kind {kind!r}")


def onecycle_lr_beta1(step: int, total_steps: int, max_lr: float, pct_start: float, div_factor: float, final_div_factor: float,
                      base_momentum: float = 0.85, max_momentum: float = 0.95):
    """(lr, beta1) of torch's OneCycleLR at ``last_epoch == step`` (anneal_strategy "cos", three_phase False)."""
    import math

    def cos_anneal(start, end, pct):
        return end + (start - end) / 2.0 * (math.cos(math.pi * pct) + 1)

    initial_lr = max_lr / div_factor
    min_lr = initial_lr / final_div_factor
    end0, end1 = float(pct_start * total_steps) - 1, total_steps - 1
    if step <= end0:
        pct = step / end0
        return cos_anneal(initial_lr, max_lr, pct), cos_anneal(max_momentum, base_momentum, pct)
    pct = (step - end0) / (end1 - end0)
    return cos_anneal(max_lr, min_lr, pct), cos_anneal(base_momentum, max_momentum, pct)


def _solve(fn, want: float, guess: float) -> Optional[float]:
    """A float x near ``guess`` with fn(x) == want exactly (the scheduler keeps fn's value, the kernel wants x)."""
    import math

    cands = [float(f"{guess:.12g}"), guess]  # the short decimal the user most likely wrote, first
    lo = hi = guess
    for _ in range(4):
        lo, hi = math.nextafter(lo, -math.inf), math.nextafter(hi, math.inf)
        cands += [lo, hi]
    for x in cands:
        if fn(x) == want:
            return x
    return None


def _describe_schedule(optimizer, scheduler):
    """(kind, dict of climsr_opt_hparams' schedule scalars) of a scheduler the device can step, else NotImplementedError."""
    pair = f"({type(optimizer).__name__}, {type(scheduler).__name__ if scheduler is not None else None})"
    if scheduler is None:
        return SCHED_NONE, {}
    if getattr(scheduler, "optimizer", None) is not optimizer:
        raise NotImplementedError(f"the pair {pair} cannot be stepped on the device: the scheduler drives another optimizer")
    group = optimizer.param_groups[0]
    if isinstance(scheduler, torch.optim.lr_scheduler.OneCycleLR):
        anneal = getattr(scheduler, "_anneal_func_type", None) or \
            {"_annealing_cos": "cos", "_annealing_linear": "linear"}.get(getattr(scheduler._anneal_func, "__name__", ""), "?")
        odd = []
        if anneal != "cos":
            odd.append(f"anneal_strategy={anneal!r}")
        if len(scheduler._schedule_phases) != 2:
            odd.append("three_phase=True")
        if not (scheduler.cycle_momentum and getattr(scheduler, "use_beta1", False)):
            odd.append("cycle_momentum=False")
        elif (group["base_momentum"], group["max_momentum"]) != (0.85, 0.95):
            odd.append(f"base_momentum={group['base_momentum']!r}, max_momentum={group['max_momentum']!r}")
        if odd:
            raise NotImplementedError(f"the pair {pair} cannot be stepped on the device: OneCycleLR with {', '.join(odd)} "
                                      "(only cos annealing in two phases with beta1 cycled 0.95 <-> 0.85)")
        total, max_lr = int(scheduler.total_steps), float(group["max_lr"])
        end0 = scheduler._schedule_phases[0]["end_step"]
        pct = _solve(lambda x: float(x * total) - 1, end0, (end0 + 1) / total)
        div = _solve(lambda x: max_lr / x, group["initial_lr"], max_lr / group["initial_lr"])
        fdiv = None if div is None else _solve(lambda x: max_lr / div / x, group["min_lr"], group["initial_lr"] / group["min_lr"])
        if pct is None or div is None or fdiv is None:
            raise NotImplementedError(f"the pair {pair} cannot be stepped on the device: OneCycleLR's pct_start, div_factor "
                                      "or final_div_factor could not be recovered from the scheduler exactly")
        return SCHED_ONECYCLE, dict(lr=max_lr, total=float(total), pct_start=pct, div_factor=div, final_div_factor=fdiv)
    if isinstance(scheduler, torch.optim.lr_scheduler.LambdaLR) and len(scheduler.lr_lambdas) == 1:
        fn = scheduler.lr_lambdas[0]
        inner = getattr(fn, "func", fn)
        kw = dict(getattr(fn, "keywords", None) or {})
        if getattr(inner, "__closure__", None):  # older transformers: a closure over the factory's arguments
            kw.update({k: c.cell_contents for k, c in zip(inner.__code__.co_freevars, inner.__closure__)})
        name = getattr(inner, "__qualname__", "").split(".<locals>")[0]
        kind = _TRANSFORMERS_LAMBDAS.get(name) if str(getattr(inner, "__module__", "")).startswith("transformers") else None
        if kind is not None and not kw.get("min_lr_rate"):
            sc = dict(warmup=float(kw.get("num_warmup_steps", 0.0)), total=float(kw.get("num_training_steps", 0.0)),
                      cycles=float(kw.get("num_cycles", 0.5)))
            probe = sorted({0, 1, int(sc["warmup"]), int(sc["warmup"]) + 1, int(sc["total"]) // 2, max(0, int(sc["total"]) - 1)})
            if sc["warmup"] >= 0.0 and all(abs(fn(s) - lr_lambda(kind, s, **sc)) <= 1e-15 for s in probe):
                return kind, dict(sc, lr=float(scheduler.base_lrs[0]))
    raise NotImplementedError(f"the pair {pair} cannot be stepped on the device: only no scheduler, OneCycleLR and transformers' "
                              "constant, constant / linear / cosine / cosine-with-hard-restarts warm-up schedules are "
                              "implemented (the polynomial schedule stays on the eager path)")


class DeviceStepped(_DeviceStep):
    """The device-stepped form of an eager ``(optimizer, scheduler or None)`` pair, for captured training steps:
    ``core.optim.AdamW`` / ``Adam`` under every schedule ``climsr_opt_hparams`` knows.

    ``step()`` is ``_DeviceStep``'s with ``climsr_opt_hparams`` as the schedule kernel and the gradients gathered into
    the network's flat gradient buffer when autograd delivered them apart.  m and v are the eager optimizer's own
    tensors, the counters start from its ``state["group0"]["step"]`` and the scheduler's ``last_epoch``, and ``flush()``
    writes them back to the host objects with one host read, after which those are what the eager pair would be.
    A pair it cannot express raises ``NotImplementedError`` naming the pair."""

    def __init__(self, optimizer, scheduler=None, max_grad_norm: Optional[float] = None):
        pair = f"({type(optimizer).__name__}, {type(scheduler).__name__ if scheduler is not None else None})"
        if type(optimizer) not in (AdamW, Adam):
            raise NotImplementedError(f"the pair {pair} cannot be stepped on the device: only climsr_amd.core.optim.AdamW and "
                                      "Adam (the fused updates over a flat parameter buffer) are implemented")
        module = optimizer.owner
        if len(optimizer.param_groups) != 1 or module is None or getattr(module, "_flat", None) is None or \
                [id(p) for p in optimizer.param_groups[0]["params"]] != [id(p) for p, _o, _n in module._flat_index]:
            raise NotImplementedError(f"the pair {pair} cannot be stepped on the device: the optimizer must hold the "
                                      "parameters of one native flat-parameter network in one group")
        self.kind, self.sched_cfg = _describe_schedule(optimizer, scheduler)
        grad_norm = self._clip_norm(module, max_grad_norm, GradNorm.of)
        self.optimizer, self.scheduler = optimizer, scheduler
        flat = module._flat
        st = optimizer.state.setdefault("group0", {})
        if "m" not in st:
            st["m"], st["v"] = torch.zeros_like(flat), torch.zeros_like(flat)
        last_epoch = scheduler.last_epoch if scheduler is not None else 0
        state = torch.tensor([float(st.get("step", 0)), float(last_epoch)], dtype=torch.float64).to(flat.device)
        super().__init__(module, st["m"], st["v"], state, optimizer._COUPLED, max_grad_norm, grad_norm)

    def zero_grad(self, set_to_none: bool = True) -> None:
        self.optimizer.zero_grad(set_to_none=set_to_none)

    def _launch_schedule(self, lib, stream) -> None:
        group, c = self.optimizer.param_groups[0], self.sched_cfg
        b1, b2 = group["betas"]
        lr = c.get("lr", group["lr"])  # a scheduler's base / max lr; without one the group's current lr
        _launch("opt_hparams", lambda: lib.climsr_opt_hparams(
            ptr(self.state), self.kind, float(lr), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
            c.get("warmup", 0.0), c.get("total", 0.0), c.get("cycles", 0.0), c.get("pct_start", 0.0), c.get("div_factor", 0.0),
            c.get("final_div_factor", 0.0), ptr(self.hp), stream))

    def _grads(self):
        module = self.module
        flat = module._flat
        if flat.numel() != self.m.numel() or flat.device != self.m.device:
            raise RuntimeError("DeviceStepped: the network's flat parameter buffer changed size or device; build the "
                               "optimizers again")
        gflat = _gather_flat_grad(module, flat, self.optimizer.param_groups[0]["params"])
        if gflat is None:
            raise RuntimeError("DeviceStepped.step: a parameter has no gradient in the network's flat gradient buffer")
        return gflat, gflat.data_ptr() == module._flat_grad.data_ptr()

    def flush(self) -> None:
        """The device counters into the host objects (one host read): the optimizer's step count, the scheduler's
        ``last_epoch`` / ``_step_count`` / ``_last_lr`` and ``param_groups[0]["lr"]`` / ``"betas"`` -- through the
        scheduler's own ``get_lr()``, so they are what its ``step()`` would have left."""
        step, last_epoch = (int(x) for x in self.state.tolist())
        st = self.optimizer.state["group0"]
        st["step"] = step
        st["m"], st["v"] = self.m, self.v
        if step == 0:  # nothing stepped yet: a state without moments, as the eager optimizer's
            del st["m"], st["v"], st["step"]
        sch = self.scheduler
        if sch is None or sch.last_epoch == last_epoch:
            return
        sch.last_epoch = last_epoch
        sch._step_count = last_epoch + 1
        with torch.optim.lr_scheduler._enable_get_lr_call(sch):
            values = sch.get_lr()  # OneCycleLR also writes betas[0] here
        for group, lr in zip(self.optimizer.param_groups, values):
            group["lr"] = lr
        sch._last_lr = [group["lr"] for group in self.optimizer.param_groups]
