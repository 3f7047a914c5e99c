"""Fused AdamW (+ device-side OneCycleLR for captured steps) over flat parameter buffers.

Replaces ``torch.optim.AdamW`` (conf/optimizers/adamw.yaml: lr, weight_decay=1e-4, betas
(0.9,0.999) with beta1 cycled by OneCycleLR, eps 1e-8) wired by
``climsr/core/instantiator.py:48-49`` and ``OneCycleLR`` (conf/schedulers/one_cycle_schedule.yaml,
instantiator.py:51-64).  One kernel updates a whole network's flat fp32 buffer.
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

    def __init__(self, params: Iterable, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 amsgrad: bool = False, owner=None, **kwargs):
        if amsgrad:
            raise ValueError("amsgrad is not supported")
        for k, v in kwargs.items():
            if k not in self._UNSUPPORTED:
                raise TypeError(f"AdamW got an unexpected keyword argument {k!r}")
            if v != self._UNSUPPORTED[k]:
                raise ValueError(f"AdamW option {k}={v!r} is not supported by the fused update (only {self._UNSUPPORTED[k]!r})")
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
                raise ValueError(f"AdamW.load_state_dict: group {gi} carries flat-buffer moments but its parameters are "
                                 "not the views of one flat buffer")
            if not isinstance(st.get("step"), int) or st["step"] < 1:
                raise ValueError(f"AdamW.load_state_dict: group {gi} has moments but step={st.get('step')!r}")
            for k in ("m", "v"):
                t = st.get(k)
                if not isinstance(t, torch.Tensor) or t.shape != flat.shape or t.dtype != flat.dtype or not t.is_contiguous():
                    got = f"{tuple(t.shape)} {t.dtype} contiguous={t.is_contiguous()}" if isinstance(t, torch.Tensor) else repr(t)
                    raise ValueError(f"AdamW.load_state_dict: group {gi} moment {k!r} is {got}; the flat parameter buffer "
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
                _adamw_flat(lib, self.owner, flat, gflat, st["m"], st["v"], hp, _lib.stream_ptr(), grad_scale)
                mirrored = True
            else:
                for p in params:
                    ps = self.state[p]
                    if "m" not in ps:
                        ps["m"] = torch.zeros_like(p)
                        ps["v"] = torch.zeros_like(p)
                    g = p.grad.contiguous()
                    if grad_scale is not None:
                        g = g.clone() if g.data_ptr() == p.grad.data_ptr() else g  # .grad stays unclipped
                        _launch("grad_scale", lambda: lib.climsr_scale_f32(ptr(g), g.numel(), ptr(grad_scale), _lib.stream_ptr()),
                                nbytes=8 * g.numel())
                    _launch("adamw", lambda: lib.climsr_adamw_step(p.numel(), ptr(p), ptr(g), ptr(ps["m"]), ptr(ps["v"]), ptr(hp),
                                                                   _lib.stream_ptr()), nbytes=28 * p.numel())
        if self.owner is not None:
            if mirrored and _mirror_of(self.owner) is not None:
                self.owner.repack_weights(mirror_done=True)
            else:
                self.owner.repack_weights()
        return loss


def _mirror_of(module):
    """(offset, numel, bf16 buffer) of a weight the module reads as a bf16 copy of its flat buffer, or None."""
    fn = getattr(module, "bf16_mirror", None)
    return fn() if fn is not None else None


def _adamw_flat(lib, module, flat, gflat, m, v, hp, stream, grad_scale=None):
    """One fused AdamW launch over a flat buffer; when ``module`` mirrors part of it in bf16 (``bf16_mirror()``), the
    same pass writes that copy.  ``grad_scale`` (device scalar): the update reads gradient * grad_scale."""
    mir = _mirror_of(module) if module is not None else None
    if grad_scale is not None:
        lo, n, buf = mir if mir is not None else (0, 0, None)
        _launch("adamw_scaled", lambda: lib.climsr_adamw_step_scaled(flat.numel(), ptr(flat), ptr(gflat), ptr(m), ptr(v), ptr(hp),
                                                                     ptr(grad_scale), lo, n, ptr(buf), stream),
                nbytes=28 * flat.numel() + 2 * n)
    elif mir is None:
        _launch("adamw", lambda: lib.climsr_adamw_step(flat.numel(), ptr(flat), ptr(gflat), ptr(m), ptr(v), ptr(hp), stream),
                nbytes=28 * flat.numel())
    else:
        lo, n, buf = mir
        _launch("adamw", lambda: lib.climsr_adamw_step_mirror(flat.numel(), ptr(flat), ptr(gflat), ptr(m), ptr(v), ptr(hp), lo, n,
                                                              ptr(buf), stream), nbytes=28 * flat.numel() + 2 * n)


class GraphedAdamW:
    """AdamW + OneCycleLR with all scalars on the device, for hipGraph-captured training steps.

    ``step()`` launches: schedule kernel (lr, beta1, bias corrections from a device step counter),
    the fused update over the flat buffer, and the bf16 weight repack.  With ``max_grad_norm`` it first takes the L2
    norm of the flat gradient (``GradNorm``) and the update reads the gradient times the device-side clip coefficient.  Semantics equal
    torch AdamW stepped before OneCycleLR.step() each iteration (Lightning interval="step").
    """

    def __init__(self, module, lr: float = 1e-4, total_steps: int = 1000, weight_decay: float = 1e-4, pct_start: float = 0.05,
                 div_factor: float = 2.0, final_div_factor: float = 100.0, betas=(0.9, 0.999), eps: float = 1e-8,
                 max_grad_norm: Optional[float] = None):
        self.module = module
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"max_grad_norm must be positive, got {max_grad_norm!r}")
        self.max_grad_norm = max_grad_norm
        self.grad_norm = GradNorm(module) if max_grad_norm is not None else None
        if self.grad_norm is not None:
            self.grad_norm._prepare(_lib.load())  # offsets table and workspace now: step() may run inside a capture
        flat = module._flat
        self.m = torch.zeros_like(flat)
        self.v = torch.zeros_like(flat)
        self.state = torch.zeros(2, dtype=torch.float64, device=flat.device)
        self.hp = torch.zeros(8, dtype=torch.float32, device=flat.device)
        self.cfg = (int(total_steps), float(lr), float(pct_start), float(div_factor), float(final_div_factor), float(betas[1]),
                    float(eps), float(weight_decay))

    def step(self):
        lib = _lib.load()
        s = _lib.stream_ptr()
        ts, lr, pct, div, fdiv, b2, eps, wd = self.cfg
        _launch("adamw_hparams", lambda: lib.climsr_adamw_hparams(ptr(self.state), ts, lr, pct, div, fdiv, b2, eps, wd, ptr(self.hp),
                                                                  s))
        flat = self.module._flat
        coef = None
        if self.grad_norm is not None:  # L2 norm of the flat gradient -> clip coefficient, kept on the device
            coef = self.grad_norm(2, self.max_grad_norm, gathered=True)[2]
        _adamw_flat(lib, self.module, flat, self.module._flat_grad, self.m, self.v, self.hp, s, coef)
        if _mirror_of(self.module) is not None:
            self.module.engine().repack(mirror_done=True)
        else:
            self.module.engine().repack()
