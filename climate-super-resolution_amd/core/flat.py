"""Flat parameter / gradient storage for the native modules.

Every trainable parameter of a native module is a view into ONE contiguous fp32 buffer, and its
``.grad`` is a view into ONE contiguous fp32 gradient buffer.  The HIP backward writes gradients
straight into that buffer (no per-parameter autograd accumulation), the fused AdamW updates the
whole buffer in one launch, and the data-parallel all-reduce sends it in a few large RCCL buckets.
``state_dict`` keys and shapes stay identical to the reference (the views are ordinary Parameters).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
import torch.nn as nn


def ddp_forward_active() -> bool:
    """True while a ``torch.nn.parallel.DistributedDataParallel`` forward runs (torch marks the wrapping module for the
    duration of its ``_run_ddp_forward``): the native modules then hand their parameter gradients to autograd, whose
    AccumulateGrad nodes fire DDP's reducer hooks (Lightning ``accelerator: ddp``, conf/trainer/benchmark.yaml:4)."""
    try:
        from torch.nn.parallel import DistributedDataParallel as DDP
    except ImportError:  # pragma: no cover
        return False
    fn = getattr(DDP, "_get_active_ddp_module", None)
    return (fn() if fn is not None else getattr(DDP, "_active_ddp_module", None)) is not None


class FlatParamsMixin:
    """Mixin for nn.Module subclasses; call ``_flatten()`` at the end of ``__init__``."""

    _flat: torch.Tensor
    _flat_grad: torch.Tensor
    _flat_index: List[Tuple[nn.Parameter, int, int]]
    # How a native backward delivers parameter gradients.  False: written in place into the flat gradient buffer that
    # every ``param.grad`` views (one buffer for the fused AdamW / bucketed all-reduce; autograd sees no parameter
    # gradient, so no AccumulateGrad node runs).  True: written into a fresh flat buffer whose views are returned to
    # autograd (AccumulateGrad steals them when ``param.grad`` is None, adds them otherwise, and runs its hooks — what
    # torch DDP's reducer needs).  None (default): True only inside a DistributedDataParallel forward.
    grads_through_autograd: Optional[bool] = None

    def _flatten(self) -> None:
        params = [p for p in self.parameters()]
        total = sum(p.numel() for p in params)
        dev = params[0].device if params else torch.device("cpu")
        flat = torch.empty(total, dtype=torch.float32, device=dev)
        index = []
        off = 0
        for p in params:
            n = p.numel()
            flat[off:off + n].copy_(p.data.reshape(-1))
            index.append((p, off, n))
            off += n
        object.__setattr__(self, "_flat", flat)
        object.__setattr__(self, "_flat_grad", torch.zeros(total, dtype=torch.float32, device=dev))
        object.__setattr__(self, "_flat_index", index)
        self._rebind()

    def _rebind(self) -> None:
        for p, off, n in self._flat_index:
            p.data = self._flat[off:off + n].view(p.shape)

    def _flat_intact(self) -> bool:
        base = self._flat.data_ptr()
        for p, off, n in self._flat_index:
            if p.data_ptr() != base + 4 * off or p.dtype != torch.float32 or p.device != self._flat.device:
                return False
        return True

    def _ensure_flat(self) -> None:
        """Re-home parameters into the flat buffer if something replaced their storage."""
        if self._flat_intact():
            return
        dev = self._flat_index[0][0].device if self._flat_index else self._flat.device
        total = self._flat.numel()
        flat = torch.empty(total, dtype=torch.float32, device=dev)
        for p, off, n in self._flat_index:
            flat[off:off + n].copy_(p.data.reshape(-1).to(torch.float32))
        object.__setattr__(self, "_flat", flat)
        object.__setattr__(self, "_flat_grad", torch.zeros(total, dtype=torch.float32, device=dev))
        self._rebind()
        self._on_flat_moved()

    def _on_flat_moved(self) -> None:  # core/native.NativeModule drops its engine (the device plans) here
        pass

    def _apply(self, fn, recurse=True):  # keep the flat layout across .to()/.cuda()
        ret = super()._apply(fn, recurse)  # type: ignore[misc]
        if getattr(self, "_flat_index", None):
            self._ensure_flat()
        return ret

    def _route_grads_through_autograd(self) -> bool:
        """Decided at forward time (the node remembers it): see ``grads_through_autograd``."""
        v = self.grads_through_autograd
        return ddp_forward_active() if v is None else bool(v)

    def _begin_autograd_grads(self):
        """Point every ``param.grad`` at a fresh flat buffer for one native backward (overwrite semantics); returns
        (buffer, the previous grads) for ``_end_autograd_grads``.  The overlapped flat-buffer reducer
        (core/ddp.OverlappedGradAllReducer) reads ``_flat_grad`` through the grad-ready hook, which this route does not
        fill: the two gradient routes are exclusive."""
        if getattr(self, "_grad_ready_hook", None) is not None:
            raise RuntimeError("a grad-ready hook (the flat-buffer DDP reducer) is installed, but this backward hands its "
                               "gradients to autograd (torch DDP): use one data-parallel route, not both")
        buf = torch.empty_like(self._flat_grad)
        saved = [p.grad for p, _o, _n in self._flat_index]
        for p, off, n in self._flat_index:
            p.grad = buf[off:off + n].view(p.shape)
        return buf, saved

    def _end_autograd_grads(self, buf, saved, needs) -> tuple:
        """Restore the previous ``param.grad`` objects and return the fresh buffer's views (None where the parameter
        needs no gradient), in flat order = the order the native Functions receive the parameters."""
        for (p, _o, _n), g in zip(self._flat_index, saved):
            p.grad = g
        return tuple(buf[off:off + n].view(p.shape) if need else None for (p, off, n), need in zip(self._flat_index, needs))

    def grads_as_views(self) -> bool:
        """Point every param.grad at its slice of the flat grad buffer.  Returns True if they
        already were (=> backward accumulates), False if (re)linked (=> backward overwrites)."""
        base = self._flat_grad.data_ptr()
        linked = True
        for p, off, n in self._flat_index:
            g = p.grad
            if g is None or g.data_ptr() != base + 4 * off:
                linked = False
                break
        if not linked:
            for p, off, n in self._flat_index:
                p.grad = self._flat_grad[off:off + n].view(p.shape)
        return linked
