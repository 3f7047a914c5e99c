"""The one base of the natively trained modules (ESRGANGenerator, TrainableRCAN, SRCNN and the two discriminators).

* ``NativeFn`` is the only autograd node: ``NativeFn.apply(box, *inputs, *params)``.  Its backward chooses the gradient
  route (in place into the flat gradient buffer, or through autograd under torch DDP: core/flat.py) and turns
  ``grads_as_views()`` into "overwrite or accumulate".
* ``NativeModule`` (on top of ``FlatParamsMixin``) owns the engine and the grad-ready hook: ``engine()``,
  ``repack_weights()``, ``set_grad_ready_hook(fn)`` with one bucket, and ``_native_forward(*inputs)``, the body of every
  ``forward``.  A network declares its engine class, whether it returns an input gradient, and its message texts.
* ``NativeEngine`` is what an engine (the launches of one network on one device) starts from.  The protocol the node
  relies on:

  - ``run(*inputs, keep, need_w) -> (out, saved)``: the forward; ``saved`` is None unless ``keep``;
  - ``bind_grads()``: point the plans at the parameters' current ``.grad`` tensors;
  - ``backward(gout, saved, need_w, need_x, accumulate) -> dx or None``: parameter gradients into the bound tensors
    (= or += with ``accumulate``) when ``need_w``, the gradient of input 0 when ``need_x``;
  - ``pack(**kw)``: refresh the bf16 MFMA weight layouts from the fp32 master weights.

  One re-pack rule for all: ``ensure_packed()`` (first thing in ``run``) re-packs when ``_params_version()`` moved,
  i.e. after any in-place torch write to the flat buffer or through a parameter (``load_state_dict``), or a re-homed
  buffer.  Updates that bypass torch's counters (the fused AdamW writes through the C ABI) call ``repack()`` themselves.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from ..ops import Workspace, nchw_to_nhwc, pack_planes8
from .flat import FlatParamsMixin


def bf16(shape, dev) -> Tensor:
    return torch.empty(shape, dtype=torch.bfloat16, device=dev)


def f32(shape, dev) -> Tensor:
    return torch.empty(shape, dtype=torch.float32, device=dev)


def pack_input8(x: Tensor, cpad: int) -> Tensor:
    """[n,c,H,W] -> bf16 NHWC with ``cpad`` channels (a multiple of 8), the padding channels zero."""
    n, c, h, w = x.shape
    x = x.contiguous().float()
    if cpad == 8:  # the channels and the zero padding in one full-pixel pass
        out = bf16((n, h, w, 8), x.device)
        pack_planes8([(x, k) for k in range(c)], n, h, w, out)
    else:
        out = torch.zeros((n, h, w, cpad), dtype=torch.bfloat16, device=x.device)
        nchw_to_nhwc(x, out, cpad, 0)
    return out


class NativeEngine:
    """Per-device state of one module's native forward / backward (see the module docstring for the protocol)."""

    def __init__(self, owner: "NativeModule"):
        self.owner = owner
        self.device = owner._flat.device
        self.ws = Workspace()
        self.scratch: Dict[str, Tensor] = {}  # also ops.bn_workspace's cache
        self.bound: List[Tuple[object, nn.Module]] = []  # (ConvPlan, its conv module) for bind_grads()
        self.version = None

    def buf(self, key: str, shape, dtype, dev, zero: bool = False) -> Tensor:
        """A scratch tensor kept between calls under ``key``; (re)allocated, zero-filled with ``zero``, when the shape
        or the device changed."""
        t = self.scratch.get(key)
        if t is None or tuple(t.shape) != tuple(shape) or t.device != dev:
            t = torch.zeros(shape, dtype=dtype, device=dev) if zero else torch.empty(shape, dtype=dtype, device=dev)
            self.scratch[key] = t
        return t

    def _params_version(self):
        # the parameters are .data views of the flat buffer with version counters of their own: load_state_dict's
        # copy_ (any in-place write through a parameter) bumps those and leaves the flat buffer's where it was
        o = self.owner
        return o._flat._version, o._flat.data_ptr(), sum(p._version for p, _o, _n in o._flat_index)

    def pack(self) -> None:
        raise NotImplementedError

    def repack(self, **kw) -> None:
        self.pack(**kw)
        self.version = self._params_version()

    def ensure_packed(self) -> None:
        if self._params_version() != self.version:
            self.repack()

    def bind_grads(self) -> None:
        for plan, conv in self.bound:
            plan.gw = conv.weight.grad
            plan.gb = conv.bias.grad if conv.bias is not None else None

    def grads_final(self) -> None:
        """End of a backward that filled the whole flat gradient buffer: the one-bucket grad-ready hook."""
        hook = self.owner._grad_ready_hook
        if hook is not None:
            hook(0)


class NativeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, box, *args):
        engine, n_in, keep, need_w, via_autograd = box  # grad mode is off inside Function.forward: decided by the caller
        out, saved = engine.run(*args[:n_in], keep=keep, need_w=need_w)
        ctx.engine, ctx.n_in, ctx.saved, ctx.via_autograd = engine, n_in, saved, via_autograd
        return out

    @staticmethod
    def backward(ctx, gout):
        engine, n_in = ctx.engine, ctx.n_in
        owner = engine.owner
        need_x = any(ctx.needs_input_grad[1:1 + n_in])
        needs_p = ctx.needs_input_grad[1 + n_in:]
        need_w = any(needs_p)
        if need_x and not owner._input_grad:
            raise NotImplementedError(f"gradient w.r.t. the {owner._label} input{'s' if n_in > 1 else ''} is not implemented "
                                      "(never needed by the task)")
        if ctx.saved is None:
            raise RuntimeError(f"{owner._label} forward ran without saving activations")
        if need_w and ctx.via_autograd:  # torch DDP: the gradients go through AccumulateGrad (and the reducer's hooks)
            buf, prev = owner._begin_autograd_grads()
            engine.bind_grads()
            dx = engine.backward(gout, ctx.saved, need_w, need_x, False)
            slots = owner._end_autograd_grads(buf, prev, needs_p)
        else:
            acc = owner.grads_as_views() if need_w else True
            engine.bind_grads()
            dx = engine.backward(gout, ctx.saved, need_w, need_x, acc)
            slots = (None,) * len(needs_p)
        ctx.saved = None
        return (None, dx) + (None,) * (n_in - 1) + slots


class NativeModule(FlatParamsMixin):
    """Mixin for nn.Module subclasses that run as one ``NativeFn`` node; call ``_flatten()`` at the end of ``__init__``."""

    _engine_cls: type = NativeEngine
    _input_grad = False  # whether the backward returns the gradient of input 0 (else asking for one raises)
    _label = "module"  # in the node's error messages
    _gpu_only_msg = "this module runs on the GPU only (no CPU fallback)"
    _device_type = "cuda"
    _engine_dies_on_apply = False  # engines that also hold buffers (BN running statistics) are rebuilt after any _apply
    _engine: Optional[NativeEngine] = None
    _grad_ready_hook = None

    def set_grad_ready_hook(self, fn) -> None:
        """Call ``fn(0)`` once at the end of every backward, when the whole flat gradient buffer is final (one bucket
        for the overlapped DDP all-reduce, core/ddp.OverlappedGradAllReducer); ``fn=None`` removes it."""
        object.__setattr__(self, "_grad_ready_hook", fn)

    def _on_flat_moved(self) -> None:
        object.__setattr__(self, "_engine", None)

    def _apply(self, fn, recurse=True):
        ret = super()._apply(fn, recurse)
        if self._engine_dies_on_apply:
            object.__setattr__(self, "_engine", None)
        return ret

    def engine(self) -> NativeEngine:
        """The engine, rebuilt only when the flat buffer moved, the device changed or it belongs to another module
        (a captured optimizer step holds ``engine().repack``, so it must stay the same object across steps)."""
        self._ensure_flat()
        eng = self._engine
        if eng is None or eng.owner is not self or eng.device != self._flat.device:
            eng = self._engine_cls(self)
            object.__setattr__(self, "_engine", eng)
        return eng

    def repack_weights(self, **kw) -> None:
        """Refresh the bf16 MFMA weight layouts after an in-place update of the fp32 master weights."""
        self.engine().repack(**kw)

    def _native_forward(self, *inputs: Tensor) -> Tensor:
        if inputs[0].device.type != self._device_type:
            raise RuntimeError(self._gpu_only_msg)
        eng = self.engine()
        params = [p for p, _o, _n in self._flat_index]
        grad_on = torch.is_grad_enabled()
        need_w = grad_on and any(p.requires_grad for p in params)
        keep = need_w or (grad_on and self._input_grad and any(x.requires_grad for x in inputs))
        box = (eng, len(inputs), keep, need_w, need_w and self._route_grads_through_autograd())
        return NativeFn.apply(box, *inputs, *params)
