"""SRCNN (drop-in for ``climsr.models.srcnn.SRCNN``, srcnn.py:6-18): conv1 9x9 -> ReLU -> conv2 1x1 -> ReLU ->
conv3 5x5.

Two roles:

* ``SRCNNParams`` is the plain parameter container ``ESRGANGenerator`` and ``RCAN`` own for its
  ``srcnn.conv{1,2,3}`` state_dict keys.  The parents flatten / pack its parameters themselves and run the three
  convs inside their own native forward (the ``torch.cat`` of esrgan.py:100 is a channel-packed NHWC buffer), so it
  is inert: no flat buffer of its own, no ``_apply`` override, no forward.
* ``SRCNN`` is the stand-alone generator of the MSE task (``generator_type: "srcnn"``, task.py:141,235-239;
  ``_target_: climsr_amd.models.srcnn.SRCNN``).  ``forward(x)`` takes the fp32 CUDA batch
  ``[n, in_channels, H, W]`` of data/tile_pipeline.py's "srcnn" mode (nearest-upscaled LR at HR size, optionally
  followed by elevation and mask: ``in_channels`` 1, 2 or 3; any H, W >= 1) and returns fp32 ``[n, 1, H, W]``:

  - forward: ``pack_planes8`` (one launch: 8-channel bf16 NHWC, unused channels zero), then csrc/srcnn.hip's
    ``srcnn_tail_kernel`` (the only MFMA launch; the 64- / 32-channel intermediates never leave the chip);
  - backward: ``srcnn_bwd_kernel`` (recomputes the intermediates; writes the conv1 output gradient dz1 and the
    conv2 / conv3 gradients), then conv1's weight gradient (the 9x9 ``in_c <= 4`` path).  The input never needs a
    gradient, so there is no conv1 data-gradient launch;
  - parameters live in one flat fp32 buffer (core/flat.py): the fused AdamW updates it in one launch, and both
    gradient routes (in place into the flat gradient buffer / through autograd under torch DDP) are honoured;
  - chunking: the two kernels use 32-bit buffer offsets (``climsr_srcnn_fwd``: n*H*W*16 B < 2 GiB;
    ``climsr_srcnn_bwd`` and conv1's weight gradient: dz1 = n*H*W*128 B < 2 GiB).  A batch past that is run in
    chunks of whole images along ``n`` (``_max_pixels_per_launch`` pixels each when the backward will follow,
    ``_max_pixels_forward_only`` under no_grad); the first chunk's gradients overwrite or accumulate as the step
    asked, later chunks accumulate.  A single image past the limit raises ``ValueError``.

  ``out_channels != 1`` raises ``NotImplementedError``: the fused kernels are single-output.
"""
from __future__ import annotations

from typing import List, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from ..core.flat import FlatParamsMixin
from ..ops import ConvPlan, SrcnnTail, Workspace, pack_planes8


class SRCNNParams(nn.Module):
    """The reference's three convs under the reference's names (srcnn.py:9-11); run by the owning generator."""

    def __init__(self, in_channels=1, out_channels=1, **kwargs):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channels=in_channels, out_channels=64, kernel_size=9, padding=4)
        self.conv2 = nn.Conv2d(in_channels=64, out_channels=32, kernel_size=1, padding=0)
        self.conv3 = nn.Conv2d(in_channels=32, out_channels=out_channels, kernel_size=5, padding=2)

    def forward(self, x):  # pragma: no cover
        raise RuntimeError("SRCNNParams only holds the srcnn.conv{1,2,3} parameters of ESRGANGenerator / RCAN, which run "
                           "them natively; the stand-alone generator is climsr_amd.models.srcnn.SRCNN")


class _Engine:
    """Native forward/backward of one stand-alone SRCNN (per device)."""

    def __init__(self, net: "SRCNN"):
        self.net = net
        self.convs = [net.conv1, net.conv2, net.conv3]
        self.plans = [ConvPlan(c.in_channels, c.out_channels, c.kernel_size[0], 1, c.padding[0], f"conv{k + 1}")
                      for k, c in enumerate(self.convs)]
        for p, c in zip(self.plans, self.convs):
            p.bind(c.weight, c.bias, need_t=False)  # no data gradient below conv1
        self.tail = SrcnnTail(self.plans, "srcnn")
        self.ws = Workspace()
        self.dz1 = None
        self.version = -1

    def bind_grads(self) -> None:
        for p, c in zip(self.plans, self.convs):
            p.gw, p.gb = c.weight.grad, c.bias.grad

    def repack(self) -> None:
        self.tail.pack()
        self.version = self.net._flat._version

    def ensure_packed(self) -> None:
        if self.net._flat._version != self.version:
            self.repack()

    @staticmethod
    def chunks(n: int, hw: int, limit: int) -> List[Tuple[int, int]]:
        """[i0, i1) image ranges of at most ``limit`` pixels each."""
        if hw > limit:
            raise ValueError(f"SRCNN: one {hw}-pixel image is past the {limit} pixels a single launch addresses "
                             "(32-bit buffer offsets); tile the image")
        per = limit // hw
        return [(i, min(i + per, n)) for i in range(0, n, per)]

    def forward(self, x: Tensor, keep: bool):
        n, c, h, w = x.shape
        net = self.net
        limit = net._max_pixels_per_launch if keep else net._max_pixels_forward_only
        parts = self.chunks(n, h * w, limit)
        self.ensure_packed()
        x = x.contiguous().float()
        xin = torch.empty((n, h, w, 8), dtype=torch.bfloat16, device=x.device)
        pack_planes8([(x, k) for k in range(c)], n, h, w, xin)
        out = torch.empty((n, 1, h, w), dtype=torch.float32, device=x.device)
        for i0, i1 in parts:
            self.tail.fwd(xin[i0:i1], 8, 0, i1 - i0, h, w, out[i0:i1])
        return out, (dict(n=n, h=h, w=w, xin=xin, parts=parts) if keep else None)

    def backward(self, gout: Tensor, sv: dict, accumulate: bool) -> None:
        h, w, xin = sv["h"], sv["w"], sv["xin"]
        gout = gout.contiguous().float()
        nmax = max(i1 - i0 for i0, i1 in sv["parts"])
        if self.dz1 is None or self.dz1.shape != (nmax, h, w, 64) or self.dz1.device != gout.device:
            self.dz1 = torch.empty((nmax, h, w, 64), dtype=torch.bfloat16, device=gout.device)
        conv1 = self.plans[0]
        for k, (i0, i1) in enumerate(sv["parts"]):
            nc, acc = i1 - i0, accumulate or k > 0
            dz1 = self.dz1[:nc]
            # conv3 / conv2 gradients and dz1 in one launch that recomputes the forward, then dW1 / db1 from dz1
            self.tail.bwd(xin[i0:i1], 8, 0, nc, h, w, gout[i0:i1], dz1, self.ws, acc)
            conv1.wgrad(xin[i0:i1], 8, 0, h, w, dz1, 64, nc, self.ws, acc)
        hook = self.net._grad_ready_hook
        if hook is not None:
            hook(0)  # 8k-20k parameters: one bucket, final here


class _SRCNNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, engine_box, *params):
        engine, keep, via_autograd = engine_box  # grad mode is off inside Function.forward: decided by the caller
        out, saved = engine.forward(x, keep=keep)
        ctx.engine = engine
        ctx.saved = saved
        ctx.via_autograd = via_autograd
        return out

    @staticmethod
    def backward(ctx, gout):
        engine = ctx.engine
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("gradient w.r.t. the SRCNN input is not implemented (never needed by the task)")
        if ctx.saved is None:
            raise RuntimeError("SRCNN forward ran without saving activations")
        net = engine.net
        if ctx.via_autograd:  # torch DDP: the gradients go through AccumulateGrad (and the reducer's hooks)
            buf, prev = net._begin_autograd_grads()
            engine.bind_grads()
            engine.backward(gout, ctx.saved, accumulate=False)
            ctx.saved = None
            return (None, None) + net._end_autograd_grads(buf, prev, ctx.needs_input_grad[2:])
        acc = net.grads_as_views()
        engine.bind_grads()
        engine.backward(gout, ctx.saved, accumulate=acc)
        ctx.saved = None
        return (None, None) + tuple(None for _ in range(len(ctx.needs_input_grad) - 2))


class SRCNN(FlatParamsMixin, SRCNNParams):
    """The stand-alone SRCNN generator (see the module docstring)."""

    # pixels (n*H*W) one launch may address: dz1's 128 B / pixel (backward) and the 16 B / pixel input (forward) < 2 GiB
    _max_pixels_per_launch = (1 << 24) - 1
    _max_pixels_forward_only = (1 << 27) - 1

    def __init__(self, in_channels=1, out_channels=1, **kwargs):
        if out_channels != 1:
            raise NotImplementedError(f"stand-alone SRCNN: out_channels={out_channels}; the fused kernels are single-output")
        if in_channels not in (1, 2, 3):
            raise ValueError(f"stand-alone SRCNN: in_channels={in_channels}; the tile pipeline's srcnn batch has 1, 2 or 3 "
                             "(lr [+ elevation] [+ mask])")
        super().__init__(in_channels=in_channels, out_channels=out_channels)
        self.in_channels, self.out_channels = in_channels, out_channels
        self._flatten()
        object.__setattr__(self, "_engine", None)
        object.__setattr__(self, "_grad_ready_hook", None)

    def set_grad_ready_hook(self, fn) -> None:
        """Call ``fn(0)`` once at the end of every backward, when the whole flat gradient buffer is final (one
        bucket for the overlapped DDP all-reduce, core/ddp.OverlappedGradAllReducer); ``fn=None`` removes it."""
        object.__setattr__(self, "_grad_ready_hook", fn)

    def _on_flat_moved(self):
        object.__setattr__(self, "_engine", None)

    def engine(self) -> _Engine:
        self._ensure_flat()
        if self._engine is None or self._engine.net is not self:
            object.__setattr__(self, "_engine", _Engine(self))
        return self._engine

    def repack_weights(self) -> None:
        """Refresh the bf16 MFMA weight layout after an in-place update of the fp32 master weights."""
        self.engine().repack()

    def forward(self, x: Tensor) -> Tensor:
        if not x.is_cuda:
            raise RuntimeError("climsr_amd.SRCNN runs on the GPU only (no CPU fallback); move it with .cuda()")
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise ValueError(f"SRCNN: expected [n, {self.in_channels}, H, W], got {tuple(x.shape)}")
        eng = self.engine()
        params = [p for p, _o, _n in self._flat_index]
        keep = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        return _SRCNNFn.apply(x, (eng, keep, keep and self._route_grads_through_autograd()), *params)
