"""SRCNN (drop-in for ``climsr.models.srcnn.SRCNN``, srcnn.py:6-18): conv1 9x9 -> ReLU -> conv2 1x1 -> ReLU ->
conv3 5x5.

Two roles:

* ``SRCNNParams`` is the plain parameter container ``ESRGANGenerator`` and ``RCAN`` own for its
  ``srcnn.conv{1,2,3}`` state_dict keys.  The parents flatten / pack its parameters themselves and run the three
  convs inside their own native forward through ``srcnn_tail_fwd`` / ``srcnn_tail_bwd`` below (the ``torch.cat`` of
  esrgan.py:100 is a channel-packed NHWC buffer), so it is inert: no flat buffer of its own, no ``_apply`` override,
  no forward.
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
    gradient routes (in place into the flat gradient buffer / through autograd under torch DDP) are honoured by the
    shared autograd node (core/native.py);
  - chunking: the two kernels use 32-bit buffer offsets (``climsr_srcnn_fwd``: n*H*W*16 B < 2 GiB;
    ``climsr_srcnn_bwd`` and conv1's weight gradient: dz1 = n*H*W*128 B < 2 GiB).  A batch past that is run in
    chunks of whole images along ``n`` (``_max_pixels_per_launch`` pixels each when the backward will follow,
    ``_max_pixels_forward_only`` under no_grad); the first chunk's gradients overwrite or accumulate as the step
    asked, later chunks accumulate.  A single image past the limit raises ``ValueError``.

  ``out_channels != 1`` raises ``NotImplementedError``: the fused kernels are single-output.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from ..core.native import NativeEngine, NativeModule, bf16, f32, pack_input8
from ..ops import ACT_RELU, OUT_F32, ConvPlan, SrcnnTail, Workspace, nchw_to_nhwc


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


def srcnn_tail_fwd(P: Dict[str, ConvPlan], last: str, feat: Tensor, feat_cs: int, n: int, hh: int, ww: int, oc: int, elev: Tensor,
                   mask: Tensor, fused: Optional[SrcnnTail] = None):
    """The tail of ESRGANGenerator and RCAN: conv ``last`` into channels [0, oc) of an 8-channel buffer, elev / mask after
    them (the torch.cat of esrgan.py:100 / rcan.py:190), then SRCNN (srcnn.py:13-18) with fused ReLUs: one ``fused``
    launch when given (its backward recomputes relu(conv1) / relu(conv2) from the buffer), else conv by conv.
    Returns (out, the 8-channel buffer, relu(conv1), relu(conv2)), the last two None with ``fused``."""
    dev = feat.device
    tail = torch.zeros((n, hh, ww, 8), dtype=torch.bfloat16, device=dev)
    P[last].fwd(feat, feat_cs, 0, hh, ww, tail, 8, 0, n)
    nchw_to_nhwc(elev.contiguous().float(), tail, 8, oc)
    nchw_to_nhwc(mask.contiguous().float(), tail, 8, oc + 1)
    if fused is not None:
        out = f32((n, oc, hh, ww), dev)
        fused.fwd(tail, 8, 0, n, hh, ww, out)
        return out, tail, None, None
    s1 = bf16((n, hh, ww, 64), dev)
    P["srcnn.conv1"].fwd(tail, 8, 0, hh, ww, s1, 64, 0, n, act=ACT_RELU)
    s2 = bf16((n, hh, ww, 32), dev)
    P["srcnn.conv2"].fwd(s1, 64, 0, hh, ww, s2, 32, 0, n, act=ACT_RELU)
    out = f32((n, oc, hh, ww), dev)
    if oc == 1:
        P["srcnn.conv3"].fwd(s2, 32, 0, hh, ww, out, 1, 0, n, out_mode=OUT_F32)
    else:
        tmp = f32((n, hh, ww, oc), dev)
        P["srcnn.conv3"].fwd(s2, 32, 0, hh, ww, tmp, oc, 0, n, out_mode=OUT_F32)
        out.copy_(tmp.permute(0, 3, 1, 2))
    return out, tail, s1, s2


def srcnn_tail_bwd(P: Dict[str, ConvPlan], fused: Optional[SrcnnTail], tail: Tensor, n: int, hh: int, ww: int, gout: Tensor,
                   dzA: Tensor, dz8: Tensor, ws: Workspace, acc: bool) -> None:
    """Backward of that tail down to d(out) in channel 0 of ``dz8``.  ``fused``: the conv3 / conv2 gradients and conv1's
    output gradient (into ``dzA``) in one launch that recomputes the forward, and ``dz8`` must come zeroed (its channels
    1..7 are never written: elev / mask take no gradient).  Without it the caller has filled ``dzA`` conv by conv."""
    if fused is not None:
        fused.bwd(tail, 8, 0, n, hh, ww, gout, dzA, ws, acc)
    P["srcnn.conv1"].wgrad(tail, 8, 0, hh, ww, dzA, 64, n, ws, acc)
    P["srcnn.conv1"].dgrad(dzA, 64, hh, ww, dz8, 8, 0, n, cout_t=1)


class _Engine(NativeEngine):
    """Native forward/backward of one stand-alone SRCNN (per device)."""

    def __init__(self, net: "SRCNN"):
        super().__init__(net)
        self.net = net
        convs = [net.conv1, net.conv2, net.conv3]
        self.plans = [ConvPlan(c.in_channels, c.out_channels, c.kernel_size[0], 1, c.padding[0], f"conv{k + 1}")
                      for k, c in enumerate(convs)]
        for p, c in zip(self.plans, convs):
            p.bind(c.weight, c.bias, need_t=False)  # no data gradient below conv1
        self.bound = list(zip(self.plans, convs))
        self.tail = SrcnnTail(self.plans, "srcnn")

    def pack(self) -> None:
        self.tail.pack()

    @staticmethod
    def chunks(n: int, hw: int, limit: int) -> List[Tuple[int, int]]:
        """[i0, i1) image ranges of at most ``limit`` pixels each."""
        if hw > limit:
            raise ValueError(f"SRCNN: one {hw}-pixel image is past the {limit} pixels a single launch addresses "
                             "(32-bit buffer offsets); tile the image")
        per = limit // hw
        return [(i, min(i + per, n)) for i in range(0, n, per)]

    def run(self, x: Tensor, keep: bool, need_w: bool = False):
        net = self.net
        if x.dim() != 4 or x.shape[1] != net.in_channels:
            raise ValueError(f"SRCNN: expected [n, {net.in_channels}, H, W], got {tuple(x.shape)}")
        n, c, h, w = x.shape
        limit = net._max_pixels_per_launch if keep else net._max_pixels_forward_only
        parts = self.chunks(n, h * w, limit)
        self.ensure_packed()
        xin = pack_input8(x, 8)
        out = f32((n, 1, h, w), x.device)
        for i0, i1 in parts:
            self.tail.fwd(xin[i0:i1], 8, 0, i1 - i0, h, w, out[i0:i1])
        return out, (dict(n=n, h=h, w=w, xin=xin, parts=parts) if keep else None)

    def backward(self, gout: Tensor, sv: dict, need_w: bool, need_x: bool, accumulate: bool) -> None:
        h, w, xin = sv["h"], sv["w"], sv["xin"]
        gout = gout.contiguous().float()
        nmax = max(i1 - i0 for i0, i1 in sv["parts"])
        dz1_all = self.buf("dz1", (nmax, h, w, 64), torch.bfloat16, gout.device)
        conv1 = self.plans[0]
        for k, (i0, i1) in enumerate(sv["parts"]):
            nc, acc = i1 - i0, accumulate or k > 0
            dz1 = dz1_all[:nc]
            # conv3 / conv2 gradients and dz1 in one launch that recomputes the forward, then dW1 / db1 from dz1
            self.tail.bwd(xin[i0:i1], 8, 0, nc, h, w, gout[i0:i1], dz1, self.ws, acc)
            conv1.wgrad(xin[i0:i1], 8, 0, h, w, dz1, 64, nc, self.ws, acc)
        self.grads_final()  # 8k-20k parameters: one bucket


class SRCNN(NativeModule, SRCNNParams):
    """The stand-alone SRCNN generator (see the module docstring)."""

    _engine_cls = _Engine
    _label = "SRCNN"
    _gpu_only_msg = "climsr_amd.SRCNN runs on the GPU only (no CPU fallback); move it with .cuda()"

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

    def forward(self, x: Tensor) -> Tensor:
        return self._native_forward(x)
