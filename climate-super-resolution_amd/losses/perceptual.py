"""Perceptual loss (drop-in for ``climsr.losses.perceptual.PerceptualLoss``, perceptual.py:7-36).

VGG19 ``features[:35]`` (conv1_1 .. conv5_4, the last without ReLU) applied to the 1->3 channel
repeat of both images, L1 between the feature maps, all without gradient (F7: the loss adds to
the value only).  Both images run as ONE batch through native implicit-GEMM convs with fused
bias+ReLU epilogues; the four MaxPool2d(2,2) run inside the epilogue of the conv before them (only the
pooled map is written: nothing reads the un-pooled one, the loss has no backward) where that conv's kernel
has the pooled epilogue, as a MaxPool2d kernel after it elsewhere; the L1 is a deterministic bf16 reduction.

``PerceptualLoss(differentiable=True)`` is the opt-in divergence from F7: the same value, with a native backward through
the stored bf16 forward into whichever image requires grad (the class docstring).

Weights: ``vgg19(pretrained=True)`` (perceptual.py:15) downloads ImageNet weights, impossible
offline; the module is built with the reference's parameter names (``loss_network.{i}.weight``)
so a torchvision VGG19 state_dict loads with ``load_state_dict`` when available.  By default it
is initialised with the deterministic He-uniform initializer (climsr_amd.core.init, gain sqrt(6)).
"""
from typing import List, Optional

import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import ops
from ..core.init import init_state, spec_from_shapes
from ..ops import ACT_NONE, ACT_RELU, ACT_RELU_BWD, ConvPlan, OUT_BF16

VGG19_E = [64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M"]


def _vgg19_features_35() -> nn.Sequential:
    layers: List[nn.Module] = []
    cin = 3
    for v in VGG19_E:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    return nn.Sequential(*layers[:35])


class PerceptualLoss(nn.Module):
    """Assumes input images of shape Nx1xHxW (perceptual.py:8-10).

    differentiable=False (the default) is the reference: no gradient, today's launches and bits.

    differentiable=True (a declared divergence from the reference): the same value, and when grad mode is on
    and an argument requires grad the result carries an autograd node whose backward returns, for each such argument,
    the exact gradient of ``mean |VGG[:35](cat3(a)) - VGG[:35](cat3(b))|`` through the stored bf16 forward, as
    [n,1,h,w] fp32.  Only a half that requires grad keeps state: its 16 conv outputs as stored (NHWC bf16, post-ReLU,
    conv5_4 pre-ReLU, before pooling; its pooled convs run conv + ops.maxpool2, the same bits); a constant half runs the
    fused path.  Kept per grad half at B=32, 256^2: 2 x 268 + 2 x 134 + 4 x 67 + 4 x 33.5 + 4 x 8.4 MB = about 1.24 GB,
    until the node's backward has run.  VGG weights get no gradient.  Under ``torch.no_grad()``, or when neither
    argument requires grad, it runs the default path.  Shape limits are the forward's (h, w multiples of 16, CUDA).

    retain_saved=True (tests) leaves ``self.saved`` after such a forward: ``{"acts": the 16 stored maps of the grad
    half, "f_grad": its conv5_4 features, "f_const": the other half's, "which": 0 | 1}``; with both arguments requiring
    grad ``which`` is 2, "acts" / "f_grad" are the first argument's and "acts2" / "f_const" the second's."""

    def __init__(self, deterministic_init: bool = True, fuse_pool: bool = True, differentiable: bool = False,
                 retain_saved: bool = False):
        """fuse_pool=False keeps every pool a kernel of its own (conv + ops.maxpool2): the same bits, for comparison."""
        super().__init__()
        self.fuse_pool = fuse_pool
        self.differentiable = bool(differentiable)
        self.retain_saved = bool(retain_saved)
        self.saved = None
        loss_network = _vgg19_features_35().eval()
        if deterministic_init:
            shapes = {k: tuple(v.shape) for k, v in loss_network.state_dict().items()}
            st = init_state(spec_from_shapes({"loss_network." + k: s for k, s in shapes.items()}), gain=float(np.sqrt(6.0)))
            loss_network.load_state_dict({k[len("loss_network."):]: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
        for param in loss_network.parameters():
            param.requires_grad = False
        self.loss_network = loss_network
        self._plans = None
        self._dev = None
        self._fused = {}  # (n, h, w) -> per conv: does its epilogue pool

    def _build(self, dev):
        plans = []
        mods = list(self.loss_network)
        for i, m in enumerate(mods):
            if isinstance(m, nn.Conv2d):
                relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
                pool = i + 2 < len(mods) and isinstance(mods[i + 2], nn.MaxPool2d)
                p = ConvPlan(m.in_channels, m.out_channels, 3, 1, 1, f"loss_network.{i}")
                w = m.weight.detach().contiguous().float()
                b = m.bias.detach().contiguous().float()
                p.bind(w, b, need_t=self.differentiable)  # the data gradient's packed weights: only where it can run
                p.pack()
                plans.append((p, relu, pool))
        self._plans = plans
        self._dev = dev
        self._fused = {}
        self._version = sum(int(p.weight._version) for p, _r, _q in plans)

    def _pool_fused(self, n: int, h: int, w: int):
        """Per conv, whether its kernel pools in the epilogue at this input shape: asked of the dispatch once per shape
        (ConvPlan.pool2_ok, no launch).  The rest -- tiles too small for the LDS-DMA conv -- keep conv + ops.maxpool2."""
        key = (n, h, w)
        if key not in self._fused:
            out, cs = [], 8
            for p, relu, pool in self._plans:
                ok = self.fuse_pool and relu and pool and h % 2 == 0 and w % 2 == 0 and p.pool2_ok(cs, 0, h, w, n, p.cout)
                out.append(ok)
                cs = p.cout
                if pool:
                    h, w = h // 2, w // 2
            self._fused[key] = out
        return self._fused[key]

    def features(self, x3: torch.Tensor, n: int, h: int, w: int, keep: Optional[list] = None) -> torch.Tensor:
        """x3: NHWC bf16 [n,h,w,8] with channels 0..2 = the image.  Returns conv5_4 features (bf16).  keep: a list
        each conv appends its stored map to (un-pooled, so every pool is then a kernel of its own)."""
        a, cs = x3, 8
        flags = self._pool_fused(n, h, w) if keep is None else [False] * len(self._plans)
        for (p, relu, pool), fused in zip(self._plans, flags):
            if fused:  # conv + bias + ReLU + MaxPool2d(2, 2) in one kernel
                h2, w2 = h // 2, w // 2
                yp = torch.empty((n, h2, w2, p.cout), dtype=torch.bfloat16, device=x3.device)
                p.fwd(a, cs, 0, h, w, yp, p.cout, 0, n, act=ACT_RELU, out_mode=OUT_BF16, pool2=True)
                a, cs, h, w = yp, p.cout, h2, w2
                continue
            y = torch.empty((n, h, w, p.cout), dtype=torch.bfloat16, device=x3.device)
            p.fwd(a, cs, 0, h, w, y, p.cout, 0, n, act=ACT_RELU if relu else ACT_NONE, out_mode=OUT_BF16)
            if keep is not None:
                keep.append(y)
            a, cs = y, p.cout
            if pool:
                h2, w2 = h // 2, w // 2
                yp = torch.empty((n, h2, w2, cs), dtype=torch.bfloat16, device=x3.device)
                ops.maxpool2(a, n, h, w, cs, yp)
                a, h, w = yp, h2, w2
        return a

    def _ready(self, dev):
        if self._plans is None or self._dev != dev:
            self.loss_network.to(dev)
            self._build(dev)

    def _half(self, img: torch.Tensor, keep: Optional[list]) -> torch.Tensor:
        """conv5_4 features of one image batch on its own (differentiable mode: the two halves keep different things)."""
        n, _c, h, w = img.shape
        x3 = torch.empty((n, h, w, 8), dtype=torch.bfloat16, device=img.device)
        ops.pack_planes8([(img.contiguous().float(), 0)] * 3, n, h, w, x3)
        return self.features(x3, n, h, w, keep)

    def backward_input(self, acts, seed: torch.Tensor, n: int, h: int, w: int, gscale: torch.Tensor, sign: float, numel: int):
        """The input gradient [n,1,h,w] fp32 of one half from its stored maps: seed (bf16, conv5_4's shape) is carried
        unscaled in bf16 through 15 data gradients with the ReLU mask (or, into a pooled map, the pool + ReLU routing
        kernel) and conv1_1's 64 -> 3 data gradient in fp32; the last kernel sums the three channels and applies
        sign * gscale / numel in fp32 (gscale: the incoming 0-d gradient, read on the device)."""
        dims = []
        for _p, _relu, pool in self._plans:
            dims.append((h, w))
            if pool:
                h, w = h // 2, w // 2
        dz = seed
        for i in range(len(self._plans) - 1, 0, -1):
            p = self._plans[i][0]
            (hi, wi), (hb, wb), below = dims[i], dims[i - 1], acts[i - 1]
            cin = p.cin_real
            g = torch.empty((n, hi, wi, cin), dtype=torch.bfloat16, device=seed.device)
            if self._plans[i - 1][2]:  # the layer below pools: plain data gradient into the pooled map, then the routing
                p.dgrad(dz, p.cout, hi, wi, g, cin, 0, n)
                dz = torch.empty((n, hb, wb, cin), dtype=torch.bfloat16, device=seed.device)
                ops.maxpool2_relu_bwd(g, below, n, hb, wb, cin, dz)
            else:
                p.dgrad(dz, p.cout, hi, wi, g, cin, 0, n, act=ACT_RELU_BWD, res1=below, res1_cs=cin, res1_co=0)
                dz = g
        p = self._plans[0][0]
        h0, w0 = dims[0]
        g3 = torch.empty((n, h0, w0, 4), dtype=torch.float32, device=seed.device)
        p.dgrad(dz, p.cout, h0, w0, g3, 4, 0, n)
        out = torch.empty((n, 1, h0, w0), dtype=torch.float32, device=seed.device)
        ops.sum3_scale(g3, n * h0 * w0, gscale, sign, numel, out)
        return out

    def forward(self, fake_high_resolution, high_resolution):
        a, b = fake_high_resolution, high_resolution
        if not a.is_cuda:
            raise RuntimeError("climsr_amd.PerceptualLoss runs on the GPU only (no CPU fallback)")
        self._ready(a.device)
        needs = (bool(a.requires_grad), bool(b.requires_grad))
        if self.differentiable and torch.is_grad_enabled() and any(needs):
            return _PerceptualGrad.apply(self, needs, a, b)
        with torch.no_grad():
            return self._forward_const(a, b)

    def _forward_const(self, a, b):
        n, _c, h, w = a.shape
        x3 = torch.empty((2 * n, h, w, 8), dtype=torch.bfloat16, device=a.device)
        a32, b32 = a.contiguous().float(), b.contiguous().float()
        # torch.cat([x, x, x], dim=1) (perceptual.py:26-31) as channels 0..2 of the padded NHWC input, one pass each
        ops.pack_planes8([(a32, 0)] * 3, n, h, w, x3[:n])
        ops.pack_planes8([(b32, 0)] * 3, n, h, w, x3[n:])
        f = self.features(x3, 2 * n, h, w)
        half = f.numel() // 2
        ws = torch.empty(512, dtype=torch.float64, device=a.device)
        out = torch.empty((), dtype=torch.float32, device=a.device)
        ops.l1_bf16(f.view(-1)[half:], f.view(-1)[:half], half, ws, out)
        return out


class _PerceptualGrad(torch.autograd.Function):
    """The value of PerceptualLoss on two n-batches, the grad half(s) keeping their stored maps for the backward."""

    @staticmethod
    def forward(ctx, mod, needs, a, b):
        keep = [[] if need else None for need in needs]
        fa = mod._half(a.detach(), keep[0])
        fb = mod._half(b.detach(), keep[1])
        ws = torch.empty(512, dtype=torch.float64, device=a.device)
        out = torch.empty((), dtype=torch.float32, device=a.device)
        ops.l1_bf16(fb.view(-1), fa.view(-1), fa.numel(), ws, out)
        ctx.mod, ctx.needs, ctx.keep, ctx.f, ctx.shape = mod, needs, keep, (fa, fb), tuple(a.shape)
        if mod.retain_saved:
            if all(needs):
                mod.saved = {"acts": keep[0], "acts2": keep[1], "f_grad": fa, "f_const": fb, "which": 2}
            else:
                k = 0 if needs[0] else 1
                mod.saved = {"acts": keep[k], "f_grad": (fa, fb)[k], "f_const": (fb, fa)[k], "which": k}
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if ctx.f is None:
            raise RuntimeError("PerceptualLoss: backward a second time; its stored maps were freed with the first")
        mod, (fa, fb) = ctx.mod, ctx.f
        n, _c, h, w = ctx.shape
        g = g.contiguous().float()
        seed = torch.empty_like(fa)  # sign(f_a - f_b); the second argument's gradient is its negative: applied at the end
        ops.l1_sign_bf16(fa.view(-1), fb.view(-1), fa.numel(), seed)
        grads = [mod.backward_input(ctx.keep[k], seed, n, h, w, g, (1.0, -1.0)[k], fa.numel()) if ctx.needs[k] else None
                 for k in (0, 1)]
        ctx.keep = ctx.f = None  # (the stored maps go with the first backward)
        return None, None, grads[0], grads[1]
