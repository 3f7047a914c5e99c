"""RFB-ESRGAN discriminator (drop-in for ``climsr.models.rfb_esrgan.RFBESRGANDiscriminator``).

Same constructor (``in_channels=1``), same ``features`` / ``fc`` submodules and ``state_dict`` keys
(rfb_esrgan.py:26-61), ``forward(x: [N,1,H,W]) -> [N,1]`` in (0,1) (rfb_esrgan.py:63-69), honours
``.train()`` / ``.eval()`` (batch statistics + running-stat update vs running statistics).  All
arithmetic runs in libclimsr_hip: implicit-GEMM convs (stride 1/2; the stride-2 data gradient as a
stride-1 conv over the zero-inserted gradient), BatchNorm fused with LeakyReLU(0.2), the adaptive
16->14 average pool, fc.0 (100352->1024) on MFMA with split-K, and the LeakyReLU/fc.2/Sigmoid head.

Each call is one autograd node (the shared ``NativeFn`` of core/native.py).  Weight/BN-affine gradients land in one flat fp32 buffer and are
only computed when the parameters require grad (Lightning toggles D off during the generator
update, pl_gan.py:63-79); the input gradient (into the generator) is computed when the input
requires grad.
"""
from __future__ import annotations

import torch
import torch.nn as nn
from torch import Tensor

from .. import ops
from ..core.native import NativeEngine, NativeModule, bf16, f32, pack_input8
from ..ops import ACT_LRELU, ACT_LRELU_BWD, BatchedPacker, ConvPlan

POOL = 14


class _DEngine(NativeEngine):
    def __init__(self, d: "RFBESRGANDiscriminator"):
        super().__init__(d)
        self.d = d
        dev = d.fc[0].weight.device
        self.layers = []  # (conv module, bn module or None, ConvPlan)
        feats = list(d.features)
        for i, m in enumerate(feats):
            if isinstance(m, nn.Conv2d):
                bn = feats[i + 1] if i + 1 < len(feats) and isinstance(feats[i + 1], nn.BatchNorm2d) else None
                plan = ConvPlan(m.in_channels, m.out_channels, 3, m.stride[0], 1, f"features.{i}")
                plan.bind(m.weight, None, need_t=True)
                self.layers.append((m, bn, plan))
        self.bound = [(p, c) for c, _b, p in self.layers]
        self.packer = BatchedPacker([p for _c, _b, p in self.layers], dev)
        self.fc0_bf16 = torch.empty(d.fc[0].weight.shape, dtype=torch.bfloat16, device=dev)

    def pack(self, mirror_done: bool = False):
        """mirror_done: the optimizer's AdamW pass already wrote fc0_bf16 (climsr_adamw_step_mirror)."""
        self.packer.run()
        if not mirror_done:
            ops.f32_to_bf16(self.d.fc[0].weight, self.fc0_bf16)

    # ------------------------------------------------------------------ forward
    def run(self, x: Tensor, keep: bool, need_w: bool):
        """need_w: also write the transposed pooled features, which only fc.0's weight gradient reads."""
        d = self.d
        n, cin, h, w = x.shape
        dev = x.device
        self.ensure_packed()
        cpad = (cin + 7) // 8 * 8
        a_prev, cs_prev, hh, ww = pack_input8(x, cpad), cpad, h, w
        saved = []
        training = d.training
        for conv, bn, plan in self.layers:
            oh, ow = plan.out_hw(hh, ww)
            c = plan.cout
            if bn is None:
                a = bf16((n, oh, ow, c), dev)
                plan.fwd(a_prev, cs_prev, 0, hh, ww, a, c, 0, n, act=ACT_LRELU, use_bias=False)
                saved.append(dict(a_in=a_prev, cs_in=cs_prev, h_in=hh, w_in=ww, z=None, a=a, mean=None, rstd=None, oh=oh, ow=ow))
            else:
                z = bf16((n, oh, ow, c), dev)
                a = bf16((n, oh, ow, c), dev)
                npix = n * oh * ow
                # train mode: the conv epilogue emits the batch statistics' partial sums (no pass over z for them)
                nparts = plan.bn_parts(cs_prev, hh, ww, n, c) if training else 0
                part = self.buf(f"bnpart{len(saved)}", (max(nparts, 1) * 2 * c,), torch.float64, dev) if nparts else None
                plan.fwd(a_prev, cs_prev, 0, hh, ww, z, c, 0, n, use_bias=False, bn_part=part)
                if training:
                    mean, rstd = f32((c,), dev), f32((c,), dev)
                    if nparts:
                        ops.bn_forward_parts(part, nparts, z, npix, c, bn.weight, bn.bias, mean, rstd, a, bn.running_mean,
                                             bn.running_var, eps=bn.eps, momentum=bn.momentum,
                                             num_batches_tracked=bn.num_batches_tracked)
                    else:
                        ops.bn_forward(z, npix, c, bn.weight, bn.bias, mean, rstd, a, ops.bn_workspace(npix, c, self.scratch, dev),
                                       bn.running_mean, bn.running_var, eps=bn.eps, momentum=bn.momentum,
                                       num_batches_tracked=bn.num_batches_tracked)
                else:
                    mean = rstd = None
                    ops.bn_inference(z, npix, c, bn.running_mean, bn.running_var, bn.weight, bn.bias, a, eps=bn.eps)
                saved.append(dict(a_in=a_prev, cs_in=cs_prev, h_in=hh, w_in=ww, z=z, a=a, mean=mean, rstd=rstd, oh=oh, ow=ow))
            a_prev, cs_prev, hh, ww = a, c, oh, ow
        c = cs_prev
        feat = c * POOL * POOL
        n_pad = (n + 31) // 32 * 32
        p = bf16((n, feat), dev)
        p_t = torch.zeros((feat, n_pad), dtype=torch.bfloat16, device=dev) if need_w else None
        ops.adaptive_pool_fwd(a_prev, n, hh, ww, c, POOL, POOL, p, p_t, n_pad)
        fc0, fc2 = d.fc[0], d.fc[2]
        hid = f32((n, fc0.out_features), dev)
        nsplit_max = 3072 // ((fc0.out_features + 63) // 64) + 1
        lin_ws = self.buf("linws", (nsplit_max * n * fc0.out_features,), torch.float32, dev)
        ops.linear_fwd(p, self.fc0_bf16, fc0.bias, n, feat, fc0.out_features, hid, lin_ws, act=ACT_LRELU, slope=0.2)
        s = f32((n, 1), dev)
        ops.d_head_fwd(hid, fc2.weight, fc2.bias, n, fc0.out_features, s)
        sv = None
        if keep:
            sv = dict(n=n, h=h, w=w, cpad=cpad, layers=saved, p_t=p_t, hid=hid, s=s, n_pad=n_pad, feat=feat, hh=hh, ww=ww, c=c)
        return s, sv

    # ------------------------------------------------------------------ backward
    def backward(self, ds: Tensor, sv: dict, need_w: bool, need_x: bool, accumulate: bool):
        d = self.d
        dev = ds.device
        n, n_pad, feat = sv["n"], sv["n_pad"], sv["feat"]
        fc0, fc2 = d.fc[0], d.fc[2]
        o = fc0.out_features
        ds = ds.contiguous().float()
        du0 = bf16((n, o), dev)
        du0_t = torch.zeros((o, n_pad), dtype=torch.bfloat16, device=dev)
        acc = accumulate
        ops.d_head_bwd(sv["hid"], sv["s"], ds, fc2.weight, n, o, n_pad, fc2.weight.grad if need_w else None,
                       fc2.bias.grad if need_w else None, fc0.bias.grad if need_w else None, acc, du0, du0_t)
        if need_w:
            ops.linear_wgrad(du0_t, sv["p_t"], n_pad, feat, o, fc0.weight.grad, acc)
            hook = d._grad_ready_hook
            if hook is not None:  # fc.0 / fc.2 (the last flat entries, 103 M of 107 M parameters) are final once
                # every backward of the step has accumulated into them (loss_d runs D twice, pl_gan.py:51-61)
                object.__setattr__(d, "_ready_calls", d._ready_calls + 1)
                if d._ready_calls >= d._ready_need:
                    object.__setattr__(d, "_ready_calls", 0)
                    hook(d._fc_flat_lo())
        dp = self.buf("dp", (n, feat), torch.float32, dev)
        ops.linear_dgrad(du0, self.fc0_bf16, n, feat, o, dp)
        hh, ww, c = sv["hh"], sv["ww"], sv["c"]
        da = f32((n, hh, ww, c), dev)
        ops.adaptive_pool_bwd(dp, n, hh, ww, c, POOL, POOL, da)
        coef = self.buf("bncoef", (3 * 512,), torch.float32, dev)
        dx = None
        dz_next = None  # layer 0's output gradient, written directly by layer 1's data gradient
        fused = {}  # layer -> (part, nparts): its BN backward statistics, from the next layer's data-gradient epilogue
        for li in reversed(range(len(self.layers))):
            conv, bn, plan = self.layers[li]
            L = sv["layers"][li]
            oh, ow, c = L["oh"], L["ow"], plan.cout
            npix = n * oh * ow
            cz = (c + 7) // 8 * 8
            if bn is not None:
                # lrelu'(a) recomputed from z: the activation is not read; da is the bf16 data gradient of the
                # next conv (fp32 only for the last layer, from the pooling backward)
                dz = bf16((n, oh, ow, cz), dev)
                if li in fused:
                    part, nparts = fused.pop(li)
                    ops.bn_backward_parts(part, nparts, da, L["z"], npix, c, L["mean"], L["rstd"], bn.weight, bn.bias, coef,
                                          bn.weight.grad if need_w else None, bn.bias.grad if need_w else None, acc, dz)
                else:
                    ops.bn_backward_z(da, L["z"], npix, c, L["mean"], L["rstd"], bn.weight, bn.bias,
                                      ops.bn_workspace(npix, c, self.scratch, dev), coef,
                                      bn.weight.grad if need_w else None, bn.bias.grad if need_w else None, acc, dz)
            elif dz_next is not None:
                dz = dz_next
            else:
                dz = bf16((n, oh, ow, cz), dev)
                ops.act_grad(npix, c, da, c, 0, L["a"], c, 0, ACT_LRELU, dz, cz)
            if need_w:
                plan.wgrad(L["a_in"], L["cs_in"], 0, L["h_in"], L["w_in"], dz, cz, n, self.ws, acc)
            if li > 0 or need_x:
                prev_bn = self.layers[li - 1][1] if li > 0 else None
                if prev_bn is None and li > 0:
                    # the previous layer has no BN (layer 0): its LeakyReLU' (from its stored bf16 activation) goes
                    # into this data gradient's epilogue, which writes that layer's bf16 output gradient
                    P0 = sv["layers"][li - 1]
                    g = bf16((n, L["h_in"], L["w_in"], plan.cin), dev)
                    plan.dgrad(dz, cz, oh, ow, g, plan.cin, 0, n, act=ACT_LRELU_BWD, res1=P0["a"], res1_cs=plan.cin, res1_co=0)
                    dz_next = g
                elif li > 0:
                    g = bf16((n, L["h_in"], L["w_in"], plan.cin), dev)  # bf16: read by the previous layer's BN backward
                    P = sv["layers"][li - 1]
                    # that BN's backward statistics (sum d, sum d * xhat) come from this data gradient's epilogue
                    # where its kernel supports them: the separate statistics pass over g and z is skipped
                    nparts = plan.dgrad_bn_parts(cz, oh, ow, plan.cin, n, plan.cin) if P["mean"] is not None else 0
                    if nparts:
                        part = self.buf(f"bnbwd{li - 1}", (nparts * 2 * plan.cin,), torch.float64, dev)
                        plan.dgrad(dz, cz, oh, ow, g, plan.cin, 0, n,
                                   bn_bwd=(part, P["z"], plan.cin, P["mean"], P["rstd"], prev_bn.weight, prev_bn.bias))
                        fused[li - 1] = (part, nparts)
                    else:
                        plan.dgrad(dz, cz, oh, ow, g, plan.cin, 0, n)
                else:
                    g = f32((n, L["h_in"], L["w_in"], plan.cin), dev)
                    plan.dgrad(dz, cz, oh, ow, g, plan.cin, 0, n)
                da = g
            if li == 0 and need_x:
                dx = torch.empty((n, 1, sv["h"], sv["w"]), dtype=torch.float32, device=dev)
                ops.nhwc_to_nchw(da, n, 1, sv["h"], sv["w"], plan.cin, 0, dx)
        return dx


class RFBESRGANDiscriminator(NativeModule, nn.Module):
    r"""The main architecture of the discriminator. Similar to VGG structure (rfb_esrgan.py:23-69)."""

    _engine_cls = _DEngine
    _input_grad = True
    _label = "discriminator"
    _gpu_only_msg = "climsr_amd.RFBESRGANDiscriminator runs on the GPU only (no CPU fallback)"
    _engine_dies_on_apply = True  # buffers (BN running stats) may have moved too

    def __init__(self, in_channels=1):
        super().__init__()
        self.features = nn.Sequential(
            nn.Conv2d(in_channels, 64, kernel_size=3, stride=1, padding=1, bias=False),
            nn.LeakyReLU(negative_slope=0.2, inplace=True),
            nn.Conv2d(64, 64, kernel_size=3, stride=2, padding=1, bias=False),
            nn.BatchNorm2d(64),
            nn.LeakyReLU(negative_slope=0.2, inplace=True),
            nn.Conv2d(64, 128, kernel_size=3, stride=1, padding=1, bias=False),
            nn.BatchNorm2d(128),
            nn.LeakyReLU(negative_slope=0.2, inplace=True),
            nn.Conv2d(128, 128, kernel_size=3, stride=2, padding=1, bias=False),
            nn.BatchNorm2d(128),
            nn.LeakyReLU(negative_slope=0.2, inplace=True),
            nn.Conv2d(128, 256, kernel_size=3, stride=1, padding=1, bias=False),
            nn.BatchNorm2d(256),
            nn.LeakyReLU(negative_slope=0.2, inplace=True),
            nn.Conv2d(256, 256, kernel_size=3, stride=2, padding=1, bias=False),
            nn.BatchNorm2d(256),
            nn.LeakyReLU(negative_slope=0.2, inplace=True),
            nn.Conv2d(256, 512, kernel_size=3, stride=1, padding=1, bias=False),
            nn.BatchNorm2d(512),
            nn.LeakyReLU(negative_slope=0.2, inplace=True),
            nn.Conv2d(512, 512, kernel_size=3, stride=2, padding=1, bias=False),
            nn.BatchNorm2d(512),
            nn.LeakyReLU(negative_slope=0.2, inplace=True),
        )
        self.avgpool = nn.AdaptiveAvgPool2d((POOL, POOL))
        self.fc = nn.Sequential(
            nn.Linear(512 * POOL * POOL, 1024),
            nn.LeakyReLU(negative_slope=0.2, inplace=True),
            nn.Linear(1024, 1),
            nn.Sigmoid(),
        )
        self._flatten()
        object.__setattr__(self, "_ready_calls", 0)
        object.__setattr__(self, "_ready_need", 1)

    def set_grad_ready_hook(self, fn, calls_per_step: int = 1) -> None:
        """Call ``fn(lo)`` during backward once the fc gradients (flat offsets >= lo; 103 M of the 107 M
        parameters, computed first) are final (core/ddp.OverlappedGradAllReducer): on the
        ``calls_per_step``-th weight-gradient backward of the step (the D loss backpropagates through two D
        calls, real and fake, pl_gan.py:51-61, so it passes 2).  ``fn=None`` removes it."""
        object.__setattr__(self, "_grad_ready_hook", fn)
        object.__setattr__(self, "_ready_calls", 0)
        object.__setattr__(self, "_ready_need", max(1, int(calls_per_step)))

    def bf16_mirror(self):
        """(flat offset, numel, bf16 buffer) of fc.0's weight: its MFMA copy, written by the fused AdamW pass."""
        eng = self.engine()
        return self._fc_flat_lo(), self.fc[0].weight.numel(), eng.fc0_bf16

    def _fc_flat_lo(self) -> int:
        p = self.fc[0].weight
        for q, off, _n in self._flat_index:
            if q is p:
                return off
        raise KeyError("fc.0.weight not in the flat parameter index")

    def forward(self, input: Tensor) -> Tensor:
        return self._native_forward(input)
