"""RCAN generator (drop-in for ``climsr.models.rcan.RCAN``): ``RCAN`` is native inference,
``TrainableRCAN`` is native training; checkpoints are interchangeable.

Same constructor kwargs (``n_resgroups, n_resblocks, n_feats, reduction, scaling_factor, in_channels,
out_channels, conv, **kwargs``; rcan.py:138-150), same submodule tree and ``state_dict`` keys
(``head.0``, ``body.{g}.body.{b}.body.{0,2}``, ``body.{g}.body.{b}.body.3.conv_du.{0,2}``,
``body.{g}.body.{n_resblocks}``, ``body.{n_resgroups}``, ``tail.0.{0,2}``, ``tail.1``, ``srcnn.conv{1,2,3}``),
same ``forward(x, elev, mask)`` (rcan.py:181-192) and the reference's lenient ``load_state_dict``
(rcan.py:194-219: shape-mismatched ``tail`` upsampler weights are skipped).

The forward runs entirely in libclimsr_hip.so: every conv on the MFMA implicit-GEMM kernels (bf16
NHWC activations, fp32 accumulation), the residual stream in fp32 with a bf16 shadow for the next
conv, channel attention as ``climsr_channel_attention`` + ``climsr_ca_scale_add`` (pool, 1x1-ReLU-1x1-
sigmoid, ``x * y + x`` in one pass), the group / body skips fused into the conv epilogues, the
Upsampler's ``nn.PixelShuffle`` as ``climsr_pixel_shuffle_bf16`` (bit-exact index map) and the SRCNN
tail as in the ESRGAN generator.  ``RCAN`` is inference only: the reference runs it from ``inference.py`` with
``net.eval()``; calling it in training mode with gradients enabled raises (no silent non-training).

``TrainableRCAN(NativeModule, RCAN)`` trains (``_target_: climsr_amd.models.rcan.TrainableRCAN`` with
``generator_type: "rcan"``; the reference's rcan_pre_training / rcan_fine_tuning experiments): same constructor
kwargs, submodule tree, ``state_dict`` keys, lenient ``load_state_dict`` and ``forward(x, elev, mask)``, so a checkpoint
saved from one class loads into the other.  Its parameters live in one flat fp32 buffer (core/flat.py) and it runs as
the shared autograd node of core/native.py (the fused AdamW, both gradient routes, the one-bucket grad-ready hook).  Under ``no_grad`` its forward is the inference
path above, bit for bit; with gradients the same launches also keep what the backward reads (per RCAB the block input,
the post-ReLU ``t``, ``u``, the attention scale and the pooled mean behind it).  The backward walks rcan.py:181-192 in
reverse on the existing conv gradient calls plus ``climsr_channel_attention_bwd`` and ``climsr_pixel_unshuffle_bf16``
(DESIGN.md §3.9).  It covers ``out_channels == 1``, ``n_feats == 64``, ``in_channels <= 4`` and ``scaling_factor`` 2
or 4; other values raise ``NotImplementedError`` from the constructor, as does a gradient w.r.t. an input.
"""
from __future__ import annotations

import logging
import math
from typing import Dict, List, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from .. import _lib
from .._lib import check, ptr
from ..core.native import NativeEngine, NativeModule
from ..ops import (ACT_NONE, ACT_RELU, ACT_RELU_BWD, OUT_BF16, OUT_F32, BatchedPacker, ConvPlan, SrcnnTail, _launch, act_grad, axpby,
                   nchw_to_nhwc)
from .srcnn import SRCNNParams, srcnn_tail_bwd, srcnn_tail_fwd


def default_conv(in_channels: int, out_channels: int, kernel_size: int, bias: bool = True) -> nn.Module:
    return nn.Conv2d(in_channels, out_channels, kernel_size, padding=kernel_size // 2, bias=bias)


class Upsampler(nn.Sequential):
    """rcan.py:17-47 (conv -> PixelShuffle per x2 stage, or one x3 stage)."""

    def __init__(self, conv, scale: int, n_feat: int, bn: bool = False, act=False, bias: bool = True):
        m: List[nn.Module] = []
        if (scale & (scale - 1)) == 0:
            for _ in range(int(math.log(scale, 2))):
                m.append(conv(n_feat, 4 * n_feat, 3, bias))
                m.append(nn.PixelShuffle(2))
        elif scale == 3:
            m.append(conv(n_feat, 9 * n_feat, 3, bias))
            m.append(nn.PixelShuffle(3))
        else:
            raise NotImplementedError
        if bn or act:
            raise NotImplementedError("RCAN's Upsampler is built with bn=False, act=False (rcan.py:166)")
        super().__init__(*m)


class CALayer(nn.Module):
    def __init__(self, channel: int, reduction: int = 16):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.conv_du = nn.Sequential(nn.Conv2d(channel, channel // reduction, 1, padding=0, bias=True), nn.ReLU(inplace=True),
                                     nn.Conv2d(channel // reduction, channel, 1, padding=0, bias=True), nn.Sigmoid())


class RCAB(nn.Module):
    def __init__(self, conv, n_feat: int, kernel_size: int, reduction: int, act: nn.Module, bias: bool = True, bn: bool = False,
                 res_scale: int = 1):
        super().__init__()
        self.body = nn.Sequential(conv(n_feat, n_feat, kernel_size, bias=bias), act, conv(n_feat, n_feat, kernel_size, bias=bias),
                                  CALayer(n_feat, reduction))
        self.res_scale = res_scale


class ResidualGroup(nn.Module):
    def __init__(self, conv, n_feat: int, kernel_size: int, reduction: int, n_resblocks: int):
        super().__init__()
        body: List[nn.Module] = [RCAB(conv, n_feat, kernel_size, reduction, bias=True, bn=False, act=nn.ReLU(True), res_scale=1)
                                 for _ in range(n_resblocks)]
        body.append(conv(n_feat, n_feat, kernel_size))
        self.body = nn.Sequential(*body)


class RCAN(nn.Module):
    def __init__(self, n_resgroups: int = 10, n_resblocks: int = 20, n_feats: int = 64, reduction: int = 16,
                 scaling_factor: int = 4, in_channels: int = 3, out_channels: int = 1, conv=default_conv, **kwargs):
        super().__init__()
        self.n_resgroups, self.n_resblocks, self.n_feats = n_resgroups, n_resblocks, n_feats
        self.kernel_size = 3
        self.reduction = reduction
        self.scaling_factor = scaling_factor
        self.in_channels, self.out_channels = in_channels, out_channels
        self.head = nn.Sequential(conv(in_channels, n_feats, self.kernel_size))
        body: List[nn.Module] = [ResidualGroup(conv, n_feats, self.kernel_size, reduction, n_resblocks=n_resblocks)
                                 for _ in range(n_resgroups)]
        body.append(conv(n_feats, n_feats, self.kernel_size))
        self.body = nn.Sequential(*body)
        self.tail = nn.Sequential(Upsampler(conv, scaling_factor, n_feats, act=False), conv(n_feats, out_channels, self.kernel_size))
        self.srcnn = SRCNNParams(in_channels=3, out_channels=out_channels)
        self._engine = None

    def load_state_dict(self, state_dict: dict, strict: bool = False):
        """rcan.py:194-219: copy matching names; a shape mismatch is tolerated only for ``tail`` keys."""
        own = self.state_dict()
        with torch.no_grad():
            for name, param in state_dict.items():
                if name in own:
                    if isinstance(param, nn.Parameter):
                        param = param.data
                    try:
                        own[name].copy_(param)
                    except Exception:
                        if name.find("tail") >= 0:
                            logging.info("Replace pre-trained upsampler to new one...")
                        else:
                            raise RuntimeError(f"While copying the parameter named {name}, whose dimensions in the model are "
                                               f"{own[name].size()} and whose dimensions in the checkpoint are {param.size()}.")
                elif strict and name.find("tail") == -1:
                    raise KeyError(f'unexpected key "{name}" in state_dict')
        if strict:
            missing = set(own.keys()) - set(state_dict.keys())
            if missing:
                raise KeyError(f'missing keys in state_dict: "{missing}"')

    def forward(self, x: Tensor, elev: Tensor, mask: Tensor) -> Tensor:
        if torch.is_grad_enabled() and self.training and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("native RCAN is inference-only in this build: call .eval() (as inference.py does) "
                                      "or run under torch.no_grad()")
        if not x.is_cuda:
            raise RuntimeError("RCAN runs in libclimsr_hip.so: inputs and parameters must be on a CUDA device")
        eng = self._engine
        if eng is None or eng.device != x.device:
            eng = _RcanEngine(self)
            object.__setattr__(self, "_engine", eng)
        return eng.forward(x, elev, mask)


class _RcanEngine:
    def _need_t(self, name: str) -> bool:
        """Whether conv ``name`` needs its transposed (data-gradient) weight layout: never for inference."""
        return False

    def __init__(self, m: RCAN):
        self.m = m
        self.device = m.head[0].weight.device
        self.nf = m.n_feats
        assert self.nf % 8 == 0, "n_feats must be a multiple of 8"
        self.cin_pad = (m.in_channels + 7) // 8 * 8
        self.plans: Dict[str, ConvPlan] = {}
        mods = dict(m.named_modules())
        self.mods = mods
        for name, mod in mods.items():
            if isinstance(mod, nn.Conv2d) and ".conv_du." not in name:
                p = ConvPlan(mod.in_channels, mod.out_channels, mod.kernel_size[0], mod.stride[0], mod.padding[0], name)
                p.bind(mod.weight, mod.bias, need_t=self._need_t(name))
                self.plans[name] = p
        self.ups: List[Tuple[str, int]] = []  # (conv name, shuffle factor)
        up = m.tail[0]
        for i, mod in enumerate(up):
            if isinstance(mod, nn.PixelShuffle):
                self.ups.append((f"tail.0.{i - 1}", mod.upscale_factor))
        self.packer = BatchedPacker(list(self.plans.values()), self.device)
        self.version = None
        self.ca_ws = None

    def _params_version(self):
        return tuple(p._version for p in self.m.parameters()) + tuple(p.data_ptr() for p in self.m.parameters())

    def ensure_packed(self):
        v = self._params_version()
        if v != self.version:
            for name, p in self.plans.items():  # rebind in case parameters were replaced
                mod = self.mods[name]
                p.bind(mod.weight, mod.bias, need_t=self._need_t(name))
            self.packer = BatchedPacker(list(self.plans.values()), self.device)
            self.packer.run()
            self.version = v

    def forward(self, x: Tensor, elev: Tensor, mask: Tensor) -> Tensor:
        return self.run(x, elev, mask, keep=False)[0]

    def run(self, x: Tensor, elev: Tensor, mask: Tensor, keep: bool):
        """(output, saved activations or None).  keep=False is the inference path.  keep=True (training) computes the
        same values with the same launches, except that every buffer the backward reads is a fresh one instead of a
        reused one, and the attention also hands out its pooled mean."""
        m, P, nf = self.m, self.plans, self.nf
        n, cin, h, w = x.shape
        dev = x.device
        sf = m.scaling_factor
        hh, ww = h * sf, w * sf
        assert elev.shape == (n, 1, hh, ww) and mask.shape == (n, 1, hh, ww), "elev/mask must be [N,1,sH,sW]"
        self.ensure_packed()
        L = _lib.load()
        st = _lib.stream_ptr()
        npx = n * h * w
        bf = lambda *s: torch.empty(s, dtype=torch.bfloat16, device=dev)  # noqa: E731
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
        lr = torch.zeros((n, h, w, self.cin_pad), dtype=torch.bfloat16, device=dev)
        nchw_to_nhwc(x.contiguous().float(), lr, self.cin_pad, 0)
        head = f32(n, h, w, nf)
        xb = bf(n, h, w, nf)
        P["head.0"].fwd(lr, self.cin_pad, 0, h, w, head, nf, 0, n, out_mode=OUT_F32, aux=xb, aux_cs=nf)
        xres = head.clone()
        xb_alt = bf(n, h, w, nf)
        gin = f32(n, h, w, nf)
        t = bf(n, h, w, nf)
        s = f32(n, nf)
        ws_bytes = L.climsr_channel_attention_workspace(n, nf)
        if self.ca_ws is None or self.ca_ws.numel() * 8 < ws_bytes or self.ca_ws.device != dev:
            self.ca_ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.float64, device=dev)
        # the RCAB's second conv pools its own output for the channel attention (per-tile channel sums in its epilogue,
        # the register-resident 64 -> 64 conv) when it can; else the pooling pass re-reads u
        cp_rows, cp_tpi = P["body.0.body.0.body.2"].ch_parts(nf, h, w, n, nf)
        cpart = f32(max(cp_rows, 1), nf)
        # u (the RCAB body's output) in bf16 when the conv pools it itself: the attention's mean comes from the fp32
        # values in the epilogue, only the scale-add reads u (half the bytes of the fp32 round trip)
        u = bf(n, h, w, nf) if cp_rows else f32(n, h, w, nf)
        new_u = (lambda: bf(n, h, w, nf)) if cp_rows else (lambda: f32(n, h, w, nf))
        nblk = m.n_resgroups * m.n_resblocks
        blocks, gtail_in = [], []  # keep: per RCAB (x_in, t, u, s, mean); per group the bf16 input of its tail conv
        s_all = f32(nblk, n, nf) if keep else None
        mean_all = f32(nblk, n, nf) if keep else None
        for g in range(m.n_resgroups):
            gin.copy_(xres)
            for b in range(m.n_resblocks):
                pre = f"body.{g}.body.{b}.body"
                mean = None
                if keep:  # this RCAB's own t / u / s / mean, and its output shadow in a buffer of its own
                    k = g * m.n_resblocks + b
                    t, u, s, mean, xb_out = bf(n, h, w, nf), new_u(), s_all[k], mean_all[k], bf(n, h, w, nf)
                    blocks.append((xb, t, u, s, mean))
                else:
                    xb_out = xb
                P[f"{pre}.0"].fwd(xb, nf, 0, h, w, t, nf, 0, n, act=ACT_RELU)
                ca = self.mods[f"{pre}.3"].conv_du
                w1, b1, w2, b2 = ca[0].weight, ca[0].bias, ca[2].weight, ca[2].bias
                if cp_rows:
                    P[f"{pre}.2"].fwd(t, nf, 0, h, w, u, nf, 0, n, ch_part=cpart)
                    if keep:
                        check(L.climsr_channel_attention_parts_keep(ptr(cpart), n, cp_tpi, h * w, nf, ptr(w1), ptr(b1), ptr(w2),
                                                                    ptr(b2), w1.shape[0], ptr(self.ca_ws), ptr(s), ptr(mean), st),
                              f"channel attention {pre}")
                    else:
                        check(L.climsr_channel_attention_parts(ptr(cpart), n, cp_tpi, h * w, nf, ptr(w1), ptr(b1), ptr(w2),
                                                               ptr(b2), w1.shape[0], ptr(self.ca_ws), ptr(s), st),
                              f"channel attention {pre}")
                else:
                    P[f"{pre}.2"].fwd(t, nf, 0, h, w, u, nf, 0, n, out_mode=OUT_F32)
                    if keep:
                        check(L.climsr_channel_attention_keep(ptr(u), n, h * w, nf, nf, ptr(w1), ptr(b1), ptr(w2), ptr(b2),
                                                              w1.shape[0], ptr(self.ca_ws), ptr(s), ptr(mean), st),
                              f"channel attention {pre}")
                    else:
                        check(L.climsr_channel_attention(ptr(u), n, h * w, nf, nf, ptr(w1), ptr(b1), ptr(w2), ptr(b2),
                                                         w1.shape[0], ptr(self.ca_ws), ptr(s), st), f"channel attention {pre}")
                check(L.climsr_ca_scale_add(ptr(u), int(bool(cp_rows)), nf, ptr(s), ptr(xres), ptr(xb_out), nf, n, h * w, nf, st),
                      f"rcab residual {pre}")
                xb = xb_out
            if keep:
                gtail_in.append(xb)
                xb_alt = bf(n, h, w, nf)
            # group tail conv + group skip (rcan.py:133-135), fp32 stream + bf16 shadow.  The shadow goes to the other
            # buffer of a pair: written in place, a tile's aux store would race the halo reads of its neighbours.
            P[f"body.{g}.body.{m.n_resblocks}"].fwd(xb, nf, 0, h, w, xres, nf, 0, n, res1=gin, res1_cs=nf, out_mode=OUT_F32,
                                                   aux=xb_alt, aux_cs=nf)
            xb, xb_alt = xb_alt, xb
        # body conv + global skip (rcan.py:185-186); only its bf16 form feeds the tail
        feat = bf(n, h, w, nf)
        P[f"body.{m.n_resgroups}"].fwd(xb, nf, 0, h, w, feat, nf, 0, n, res1=head, res1_cs=nf, out_mode=OUT_BF16)
        cur, ch, cw = feat, h, w
        up_in = []
        for name, r in self.ups:
            c4 = P[name].cout
            t4 = bf(n, ch, cw, c4)
            P[name].fwd(cur, nf, 0, ch, cw, t4, c4, 0, n)
            nxt = bf(n, ch * r, cw * r, nf)
            check(L.climsr_pixel_shuffle_bf16(ptr(t4), n, ch, cw, nf, r, c4, ptr(nxt), nf, st), f"pixel shuffle {name}")
            up_in.append(cur)
            cur, ch, cw = nxt, ch * r, cw * r
        assert (ch, cw) == (hh, ww)
        out, tail, _s1, _s2 = srcnn_tail_fwd(P, "tail.1", cur, nf, n, hh, ww, m.out_channels, elev, mask)
        if not keep:
            return out, None
        # head output: only its gradient is needed (the global skip), which is the body conv's output gradient
        return out, dict(n=n, h=h, w=w, hh=hh, ww=ww, lr=lr, blocks=blocks, gtail_in=gtail_in, body_in=xb, up_in=up_in, up_out=cur,
                         u_bf16=bool(cp_rows), tail=tail)


class _RcanTrainEngine(NativeEngine, _RcanEngine):
    """``_RcanEngine`` over a ``TrainableRCAN``'s flat parameters, with the backward (re-pack rule, scratch and
    ``bind_grads`` from ``NativeEngine``)."""

    def _need_t(self, name: str) -> bool:
        # no data gradient below the head; tail.1 (64 -> 1) and srcnn.conv2 / conv3 have kernels of their own
        return name not in ("head.0", "tail.1", "srcnn.conv2", "srcnn.conv3")

    def __init__(self, m: "TrainableRCAN"):
        NativeEngine.__init__(self, m)
        _RcanEngine.__init__(self, m)
        self.bound = [(p, self.mods[name]) for name, p in self.plans.items()]
        self.srcnn_tail = SrcnnTail([self.plans[f"srcnn.conv{k}"] for k in (1, 2, 3)])
        self.cab_ws = None

    def pack(self) -> None:
        self.packer.run()
        self.srcnn_tail.pack()

    def run(self, x: Tensor, elev: Tensor, mask: Tensor, keep: bool, need_w: bool = False):
        return _RcanEngine.run(self, x, elev, mask, keep)

    def backward(self, gout: Tensor, sv: dict, need_w: bool, need_x: bool, accumulate: bool) -> None:
        """Parameter gradients into the bound ``.grad`` views (= or += with ``accumulate``), the network walked in
        reverse (rcan.py:181-192).  bf16 output gradients between convs, activation backward in the data-gradient
        epilogues, fp32 only for the residual-stream gradient G."""
        m, P, nf = self.m, self.plans, self.nf
        n, h, w, hh, ww = sv["n"], sv["h"], sv["w"], sv["hh"], sv["ww"]
        dev = gout.device
        acc, ws = accumulate, self.ws
        L = _lib.load()
        st = _lib.stream_ptr()
        npx = n * h * w
        bf16, f32 = torch.bfloat16, torch.float32
        gout = gout.contiguous().float()
        # ---- SRCNN tail (srcnn.py:13-18): conv3 / conv2 gradients and conv1's output gradient in one launch that
        # recomputes the two ReLU layers from the 8-channel buffer; dz8's channels 1..7 stay zero (elev / mask: no gradient)
        dzA = self.buf("dzA", (n, hh, ww, nf), bf16, dev)
        dz8 = self.buf("dz8", (n, hh, ww, 8), bf16, dev, zero=True)
        srcnn_tail_bwd(P, self.srcnn_tail, sv["tail"], n, hh, ww, gout, dzA, dz8, ws, acc)
        # ---- tail.1 (64 -> 1): its data gradient is the single-output stencil
        P["tail.1"].wgrad(sv["up_out"], nf, 0, hh, ww, dz8, 8, n, ws, acc)
        P["tail.1"].dgrad(dz8, 8, hh, ww, dzA, nf, 0, n)
        # ---- Upsampler, last stage first: PixelShuffle backward (index map), then the 64 -> r*r*64 conv
        gb = self.buf("Gb", (n, h, w, nf), f32, dev)  # fp32 gradient at the body output (= at the head, global skip)
        cur, ch, cw = dzA, hh, ww
        for k in reversed(range(len(self.ups))):
            name, r = self.ups[k]
            c4 = P[name].cout
            ch, cw = ch // r, cw // r
            dz4 = self.buf(f"dz4.{k}", (n, ch, cw, c4), bf16, dev)
            _launch(f"pixel unshuffle {name}", lambda: L.climsr_pixel_unshuffle_bf16(ptr(cur), n, ch, cw, nf, r, nf, ptr(dz4), c4, st),
                    nbytes=4 * n * ch * cw * c4)
            P[name].wgrad(sv["up_in"][k], nf, 0, ch, cw, dz4, c4, n, ws, acc)
            if k > 0:
                nxt = self.buf(f"dzup.{k}", (n, ch, cw, nf), bf16, dev)
                P[name].dgrad(dz4, c4, ch, cw, nxt, nf, 0, n)
                cur = nxt
            else:
                P[name].dgrad(dz4, c4, ch, cw, gb, nf, 0, n)
        assert (ch, cw) == (h, w)
        # ---- body conv + global skip (rcan.py:185-186): Gb stays for the head, G = conv^T(bf16(Gb)) enters the groups
        dz64 = self.buf("dz64", (n, h, w, nf), bf16, dev)
        g_cur = self.buf("G0", (n, h, w, nf), f32, dev)
        g_alt = self.buf("G1", (n, h, w, nf), f32, dev)
        dzu = self.buf("dzu", (n, h, w, nf), bf16, dev)
        dzt = self.buf("dzt", (n, h, w, nf), bf16, dev)
        mbuf = self.buf("m", (n, nf), f32, dev)
        body = P[f"body.{m.n_resgroups}"]
        act_grad(npx, nf, gb, nf, 0, None, 0, 0, ACT_NONE, dz64, nf)
        body.wgrad(sv["body_in"], nf, 0, h, w, dz64, nf, n, ws, acc)
        body.dgrad(dz64, nf, h, w, g_cur, nf, 0, n)
        cr = m.n_feats // m.reduction
        need = L.climsr_channel_attention_bwd_workspace(n, nf, cr)
        if self.cab_ws is None or self.cab_ws.numel() * 8 < need or self.cab_ws.device != dev:
            self.cab_ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=dev)
        u_bf16 = int(sv["u_bf16"])
        for g in reversed(range(m.n_resgroups)):
            # group tail conv + group skip (rcan.py:133-135): g_cur = the gradient at the group's output, which is also
            # the skip's gradient at the group's input; g_alt = conv^T(bf16(g_cur)) walks the RCABs
            gt = P[f"body.{g}.body.{m.n_resblocks}"]
            act_grad(npx, nf, g_cur, nf, 0, None, 0, 0, ACT_NONE, dz64, nf)
            gt.wgrad(sv["gtail_in"][g], nf, 0, h, w, dz64, nf, n, ws, acc)
            gt.dgrad(dz64, nf, h, w, g_alt, nf, 0, n)
            for b in reversed(range(m.n_resblocks)):
                pre = f"body.{g}.body.{b}.body"
                x_in, t, u, s, mean = sv["blocks"][g * m.n_resblocks + b]
                ca = self.mods[f"{pre}.3"].conv_du
                c0, c2 = ca[0], ca[2]
                # x_out = u s(u) + x_in: attention + scale backward (three launches) -> dzu = the gradient at u
                _launch(f"channel attention bwd {pre}", lambda: L.climsr_channel_attention_bwd(
                    ptr(g_alt), nf, ptr(u), u_bf16, nf, ptr(s), ptr(mean), n, h * w, nf, ptr(c0.weight), ptr(c0.bias), ptr(c2.weight),
                    cr, ptr(self.cab_ws), ptr(mbuf), ptr(c0.weight.grad), ptr(c0.bias.grad), ptr(c2.weight.grad), ptr(c2.bias.grad),
                    int(acc), ptr(dzu), nf, st), nbytes=npx * nf * (8 + 2 * u.element_size() + 2))
                P[f"{pre}.2"].wgrad(t, nf, 0, h, w, dzu, nf, n, ws, acc)
                P[f"{pre}.2"].dgrad(dzu, nf, h, w, dzt, nf, 0, n, act=ACT_RELU_BWD, res1=t, res1_cs=nf, res1_co=0)
                P[f"{pre}.0"].wgrad(x_in, nf, 0, h, w, dzt, nf, n, ws, acc)
                P[f"{pre}.0"].dgrad(dzt, nf, h, w, g_alt, nf, 0, n, accumulate=True)  # the RCAB skip passes G unchanged
            axpby(npx, nf, 1.0, g_cur, nf, 0, 1.0, g_alt, nf, 0)  # + the group skip
            g_cur, g_alt = g_alt, g_cur
        # ---- head: the body path + the global skip; no data gradient below it
        axpby(npx, nf, 1.0, gb, nf, 0, 1.0, g_cur, nf, 0)
        act_grad(npx, nf, g_cur, nf, 0, None, 0, 0, ACT_NONE, dz64, nf)
        P["head.0"].wgrad(sv["lr"], self.cin_pad, 0, h, w, dz64, nf, n, ws, acc)
        self.grads_final()


class TrainableRCAN(NativeModule, RCAN):
    """``RCAN`` that trains (see the module docstring): same constructor, submodules, ``state_dict`` and forward."""

    _engine_cls = _RcanTrainEngine
    _label = "RCAN"
    _gpu_only_msg = "TrainableRCAN runs in libclimsr_hip.so: inputs and parameters must be on a CUDA device"

    def __init__(self, n_resgroups: int = 10, n_resblocks: int = 20, n_feats: int = 64, reduction: int = 16,
                 scaling_factor: int = 4, in_channels: int = 3, out_channels: int = 1, conv=default_conv, **kwargs):
        if out_channels != 1:
            raise NotImplementedError(f"TrainableRCAN: out_channels={out_channels}; the backward of the SRCNN tail is "
                                      "single-output (RCAN runs inference for any)")
        if n_feats != 64:
            raise NotImplementedError(f"TrainableRCAN: n_feats={n_feats}; the backward is built for 64 features")
        if not 1 <= in_channels <= 4:
            raise NotImplementedError(f"TrainableRCAN: in_channels={in_channels}; the backward takes 1 to 4")
        if scaling_factor not in (2, 4):
            raise NotImplementedError(f"TrainableRCAN: scaling_factor={scaling_factor}; x2 and x4 train (the x3 upsampler's "
                                      "64 -> 576 conv has no tested gradient route; RCAN runs x3 inference)")
        if conv is not default_conv:
            raise NotImplementedError("TrainableRCAN: a custom conv factory is not supported")
        super().__init__(n_resgroups=n_resgroups, n_resblocks=n_resblocks, n_feats=n_feats, reduction=reduction,
                         scaling_factor=scaling_factor, in_channels=in_channels, out_channels=out_channels, conv=conv, **kwargs)
        self._flatten()

    def forward(self, x: Tensor, elev: Tensor, mask: Tensor) -> Tensor:
        return self._native_forward(x, elev, mask)
