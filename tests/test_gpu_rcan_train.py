"""GPU checks of native RCAN training (``climsr_amd.models.rcan.TrainableRCAN``):

* the PixelShuffle backward (pixel unshuffle): bit-exact vs torch, and the inverse of the shuffle;
* the channel-attention backward vs torch fp64 autograd on the CPU;
* the training (keep) forward, the no-grad forward and ``RCAN`` agree bit for bit;
* parameter gradients and three trainer steps vs the fp64 oracle, inside 2x the spread of the oracle's own torch-autocast
  fp16 / bf16 runs (helpers.update_envelope) and cosine >= 0.97.  The channel-attention tensors are compared as ONE
  vector and the other tensors under 128 elements pooled: with random weights some attention hidden units are dead
  (an exactly zero fp64 gradient) and others carry gradients of ~1e-8, for which a per-tensor relative error is undefined.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from climsr_amd.core.init import init_state, spec_from_shapes
from oracle import climsr_ref as ref
from tests.helpers import gemm_conv, pool_small, update_envelope

pytestmark = pytest.mark.gpu
DEV = "cuda"
POOL_BELOW = 128
# name -> (n_resgroups, n_resblocks, scaling_factor, batch, LR size)
CONFIGS = {"g2b2_x4": (2, 2, 4, 2, 16), "g2b2_x2": (2, 2, 2, 1, 24), "g10b20_x4": (10, 20, 4, 1, 16)}
ADAMW_YAML = {"_target_": "torch.optim.AdamW", "lr": 1e-4, "weight_decay": 1e-4}
ONE_CYCLE_YAML = {"_target_": "torch.optim.lr_scheduler.OneCycleLR", "max_lr": 1e-4, "num_training_steps": -1, "epochs": 1,
                  "pct_start": 0.05, "div_factor": 2, "final_div_factor": 100}


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("r,c_out,h,w", [(2, 64, 5, 7), (3, 64, 4, 4), (2, 8, 9, 3)])
def test_pixel_unshuffle_bit_exact(r, c_out, h, w):
    from climsr_amd import _lib
    from climsr_amd._lib import check, ptr

    n = 2
    L, st = _lib.load(), _lib.stream_ptr()
    gen = torch.Generator().manual_seed(7)
    g = torch.randn((n, c_out, h * r, w * r), generator=gen).to(torch.bfloat16)
    want = F.pixel_unshuffle(g, r)  # [n, c_out r r, h, w]
    gd = g.permute(0, 2, 3, 1).contiguous().to(DEV)
    y = torch.empty((n, h, w, c_out * r * r), dtype=torch.bfloat16, device=DEV)
    check(L.climsr_pixel_unshuffle_bf16(ptr(gd), n, h, w, c_out, r, c_out, ptr(y), c_out * r * r, st), "unshuffle")
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().permute(0, 3, 1, 2), want)
    # shuffle followed by unshuffle is the identity
    x = torch.randn((n, h, w, c_out * r * r), generator=gen).to(torch.bfloat16).to(DEV)
    mid = torch.empty((n, h * r, w * r, c_out), dtype=torch.bfloat16, device=DEV)
    back = torch.empty_like(x)
    check(L.climsr_pixel_shuffle_bf16(ptr(x), n, h, w, c_out, r, c_out * r * r, ptr(mid), c_out, st), "shuffle")
    check(L.climsr_pixel_unshuffle_bf16(ptr(mid), n, h, w, c_out, r, c_out, ptr(back), c_out * r * r, st), "unshuffle")
    torch.cuda.synchronize()
    assert torch.equal(back, x)


@pytest.mark.parametrize("u_bf16", [0, 1], ids=["u_fp32", "u_bf16"])
@pytest.mark.parametrize("n,h,w,c,cr", [(2, 13, 17, 64, 4), (1, 2, 3, 64, 4), (3, 16, 16, 64, 4)])
def test_channel_attention_backward_vs_fp64_autograd(n, h, w, c, cr, u_bf16):
    """out = u s(u) + x with a random upstream gradient G: m and the four parameter gradients within 1e-5 of the
    reference tensor's max-abs (the forward test's bound; the sums are fp64), dz_u within |diff| <= 2^-8 |ref| of
    bf16(G s + m) from the device's own s and m, accumulate = 2x, reruns bit-identical."""
    from climsr_amd import _lib
    from climsr_amd._lib import check, ptr

    gen = torch.Generator().manual_seed(11)
    u = torch.randn((n, h, w, c), generator=gen)
    if u_bf16:
        u = u.to(torch.bfloat16).float()  # the reference uses the rounded u
    G = torch.randn((n, h, w, c), generator=gen)
    w1 = torch.randn((cr, c), generator=gen) * 0.2
    b1 = torch.randn((cr,), generator=gen) * 0.1
    w2 = torch.randn((c, cr), generator=gen) * 0.2
    b2 = torch.randn((c,), generator=gen) * 0.1
    # ---- torch fp64 autograd on the CPU
    p = [t.double().requires_grad_(True) for t in (u, w1, b1, w2, b2)]
    u64, w1d, b1d, w2d, b2d = p
    s_ref = torch.sigmoid(torch.relu(u64.mean(dim=(1, 2)) @ w1d.T + b1d) @ w2d.T + b2d)
    out = u64 * s_ref[:, None, None, :]  # (+ x: its gradient is G itself)
    du, gw1, gb1, gw2, gb2 = torch.autograd.grad((out * G.double()).sum(), p)
    m_ref = (du - G.double() * s_ref.detach()[:, None, None, :])[:, 0, 0, :]  # the part of du that is constant over pixels
    want = dict(m=m_ref, gw1=gw1, gb1=gb1, gw2=gw2, gb2=gb2)
    # ---- device: the training forward's s and mean, then the backward
    L, st = _lib.load(), _lib.stream_ptr()
    d = {k: v.to(DEV).contiguous() for k, v in dict(u=u, G=G, w1=w1, b1=b1, w2=w2, b2=b2).items()}
    s = torch.empty((n, c), device=DEV)
    mean = torch.empty((n, c), device=DEV)
    fws = torch.empty(L.climsr_channel_attention_workspace(n, c) // 8, dtype=torch.float64, device=DEV)
    check(L.climsr_channel_attention_keep(ptr(d["u"]), n, h * w, c, c, ptr(d["w1"]), ptr(d["b1"]), ptr(d["w2"]), ptr(d["b2"]), cr,
                                          ptr(fws), ptr(s), ptr(mean), st), "ca keep")
    s_plain = torch.empty_like(s)
    check(L.climsr_channel_attention(ptr(d["u"]), n, h * w, c, c, ptr(d["w1"]), ptr(d["b1"]), ptr(d["w2"]), ptr(d["b2"]), cr,
                                     ptr(fws), ptr(s_plain), st), "ca")
    ud = d["u"].to(torch.bfloat16) if u_bf16 else d["u"]
    bws = torch.empty((L.climsr_channel_attention_bwd_workspace(n, c, cr) + 7) // 8, dtype=torch.float64, device=DEV)

    def run(acc, grads=None):
        o = dict(m=torch.empty((n, c), device=DEV), dzu=torch.empty((n, h, w, c), dtype=torch.bfloat16, device=DEV))
        o.update(grads or dict(gw1=torch.empty((cr, c), device=DEV), gb1=torch.empty((cr,), device=DEV),
                               gw2=torch.empty((c, cr), device=DEV), gb2=torch.empty((c,), device=DEV)))
        check(L.climsr_channel_attention_bwd(ptr(d["G"]), c, ptr(ud), u_bf16, c, ptr(s), ptr(mean), n, h * w, c, ptr(d["w1"]),
                                             ptr(d["b1"]), ptr(d["w2"]), cr, ptr(bws), ptr(o["m"]), ptr(o["gw1"]), ptr(o["gb1"]),
                                             ptr(o["gw2"]), ptr(o["gb2"]), acc, ptr(o["dzu"]), c, st), "ca bwd")
        torch.cuda.synchronize()
        return o

    a = run(0)
    assert torch.equal(s, s_plain)  # the keep form computes the same scale
    assert (mean.cpu().double() - u.double().mean(dim=(1, 2))).abs().max() <= 1e-6
    for k, ref_t in want.items():
        err, scale = float((a[k].cpu().double() - ref_t).abs().max()), float(ref_t.abs().max())
        print(f"ca bwd {k}: max abs err {err:.3e}, reference max-abs {scale:.3e}")
        assert err <= 1e-5 * scale, (k, err, scale)
    z_ref = (G.double() * s.cpu().double()[:, None, None, :] + a["m"].cpu().double()[:, None, None, :]).to(torch.bfloat16).double()
    diff = (a["dzu"].cpu().double() - z_ref).abs()
    assert bool((diff <= 2.0 ** -8 * z_ref.abs()).all()), float((diff / z_ref.abs().clamp_min(1e-30)).max())
    again = run(0)
    assert all(torch.equal(a[k], again[k]) for k in a), "reruns must be bit-identical"
    acc = {k: torch.zeros_like(a[k]) for k in ("gw1", "gb1", "gw2", "gb2")}
    run(1, acc)
    two = run(1, acc)
    for k in acc:
        assert torch.allclose(two[k], 2 * a[k], rtol=1e-6, atol=0), k
    assert torch.equal(two["dzu"], a["dzu"]) and torch.equal(two["m"], a["m"])


# ------------------------------------------------------------------------------------------------ model
def rcan_kwargs(ng, nb, sf):
    return dict(n_resgroups=ng, n_resblocks=nb, n_feats=64, reduction=16, scaling_factor=sf, in_channels=3, out_channels=1)


_STATE = {}


def init_params(ng, nb, sf):
    """The deterministic test weights (fp64, keyed like the reference), built once per configuration."""
    key = (ng, nb, sf)
    if key not in _STATE:
        from climsr_amd.models.rcan import RCAN

        shapes = {k: tuple(v.shape) for k, v in RCAN(**rcan_kwargs(ng, nb, sf)).state_dict().items()}
        st = init_state(spec_from_shapes(shapes))
        _STATE[key] = {k: torch.from_numpy(np.asarray(v)).double() for k, v in st.items()}
    return _STATE[key]


def build(ng, nb, sf):
    from climsr_amd.models.rcan import TrainableRCAN

    net = TrainableRCAN(**rcan_kwargs(ng, nb, sf))
    net.load_state_dict({k: v.float() for k, v in init_params(ng, nb, sf).items()}, strict=True)
    return net.to(DEV)


def test_keep_nokeep_and_rcan_forward_are_bit_identical():
    from climsr_amd.models.rcan import RCAN

    ng, nb, sf, b, lr = CONFIGS["g2b2_x4"]
    net = build(ng, nb, sf).train()
    bt = ref.synthetic_batch(b, lr * sf, seed=5, scale=sf)
    args = [bt[k].to(DEV) for k in ("lr", "elevation", "mask")]
    kept = net(*args)
    assert kept.requires_grad and kept.grad_fn is not None
    net.eval()
    with torch.no_grad():
        plain = net(*args)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    inf = RCAN(**rcan_kwargs(ng, nb, sf))
    inf.load_state_dict(sd, strict=True)  # a checkpoint saved from one class loads into the other
    inf = inf.to(DEV).eval()
    with torch.no_grad():
        want = inf(*args)
    torch.cuda.synchronize()
    assert torch.equal(kept.detach(), plain), "keep / no-keep forward paths must be bit-identical"
    assert torch.equal(plain, want), "TrainableRCAN's no-grad forward must equal RCAN's"
    with pytest.raises(NotImplementedError, match="inputs"):
        x = args[0].clone().requires_grad_(True)
        net.train()(x, args[1], args[2]).sum().backward()


def pooled(t):
    """The comparison layout: every channel-attention (``.conv_du.``) tensor in one vector, the rest as they are (the
    tensors under POOL_BELOW elements among them are pooled by update_envelope / pool_small)."""
    out = {k: v for k, v in t.items() if ".conv_du." not in k}
    out["<all .conv_du. tensors>"] = torch.cat([v.reshape(-1).double() for k, v in t.items() if ".conv_du." in k])
    return out


def oracle_grads(p, bt, cfg, dev, dtype, autocast=None, scale=1.0):
    """(loss, gradients) of the oracle's L1 loss at ``p``; under autocast the loss is scaled as precision=16's GradScaler
    scales it (from 2^16, halved while a gradient overflows, as the scaler does)."""
    ng, nb, sf = cfg
    keys = list(p)
    q = {k: v.detach().clone().to(dev, dtype).requires_grad_(True) for k, v in p.items()}  # fresh leaves: p stays as it is
    b_ = {k: v.to(dev, dtype) for k, v in bt.items()}
    while True:
        with torch.autocast("cuda", dtype=autocast or torch.float16, enabled=autocast is not None):
            sr = ref.rcan_forward(q, b_["lr"], b_["elevation"], b_["mask"], ng, nb, sf)
        loss = ref.l1_loss(sr.to(dtype), b_["hr"])
        gs = torch.autograd.grad(loss * scale, [q[k] for k in keys])
        if all(torch.isfinite(g).all() for g in gs) or scale <= 1.0:
            break
        scale /= 2.0
    assert all(torch.isfinite(g).all() for g in gs)
    return float(loss.detach()), {k: g.double().cpu() / scale for k, g in zip(keys, gs)}


def autocast_runs(fn, monkeypatch):
    with monkeypatch.context() as mp:
        mp.setattr(ref, "_conv", gemm_conv)  # rocBLAS GEMMs on the GPU (no MIOpen per-shape compiles)
        torch.backends.cuda.matmul.allow_tf32 = False
        return [fn(dt, sc) for dt, sc in ((torch.float16, 2.0 ** 16), (torch.bfloat16, 1.0))]


def check_envelope(what, native, want, amps):
    native, want, amps = pooled(native), pooled(want), [pooled(a) for a in amps]
    bad, worst, rows = update_envelope(native, want, amps, pool_below=POOL_BELOW)
    nat, w64 = pool_small(native, POOL_BELOW), pool_small(want, POOL_BELOW)
    assert set(nat) == set(w64) == set(rows)  # no tensor excluded
    cos = {k: float((nat[k].double() * w64[k].double()).sum() / (nat[k].double().norm() * w64[k].double().norm() + 1e-30)) for k in w64}
    kc = min(cos, key=cos.get)
    ratios = sorted(r / max(2.0 * ra, 2e-2) for r, ra in rows.values())
    print(f"{what}: {len(rows)} compared tensors, worst {worst}, native / bound median {ratios[len(ratios) // 2]:.3f} max "
          f"{ratios[-1]:.3f}, min cosine {cos[kc]:.5f} ({kc})", flush=True)
    assert not bad, f"{what}: {len(bad)} tensors outside 2x the autocast spread: {bad[:8]}"
    low = [(k, round(c, 4)) for k, c in cos.items() if c < 0.97]
    assert not low, f"{what}: cosine under 0.97: {low[:8]}"


@pytest.mark.parametrize("name", list(CONFIGS))
def test_parameter_gradients_vs_fp64_oracle(name, monkeypatch):
    from climsr_amd.losses.l1 import l1_loss

    ng, nb, sf, b, lr = CONFIGS[name]
    cfg = (ng, nb, sf)
    net = build(*cfg).train()
    p64 = init_params(*cfg)
    bt = ref.synthetic_batch(b, lr * sf, seed=3, scale=sf)
    loss = l1_loss(net(bt["lr"].to(DEV), bt["elevation"].to(DEV), bt["mask"].to(DEV)), bt["hr"].to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    got = {k: v.grad.double().cpu().clone() for k, v in net.named_parameters()}
    assert set(got) == set(p64)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    l64, g64 = oracle_grads(p64, bt, cfg, "cpu", torch.float64)
    print(f"{name}: native loss {float(loss):.8f}, fp64 oracle {l64:.8f}")
    assert abs(float(loss) - l64) <= 2e-3 * abs(l64)
    amps = autocast_runs(lambda dt, sc: oracle_grads(p64, bt, cfg, DEV, torch.float32, dt, sc)[1], monkeypatch)
    check_envelope(f"{name} gradients", got, g64, amps)


def test_grad_accumulation_semantics():
    from climsr_amd.losses.l1 import l1_loss

    ng, nb, sf, _b, lr = CONFIGS["g2b2_x4"]
    net = build(ng, nb, sf).train()
    bt = ref.synthetic_batch(1, lr * sf, seed=4, scale=sf)
    args = [bt[k].to(DEV) for k in ("lr", "elevation", "mask")]
    hr = bt["hr"].to(DEV)
    l1_loss(net(*args), hr).backward()
    g1 = net._flat_grad.clone()
    l1_loss(net(*args), hr).backward()  # accumulates (grads left linked)
    g2 = net._flat_grad.clone()
    assert torch.allclose(g2, 2 * g1, rtol=1e-5, atol=1e-9)
    for p in net.parameters():
        p.grad = None  # zero_grad(set_to_none=True) -> the next backward overwrites
    l1_loss(net(*args), hr).backward()
    torch.cuda.synchronize()
    assert torch.equal(net._flat_grad, g1)
    # the other gradient route of core/flat.py (torch DDP): the same values handed to autograd's AccumulateGrad
    seen = []
    net.set_grad_ready_hook(seen.append)
    l1_loss(net(*args), hr).backward()
    assert seen == [0]  # one bucket, once, at the end of backward
    net.set_grad_ready_hook(None)
    for p in net.parameters():
        p.grad = None
    net.grads_through_autograd = True
    l1_loss(net(*args), hr).backward()
    torch.cuda.synchronize()
    via = torch.cat([p.grad.reshape(-1) for p, _o, _n in net._flat_index])
    assert torch.equal(via, g1)


def test_three_pretraining_steps_through_task_and_trainer(monkeypatch):
    from climsr_amd.core.optim import AdamW
    from climsr_amd.core.trainer import Trainer
    from climsr_amd.task.pl_generator_pre_training import SuperResolutionLightningModule

    ng, nb, sf, b, lr_size = CONFIGS["g2b2_x4"]
    cfg, total, seeds = (ng, nb, sf), 10, (100, 101, 102)
    m = SuperResolutionLightningModule(
        generator=dict(rcan_kwargs(*cfg), _target_="climsr_amd.models.rcan.TrainableRCAN"), generator_type="rcan",
        optimizers={"generator_optimizer": dict(ADAMW_YAML)}, schedulers={"generator_scheduler": dict(ONE_CYCLE_YAML)})
    init = init_params(*cfg)
    m.generator.load_state_dict({k: v.float() for k, v in init.items()}, strict=True)
    m = m.to(DEV)
    tr = Trainer(m, limit_train_batches=total, max_epochs=1)
    assert type(tr.optimizers[0]) is AdamW and tr.optimizers[0].owner is m.generator  # the fused flat-buffer update
    assert tr.schedulers[0]["scheduler"].total_steps == total
    assert type(m.loss).__name__ == "L1Loss"
    batches = [ref.synthetic_batch(b, lr_size * sf, seed=s, scale=sf) for s in seeds]
    losses = []
    for i, bt in enumerate(batches):
        out = tr.training_batch({k: v.to(DEV) for k, v in bt.items()}, i)
        losses.append(float(out[0].detach()))
    torch.cuda.synchronize()
    upd = {k: p.detach().double().cpu() - init[k] for k, p in m.generator.named_parameters()}
    keys = list(init)

    def oracle_steps(dev, dtype, autocast=None, scale=1.0):
        """The oracle's three steps (ref.rcan_forward, L1, AdamW + OneCycleLR): per-step losses, the parameter update."""
        q = {k: v.detach().clone().to(dev, dtype) for k, v in init.items()}
        opt = ref.AdamWState(q, keys, lr=1e-4, total_steps=total)
        out = []
        for bt in batches:
            b_ = {k: v.to(dev, dtype) for k, v in bt.items()}
            for k in keys:
                q[k].requires_grad_(True)
            while True:
                with torch.autocast("cuda", dtype=autocast or torch.float16, enabled=autocast is not None):
                    sr = ref.rcan_forward(q, b_["lr"], b_["elevation"], b_["mask"], ng, nb, sf)
                loss = ref.l1_loss(sr.to(dtype), b_["hr"])
                grads = ref._grads(loss * scale, q, keys)
                if all(torch.isfinite(g).all() for g in grads.values()) or scale <= 1.0:
                    break
                scale /= 2.0  # precision=16's GradScaler backs off the same way
            grads = {k: g / scale for k, g in grads.items()}
            for k in keys:
                q[k].requires_grad_(False)
            out.append(float(loss.detach()))
            opt.step(q, grads)
            opt.sched()
        return out, {k: q[k].double().cpu() - init[k] for k in keys}

    torch.set_num_threads(min(16, torch.get_num_threads()))
    l64, u64 = oracle_steps("cpu", torch.float64)
    print("rcan trainer losses", losses, "fp64 oracle", l64)
    for got, want in zip(losses, l64):
        assert abs(got - want) <= 2e-3 * abs(want), (losses, l64)
    amps = autocast_runs(lambda dt, sc: oracle_steps(DEV, torch.float32, dt, sc)[1], monkeypatch)
    check_envelope("rcan 3-step update", upd, u64, amps)
