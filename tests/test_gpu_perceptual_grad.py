"""``PerceptualLoss(differentiable=True)`` on the GPU: the new kernels alone, the backward against the routed fp64
reference (tests/perceptual_ref.py), value and determinism, a wiring guard against the fp64 oracle's autograd, the
task switch and graph mode.

Inputs: hr = U(-1, 1), sr = hr + 0.2 N(0, 1), seeded.  Shapes (n, h, w): (2, 32, 32); (1, 48, 80), non-square with
3 x 5 maps at the last level; (2, 64, 64), the smallest whose data gradients reach the LDS-DMA conv (conv2_1 / conv2_2
at 32 x 32; at the other two shapes every data gradient stays on the generic, 64 -> 64 and 16-output kernels).

The kernel check is ``test_backward_vs_routed_reference``: ``exact`` is the fp64 gradient through the *stored* bf16
forward (every sign, mask and argmax read from the stored maps), ``rounded`` the same with each inter-layer gradient
rounded to bf16 -- the one thing the kernels may differ in -- and the native gradient must be within 2x of rounded's
distance from exact (the project's envelope convention, helpers.update_envelope).  Both come from the reference alone.
"""
import pytest
import torch
import torch.nn.functional as F

from climsr_amd import ops
from climsr_amd._lib import ClimsrError
from oracle import climsr_ref as ref
from tests.helpers import gen_params, rel_l2, rfb_d_params, update_envelope, vgg_params
from tests.perceptual_ref import bf16_round, routed_backward

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 0x7B7B
SHAPES = [(2, 32, 32), (1, 48, 80), (2, 64, 64)]
IDS = ["%dx%dx%d" % s for s in SHAPES]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu()


def sentinel_bf16(shape):
    return torch.full(shape, SENT, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def refused(call):
    with pytest.raises(ClimsrError, match=r"rc=-1"):
        call()


def images(n, h, w):
    g = gen(1000 + n + h + w)
    hr = torch.rand((n, 1, h, w), generator=g) * 2 - 1
    sr = hr + 0.2 * torch.randn((n, 1, h, w), generator=g)
    return hr, sr


# --------------------------------------------------------------------------------------------------------------
# 1. the new kernels, exact
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [8, 64])
@pytest.mark.parametrize("n,h,w", [(1, 2, 2), (2, 6, 10), (1, 16, 16)])
def test_maxpool2_relu_bwd_is_the_torch_rule(n, h, w, c):
    """Few distinct values (ties inside most windows), negative and +-0 entries, planted all-zero, all-equal-positive
    and all-negative windows; the routing is a copy, so the result is torch's fp64 rule bit for bit."""
    g = gen(7000 + h * w + c)
    y = torch.randint(-1, 4, (n, h, w, c), generator=g).float() * 0.5
    y[y < 0] = 0.0  # a post-ReLU map: zeros and a few positive levels
    y[0, 0:2, 0:2, :] = 0.0  # an all-zero window: passes nothing
    y[0, 0, 1, 0] = -0.0
    if h >= 6:
        y[0, 2:4, 2:4, :] = 1.5  # four equal maxima: the first one, (0, 0)
        y[0, 4:6, 0:2, :] = 0.0
        y[0, 5, 0:2, :] = 2.0    # two equal maxima in the second row: (1, 0)
        y[0, 0:2, 2:4, :] = -1.0  # no ReLU output is negative, but the rule is max > 0: nothing passes
    y = y.to(torch.bfloat16)
    gp = torch.randn((n, h // 2, w // 2, c), generator=g).to(torch.bfloat16)
    dz = sentinel_bf16((n, h, w, c))
    ops.maxpool2_relu_bwd(gp.to(DEV), y.to(DEV), n, h, w, c, dz)
    torch.cuda.synchronize()
    y64 = y.double().permute(0, 3, 1, 2)
    _m, ind = F.max_pool2d(y64, 2, 2, return_indices=True)
    want = F.max_unpool2d(gp.double().permute(0, 3, 1, 2), ind, 2, 2, output_size=(h, w)) * (y64 > 0)
    want = want.permute(0, 2, 3, 1).to(torch.bfloat16)
    assert torch.equal(bits(dz), bits(want + 0.0))  # (+ 0.0: the product's -0 where a negative gp meets a closed mask)
    assert int((dz != 0).sum()) > 0 or h == 2


@pytest.mark.parametrize("h,w,c", [(3, 4, 8), (4, 3, 8), (4, 4, 12)])
def test_maxpool2_relu_bwd_refuses(h, w, c):
    y = torch.zeros((2, h, w, c), dtype=torch.bfloat16, device=DEV)
    gp = torch.zeros((2, h // 2 + 1, w // 2 + 1, c + 8), dtype=torch.bfloat16, device=DEV)
    dz = sentinel_bf16((2, h + 1, w + 1, c + 8))
    refused(lambda: ops.maxpool2_relu_bwd(gp, y, 2, h, w, c, dz))
    torch.cuda.synchronize()
    assert bool((bits(dz) == SENT).all())


@pytest.mark.parametrize("n", [8, 2048 + 8, 8 * 256 * 3 + 16])
def test_l1_sign_bf16(n):
    g = gen(7100 + n % 89)
    a = torch.randn((n,), generator=g).to(torch.bfloat16)
    b = torch.randn((n,), generator=g).to(torch.bfloat16)
    b[::3] = a[::3]  # planted equal elements: sign(0) = 0
    a[1], b[1] = 1e-38, 2e-38  # a difference below the smallest normal fp32 still has a sign
    a[2], b[2] = 0.0, -0.0
    out = sentinel_bf16((n + 8,))
    ops.l1_sign_bf16(a.to(DEV), b.to(DEV), n, out)
    torch.cuda.synchronize()
    want = torch.sign(a.double() - b.double()).to(torch.bfloat16)
    assert torch.equal(bits(out[:n]), bits(want)) and bool((bits(out[n:]) == SENT).all())
    assert int((want == 0).sum()) >= n // 3 and int((want > 0).sum()) > 0 and int((want < 0).sum()) > 0


def test_l1_sign_and_sum3_refuse_bad_arguments():
    a = torch.zeros((16,), dtype=torch.bfloat16, device=DEV)
    out = sentinel_bf16((16,))
    refused(lambda: ops.l1_sign_bf16(a, a, 12, out))
    refused(lambda: ops.l1_sign_bf16(a, a, 0, out))
    x = torch.zeros((4, 4), device=DEV)
    o = torch.full((4,), 3.0, device=DEV)
    refused(lambda: ops.sum3_scale(x, 4, None, 1.0, 8, o))
    refused(lambda: ops.sum3_scale(x, 4, o, 1.0, 0, o))
    torch.cuda.synchronize()
    assert bool((bits(out) == SENT).all()) and bool((o == 3.0).all())


def test_sum3_scale():
    """Three channels of rows of four (the fourth is not read: NaN here), times sign * gscale / numel, in fp32."""
    g = gen(7200)
    npix = 1000
    x = torch.randn((npix, 4), generator=g)
    x[:, 3] = float("nan")
    gs = torch.tensor(0.37, device=DEV)
    out = torch.full((npix + 3,), 5.0, device=DEV)
    ops.sum3_scale(x.to(DEV), npix, gs, -1.0, 4096, out)
    torch.cuda.synchronize()
    want = x[:, :3].double().sum(1) * (-0.37 / 4096)
    # two fp32 additions, the scale's two roundings (and 0.37's own) and the product: each at most 2^-24 of a partial
    # sum no larger than |x0| + |x1| + |x2|, six of them
    bound = 6 * 2.0 ** -24 * x[:, :3].double().abs().sum(1) * (0.37 / 4096)
    assert bool(((out[:npix].double().cpu() - want).abs() <= bound).all())
    assert bool((out[npix:] == 5.0).all())


# --------------------------------------------------------------------------------------------------------------
# 2. the backward against the routed reference
# --------------------------------------------------------------------------------------------------------------
_MODS = {}


def module(**kw):
    """One module per option set, shared (its packed weights are built once)."""
    from climsr_amd.losses.perceptual import PerceptualLoss

    key = tuple(sorted(kw.items()))
    if key not in _MODS:
        _MODS[key] = PerceptualLoss(**kw).to(DEV)
    return _MODS[key]


def weights_bf16():
    """The weights the native convs multiply with: the module's fp32 weights rounded to bf16, as fp64."""
    return {k: bf16_round(v).double() for k, v in vgg_params(torch.float32).items()}


def nchw64(t):
    return t.detach().permute(0, 3, 1, 2).double().cpu()


def run_native(n, h, w, which, gout=None):
    """Forward + backward of the differentiable module on (hr, sr) in the task's order; which: 1 = gradient to the
    second argument, 0 = to the first, 2 = both.  -> (loss, [grad or None] * 2, saved)."""
    hr, sr = images(n, h, w)
    a = hr.to(DEV).requires_grad_(which in (0, 2))
    b = sr.to(DEV).requires_grad_(which in (1, 2))
    m = module(differentiable=True, retain_saved=True)
    loss = m(a, b)
    assert loss.grad_fn is not None
    if gout is None:
        loss.backward()
    else:
        loss.backward(gout)
    torch.cuda.synchronize()
    saved, m.saved = m.saved, None
    return loss.detach(), [a.grad, b.grad], saved


def check_against_routed(native, acts, f_own, f_other, scale=1.0, what=""):
    p = weights_bf16()
    acts64 = [nchw64(t) for t in acts]
    fo, ft = nchw64(f_own), nchw64(f_other)
    exact = routed_backward(p, acts64, fo, ft) * scale
    rounded = routed_backward(p, acts64, fo, ft, round=bf16_round) * scale
    e_model, e_native = rel_l2(rounded, exact), rel_l2(native.double().cpu(), exact)
    print(f"{what}: rel L2 vs exact: bf16-rounded chain {e_model:.3e}, native {e_native:.3e}", flush=True)
    assert native.shape == exact.shape and native.dtype == torch.float32
    assert float(exact.abs().max()) > 0
    assert e_model <= 1e-2, f"{what}: the inputs' rounded chain is {e_model:.3e} from exact"
    assert e_native <= 2.0 * e_model, f"{what}: native {e_native:.3e} > 2 x {e_model:.3e}"


@pytest.mark.parametrize("n,h,w", SHAPES, ids=IDS)
def test_backward_vs_routed_reference_second_argument(n, h, w):
    _loss, grads, s = run_native(n, h, w, 1)
    assert grads[0] is None and s["which"] == 1 and len(s["acts"]) == 16
    check_against_routed(grads[1], s["acts"], s["f_grad"], s["f_const"], what="d/d second")


@pytest.mark.parametrize("n,h,w", SHAPES, ids=IDS)
def test_backward_vs_routed_reference_first_argument(n, h, w):
    _loss, grads, s = run_native(n, h, w, 0)
    assert grads[1] is None and s["which"] == 0 and len(s["acts"]) == 16
    check_against_routed(grads[0], s["acts"], s["f_grad"], s["f_const"], what="d/d first")


@pytest.mark.parametrize("n,h,w", SHAPES, ids=IDS)
def test_backward_vs_routed_reference_both_arguments(n, h, w):
    """Both halves keep their maps; the seeds sign(f_a - f_b) and sign(f_b - f_a) are negatives of each other, each
    gradient runs through its own half's masks and argmaxes, and each equals the one-sided run's bit for bit."""
    _loss, grads, s = run_native(n, h, w, 2)
    assert s["which"] == 2
    check_against_routed(grads[0], s["acts"], s["f_grad"], s["f_const"], what="both: d/d first")
    check_against_routed(grads[1], s["acts2"], s["f_const"], s["f_grad"], what="both: d/d second")
    assert torch.equal(bits(grads[0]), bits(run_native(n, h, w, 0)[1][0]))
    assert torch.equal(bits(grads[1]), bits(run_native(n, h, w, 1)[1][1]))


def test_backward_with_a_device_grad_output():
    n, h, w = SHAPES[0]
    _loss, grads, s = run_native(n, h, w, 1, gout=torch.tensor(0.37, device=DEV))
    check_against_routed(grads[1], s["acts"], s["f_grad"], s["f_const"], scale=0.37, what="grad_output 0.37")


# --------------------------------------------------------------------------------------------------------------
# 3. value and determinism
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", SHAPES, ids=IDS)
def test_value_is_the_default_modules_and_runs_repeat(n, h, w):
    hr, sr = images(n, h, w)
    with torch.no_grad():
        want = module()(hr.to(DEV), sr.to(DEV))
        plain = module(differentiable=True)(hr.to(DEV), sr.to(DEV).requires_grad_(True))
    assert want.grad_fn is None and plain.grad_fn is None and not plain.requires_grad
    assert module(differentiable=True)(hr.to(DEV), sr.to(DEV)).grad_fn is None  # nothing requires grad: today's path
    assert module()(hr.to(DEV), sr.to(DEV).requires_grad_(True)).grad_fn is None  # the default never carries a node
    runs = [run_native(n, h, w, which) for which in (1, 1, 0, 2)]
    for loss, _g, _s in runs:
        assert torch.equal(bits(loss), bits(want)) and torch.equal(bits(plain), bits(want))
    assert torch.equal(bits(runs[0][1][1]), bits(runs[1][1][1]))
    assert float(runs[0][1][1].abs().max()) > 0


def test_retain_saved_defaults_off_and_second_backward_is_refused():
    n, h, w = SHAPES[0]
    hr, sr = images(n, h, w)
    m = module(differentiable=True)
    loss = m(hr.to(DEV), sr.to(DEV).requires_grad_(True))
    assert m.saved is None
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="a second time"):
        loss.backward()


# --------------------------------------------------------------------------------------------------------------
# 4. wiring guard against the fp64 oracle
# --------------------------------------------------------------------------------------------------------------
def oracle_grad(p, hr, sr, autocast=None):
    hr, sr = hr.to(p["loss_network.0.weight"].dtype), sr.to(p["loss_network.0.weight"].dtype).requires_grad_(True)
    with torch.autocast("cpu", dtype=autocast or torch.bfloat16, enabled=autocast is not None):
        loss = (ref.vgg19_features(p, torch.cat([hr] * 3, 1)) - ref.vgg19_features(p, torch.cat([sr] * 3, 1))).abs().mean()
    return torch.autograd.grad(loss.float() if autocast else loss, sr)[0].double()


@pytest.mark.parametrize("n,h,w", SHAPES[:2], ids=IDS[:2])
def test_wiring_against_the_fp64_oracle(n, h, w):
    """Catches swapped arguments, a wrong sign or a missing scale only: the native gradient against fp64 autograd of the
    oracle VGG (fp32 weights, nothing taken from the native run), within 2x the spread of the oracle's own CPU autocast
    bf16 and fp16 runs (update_envelope).  That spread is large by nature -- a 16-layer chain of sign, mask and argmax
    decisions flips under any 16-bit rounding (0.1 .. 0.3 here) -- so this says nothing about the kernels' arithmetic;
    test_backward_vs_routed_reference_* is the kernel check."""
    hr, sr = images(n, h, w)
    _loss, grads, _s = run_native(n, h, w, 1)
    want = oracle_grad(vgg_params(torch.float64), hr, sr)
    p32 = vgg_params(torch.float32)
    amps = [{"g": oracle_grad(p32, hr, sr, dt)} for dt in (torch.bfloat16, torch.float16)]
    bad, worst, rows = update_envelope({"g": grads[1].double().cpu()}, {"g": want}, amps)
    print("native vs fp64 oracle, rel L2 (native, autocast spread):", rows["g"], flush=True)
    assert not bad, bad
    assert rel_l2(-grads[1].double().cpu(), want) > 1.0  # (a flipped sign is far outside)


# --------------------------------------------------------------------------------------------------------------
# 5. the task
# --------------------------------------------------------------------------------------------------------------
ESRGAN_CFG = {"_target_": "climsr_amd.models.esrgan.ESRGANGenerator", "in_channels": 3, "out_channels": 1, "nf": 64, "nb": 1,
              "gc": 16, "scale_factor": 4}
RFB_D = {"_target_": "climsr_amd.models.rfb_esrgan.RFBESRGANDiscriminator", "in_channels": 1}
ADAMW = {"_target_": "torch.optim.AdamW", "lr": 1e-4, "weight_decay": 1e-4}
TOTAL = 10
ONE_CYCLE = {"_target_": "torch.optim.lr_scheduler.OneCycleLR", "max_lr": 1e-4, "num_training_steps": TOTAL, "pct_start": 0.3,
             "div_factor": 2, "final_div_factor": 100}
PERCEPTUAL_ONLY = dict(pixel_level_loss_factor=0.0, adversarial_loss_factor=0.0, perceptual_loss_factor=1.0)


def make_task(option, **factors):
    from climsr_amd.task.pl_gan import GANLightningModule

    m = GANLightningModule(generator=dict(ESRGAN_CFG), discriminator=dict(RFB_D),
                           optimizers={"generator_optimizer": dict(ADAMW), "discriminator_optimizer": dict(ADAMW)},
                           schedulers={"generator_scheduler": dict(ONE_CYCLE), "discriminator_scheduler": dict(ONE_CYCLE)},
                           differentiable_perceptual_loss=option, **factors)
    m.generator.load_state_dict(gen_params(1, torch.float32))
    m.discriminator.load_state_dict(rfb_d_params(torch.float32))
    return m.to(DEV)


def small_batch(seed=42):
    return {k: v.to(DEV) for k, v in ref.synthetic_batch(2, 64, seed=seed).items()}


def g_pass(m, bt):
    """The generator's pass of one GAN step as the Trainer runs it (D's parameters frozen) -> (generator gradients,
    the (hr, sr) the criterion saw, the gradient that reached sr)."""
    seen = {}
    crit = m.perceptual_criterion.forward

    def spy(hr, sr):
        seen["hr"], seen["sr"] = hr.detach().clone(), sr.detach().clone()
        if sr.requires_grad:
            sr.register_hook(lambda g: seen.__setitem__("g_sr", g.detach().clone()))
        return crit(hr, sr)

    m.perceptual_criterion.forward = spy
    for p in m.discriminator.parameters():
        p.requires_grad_(False)
    try:
        out = m.training_step(bt, 0, 0)
        out["loss"].backward()
    finally:
        m.perceptual_criterion.forward = crit
        for p in m.discriminator.parameters():
            p.requires_grad_(True)
    torch.cuda.synchronize()
    return {k: p.grad for k, p in m.generator.named_parameters()}, seen


def test_task_option_trains_g_through_the_perceptual_term():
    bt = small_batch()
    off, _seen = g_pass(make_task(False, **PERCEPTUAL_ONLY), bt)
    assert all(g is None or not bool(g.any()) for g in off.values())  # F7: the reference's term gives G no gradient
    m = make_task(True, **PERCEPTUAL_ONLY)
    on, seen = g_pass(m, bt)
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in on.values())
    assert sum(int(bool(g.any())) for g in on.values()) > len(on) // 2 and bool(on["conv_first.weight"].any())
    # the gradient at sr is the module's own on the same (hr, sr); the other two terms' factor-0 gradients add +-0,
    # which can only turn a -0 into +0: compared as floats
    sr = seen["sr"].clone().requires_grad_(True)
    m.perceptual_criterion(seen["hr"], sr).backward()
    assert torch.equal(seen["g_sr"], sr.grad) and bool(sr.grad.any())


def val_batch():
    """A validation batch of the device tile pipeline (tests/test_gpu_pipeline_metrics.py); made anew per use: the step
    masks its hr in place."""
    import numpy as np

    from climsr_amd.data import DeviceTilePipeline

    rs = np.random.RandomState(14)
    raw = rs.rand(2, 64, 64).astype(np.float32) * 30 - 5
    raw[:, :10, :] = np.nan
    elev = (rs.rand(2, 64, 64) * 1000).astype(np.float32)
    return DeviceTilePipeline(stage="val")(torch.from_numpy(raw).to(DEV), torch.from_numpy(elev).to(DEV), [-6.0, -6.0], [26.0, 26.0])


def test_validation_step_is_unchanged_by_the_option():
    vals = []
    for option in (False, True):
        m = make_task(option, normalization_method="minmax", normalization_range=(-1.0, 1.0)).eval()
        with torch.no_grad():
            out = m.validation_step(val_batch(), 0)
        vals.append(out["val/perceptual_loss"])
        assert out["val/perceptual_loss"].grad_fn is None
    torch.cuda.synchronize()
    assert torch.equal(bits(vals[0]), bits(vals[1])) and float(vals[0]) > 0


# --------------------------------------------------------------------------------------------------------------
# 6. graph mode
# --------------------------------------------------------------------------------------------------------------
def test_graph_steps_replay_the_step_with_the_option_on():
    """tests/test_gpu_graph_steps.py's pattern on the small GAN workload with the option on (the task's default loss
    factors): 2 eager warm-up steps, a capture, 3 replayed steps, against 5 eager device-stepped steps (graph_warmup = 5:
    nothing captured), every step on a batch of its own; parameters, Adam moments and buffers bit for bit."""
    from climsr_amd.core.trainer import Trainer
    from tests.test_gpu_graph_steps import assert_bit_identical, losses_of, snapshot

    def run(**kw):
        m = make_task(True)
        tr = Trainer(m, num_training_steps=TOTAL, graph_steps=True, **kw)
        losses = [[float(x) for x in losses_of(tr.training_batch(small_batch(200 + i), i))] for i in range(5)]
        snap = snapshot(m, tr)
        torch.cuda.synchronize()
        return losses, snap, dict(tr.graph_stats)

    la, sa, stats_a = run(graph_warmup=2)
    lb, sb, stats_b = run(graph_warmup=5)
    assert stats_a == {"captures": 1, "replayed": 3, "eager": 2} and stats_a["replayed"] > 0
    assert stats_b == {"captures": 0, "replayed": 0, "eager": 5}
    assert la == lb and len({tuple(row) for row in la}) == 5
    assert_bit_identical(sa, sb)
