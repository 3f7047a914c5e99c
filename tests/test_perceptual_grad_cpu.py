"""The opt-in backward of the perceptual term, the parts that need no GPU: the fp64 yardstick the GPU tests judge the
kernels with (tests/perceptual_ref.py) is pinned against torch.autograd first, then the switches -- the module's
``differentiable`` flag, the task's ``differentiable_perceptual_loss`` hparam -- and that the defaults build today's
objects and CPU tensors are still refused."""
import pytest
import torch

from oracle import climsr_ref as ref
from tests.helpers import rel_l2, vgg_params
from tests.perceptual_ref import forward_acts, routed_backward

ESRGAN_CFG = {"_target_": "climsr_amd.models.esrgan.ESRGANGenerator", "in_channels": 3, "out_channels": 1, "nf": 64, "nb": 1,
              "gc": 16, "scale_factor": 4}
RFB_D = {"_target_": "climsr_amd.models.rfb_esrgan.RFBESRGANDiscriminator", "in_channels": 1}


def cat3(x):
    return torch.cat([x, x, x], 1)


def test_routed_backward_is_autograd_in_fp64():
    """With an fp64 forward's own stored maps the recipe is torch.autograd's gradient, for either argument."""
    p = vgg_params(torch.float64)
    g = torch.Generator().manual_seed(3)
    hr = torch.rand((2, 1, 32, 32), generator=g, dtype=torch.float64) * 2 - 1
    sr = (hr + 0.2 * torch.randn((2, 1, 32, 32), generator=g, dtype=torch.float64)).requires_grad_(True)
    hr.requires_grad_(True)
    loss = (ref.vgg19_features(p, cat3(hr)) - ref.vgg19_features(p, cat3(sr))).abs().mean()
    want_hr, want_sr = torch.autograd.grad(loss, (hr, sr))
    with torch.no_grad():
        acts_hr, f_hr = forward_acts(p, cat3(hr))
        acts_sr, f_sr = forward_acts(p, cat3(sr))
        got_sr = routed_backward(p, acts_sr, f_sr, f_hr)
        got_hr = routed_backward(p, acts_hr, f_hr, f_sr)
    assert float(want_sr.abs().max()) > 0 and got_sr.shape == sr.shape
    e_sr, e_hr = rel_l2(got_sr, want_sr), rel_l2(got_hr, want_hr)
    print("routed_backward vs autograd, rel L2 (second, first argument):", e_sr, e_hr)
    assert e_sr <= 1e-12 and e_hr <= 1e-12


def test_differentiable_module_constructs():
    from climsr_amd.losses.perceptual import PerceptualLoss

    m = PerceptualLoss(differentiable=True)
    assert m.differentiable is True and m.retain_saved is False and m.saved is None
    assert all(not p.requires_grad for p in m.parameters())  # VGG weights get no gradient
    assert PerceptualLoss(differentiable=True, retain_saved=True).retain_saved is True


def test_task_switch_builds_the_criterion_and_stores_the_hparam():
    from climsr_amd.task.pl_gan import GANLightningModule

    m = GANLightningModule(generator=dict(ESRGAN_CFG), discriminator=dict(RFB_D), differentiable_perceptual_loss=True)
    assert m.hparams.differentiable_perceptual_loss is True
    assert m.perceptual_criterion.differentiable is True and m.perceptual_criterion.retain_saved is False


def test_defaults_build_todays_objects():
    from climsr_amd.losses.perceptual import PerceptualLoss
    from climsr_amd.task.pl_gan import GANLightningModule

    assert PerceptualLoss().differentiable is False and PerceptualLoss().fuse_pool is True
    m = GANLightningModule(generator=dict(ESRGAN_CFG), discriminator=dict(RFB_D))
    assert m.hparams.differentiable_perceptual_loss is False and m.perceptual_criterion.differentiable is False
    assert (m.hparams.pixel_level_loss_factor, m.hparams.perceptual_loss_factor, m.hparams.adversarial_loss_factor) == (0.01, 1.0, 0.005)


# The 16 data gradients of the backward at 256^2, conv5_4 first, as PerceptualLoss.backward_input calls them
# (DESIGN.md 3.16).  Every kernel applies the ReLU mask it is handed: the generic and LDS-DMA kernels' EP 4, the
# 64 -> 64 kernel's EP 2; EP 8 (plain bf16) and conv_n16's EP 0 (fp32 out) are the calls made without a mask.
GENERIC_512, GENERIC_512_PLAIN = "conv_fwd_kernel<4, 4, false, 4, 6, 9, 4, 1>", "conv_fwd_kernel<4, 4, false, 4, 6, 9, 8, 1>"
DMA_MASK, DMA_PLAIN = "conv_fwd_dma_kernel<4, false>", "conv_fwd_dma_kernel<8, false>"
BACKWARD_ROUTES = [
    (512, 512, 16, True, GENERIC_512), (512, 512, 16, True, GENERIC_512), (512, 512, 16, True, GENERIC_512),
    (512, 512, 16, False, GENERIC_512_PLAIN),                                                       # conv5_1 into pool 4
    (512, 512, 32, True, DMA_MASK), (512, 512, 32, True, DMA_MASK), (512, 512, 32, True, DMA_MASK),
    (256, 512, 32, False, DMA_PLAIN),                                                               # conv4_1 into pool 3
    (256, 256, 64, True, DMA_MASK), (256, 256, 64, True, DMA_MASK), (256, 256, 64, True, DMA_MASK),
    (128, 256, 64, False, DMA_PLAIN),                                                               # conv3_1 into pool 2
    (128, 128, 128, True, DMA_MASK),
    (64, 128, 128, False, DMA_PLAIN),                                                               # conv2_1 into pool 1
    (64, 64, 256, True, "conv_wr_kernel<2>"),
    (3, 64, 256, False, "conv_n16_kernel<2, 0>"),                                                   # conv1_1, fp32 out
]


@pytest.mark.parametrize("n", [32, 64])
def test_backward_routes_at_the_gan_step_shape(n, monkeypatch):
    """Asked of the dispatch through ConvPlan.dgrad with a recording launch observer, as tests/test_dispatch_routes.py
    does: nothing is launched.  A route without the mask epilogue would show here as a name without EP 4 / EP 2."""
    from climsr_amd import _lib, ops
    from climsr_amd.ops import ACT_RELU_BWD, ConvPlan

    _lib.load()
    names = []
    monkeypatch.setattr(ops, "PROFILER", lambda name, flops, fn, tag="", nbytes=0: names.append(name))
    monkeypatch.setattr(_lib, "stream_ptr", lambda: 0)
    bf, f32 = torch.empty(8, dtype=torch.bfloat16), torch.empty(8)
    for cin, cout, hw, mask, want in BACKWARD_ROUTES:
        p = ConvPlan(cin, cout, 3, 1, 1, "route")
        p.weight, p.bias, p.wpk_t = torch.zeros(1), torch.zeros(cout), bf
        if cin == 3:
            p.dgrad(bf, cout, hw, hw, f32, 4, 0, n)
        elif mask:
            p.dgrad(bf, cout, hw, hw, bf, cin, 0, n, act=ACT_RELU_BWD, res1=bf, res1_cs=cin, res1_co=0)
        else:
            p.dgrad(bf, cout, hw, hw, bf, cin, 0, n)
        assert names[-1] == want, (cin, cout, hw, names[-1])
    assert len(names) == 16


@pytest.mark.parametrize("differentiable", [False, True])
def test_cpu_tensors_are_refused(differentiable):
    from climsr_amd.losses.perceptual import PerceptualLoss

    x = torch.zeros((1, 1, 16, 16), requires_grad=differentiable)
    with pytest.raises(RuntimeError, match="runs on the GPU only"):
        PerceptualLoss(differentiable=differentiable)(x, torch.zeros((1, 1, 16, 16)))
