"""The built-in Trainer's Lightning options on the GPU (core/trainer.py): gradient accumulation, gradient clipping
through the fused AdamW, grad-norm tracking, terminate_on_nan, and that the defaults launch nothing new.  The
stand-alone SRCNN task (the recipe of tests/test_gpu_srcnn_task.py, restated) at B=2, HR 32; one GAN case on the nb=1
ESRGAN + RFB discriminator of tests/test_gpu_gan.py.

Clipping is checked on Adam's first moment, not on the parameters: Adam's update is nearly invariant to the gradient's
scale, so a missing clip would not show in the weights."""
import numpy as np
import pytest
import torch

from oracle import climsr_ref as ref
from tests.helpers import gen_params, rfb_d_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
ADAMW_YAML = {"_target_": "torch.optim.AdamW", "lr": 1e-4, "weight_decay": 1e-4}
ONE_CYCLE_YAML = {"_target_": "torch.optim.lr_scheduler.OneCycleLR", "max_lr": 1e-4, "num_training_steps": -1, "epochs": 1,
                  "pct_start": 0.05, "div_factor": 2, "final_div_factor": 100}
SRCNN_CFG = {"_target_": "climsr_amd.models.srcnn.SRCNN", "in_channels": 3}
B, HR = 2, 32


def srcnn_batch(b, hr, seed):
    bt = ref.synthetic_batch(b, hr, seed=seed)
    up = bt["lr"][:, :1].repeat_interleave(4, dim=-2).repeat_interleave(4, dim=-1)
    bt["lr"] = torch.cat([up, bt["elevation"], bt["mask"]], 1).contiguous()
    return {k: v.to(DEV) for k, v in bt.items()}


def make_task(**kw):
    from climsr_amd.task.pl_generator_pre_training import SuperResolutionLightningModule

    torch.manual_seed(0)  # nn.Conv2d's default initialisation: every task made here starts from the same weights
    return SuperResolutionLightningModule(generator=dict(SRCNN_CFG), generator_type="srcnn",
                                          optimizers={"generator_optimizer": dict(ADAMW_YAML)},
                                          schedulers={"generator_scheduler": dict(ONE_CYCLE_YAML)}, **kw).to(DEV)


@pytest.fixture(scope="module")
def batches():
    return [srcnn_batch(B, HR, 60 + s) for s in range(4)]


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def one_minus(b1):
    """The kernel's ``1.f - b1`` on the float32 the optimizer hands it."""
    return torch.tensor(1.0, dtype=torch.float32, device=DEV) - torch.tensor(b1, dtype=torch.float32, device=DEV)


def beta1(tr):
    return tr.optimizers[0].param_groups[0]["betas"][0]


def moments(tr):
    return tr.optimizers[0].state["group0"]["m"]


def ulp_close(got, want):
    got, want = np.float32(got), np.float32(want)
    return abs(got - want) <= np.spacing(want)


@pytest.fixture(scope="module")
def default_first_step(batches):
    """A default trainer's first step on batch 0: its gradient, the gradient's fp64 norm N0, beta1 and Adam's first
    moment.  Shared (read only) by the clipping tests."""
    from climsr_amd.core.trainer import Trainer

    m = make_task()
    tr = Trainer(m, num_training_steps=10)
    b1 = beta1(tr)
    tr.training_batch(batches[0], 0)
    torch.cuda.synchronize()
    g = m.generator._flat_grad.clone()
    return dict(task=m, trainer=tr, g=g, n0=float(g.double().norm()), b1=b1, m=moments(tr).clone())


# ------------------------------------------------------------------------------------------ accumulation
def test_accumulation_steps_the_scheduler_it_sized(batches):
    """20 batches at accumulate_grad_batches=2: OneCycleLR is built for 10 steps and must be stepped 10 times (a
    trainer that steps on every batch over-steps it and torch raises halfway through)."""
    from climsr_amd.core.trainer import Trainer

    m = make_task()
    tr = Trainer(m, limit_train_batches=20, max_epochs=1, accumulate_grad_batches=2)
    sched = tr.schedulers[0]["scheduler"]
    assert sched.total_steps == 10
    outs = tr.fit(batches[i % len(batches)] for i in range(20))
    torch.cuda.synchronize()
    assert len(outs) == 20
    assert tr.optimizers[0].state["group0"]["step"] == 10 and sched.last_epoch == 10
    assert torch.isfinite(m.generator._flat).all()


def test_accumulated_gradient_is_the_mean_of_the_micro_batches(batches):
    from climsr_amd.core.trainer import Trainer

    m = make_task()
    tr = Trainer(m, num_training_steps=10, accumulate_grad_batches=2)
    b1 = beta1(tr)
    tr.training_batch(batches[0], 0)
    assert "group0" not in tr.optimizers[0].state or "m" not in tr.optimizers[0].state["group0"]  # no step yet
    tr.training_batch(batches[1], 1)
    got = moments(tr).double()
    twin = make_task()
    gs = []
    for bt in batches[:2]:  # plain overwrite-mode backward of one micro-batch each
        twin.generator.zero_grad(set_to_none=True)
        twin.training_step(bt, 0).backward()
        gs.append(twin.generator._flat_grad.double().clone())
    torch.cuda.synchronize()
    want = float(one_minus(b1)) * (gs[0] + gs[1]) / 2  # (1 - beta1) as the kernel forms it, then fp64
    for (name, _p), (_q, off, n) in zip(m.generator.named_parameters(), m.generator._flat_index):
        sl = slice(off, off + n)
        diff = float((got[sl] - want[sl]).abs().max())
        # a handful of fp32 roundings (each <= 2^-24 of its operands); 16x for the order split-K partials meet the sum
        bound = 2.0 ** -20 * float((gs[0][sl].abs() + gs[1][sl].abs()).max())
        print(f"accumulated m {name}: max |diff| {diff:.3e}, bound {bound:.3e}")
        assert diff <= bound, (name, diff, bound)
    assert float(want.abs().max()) > 0


def test_open_accumulation_window_steps_on_the_last_batch(batches):
    from climsr_amd.core.trainer import Trainer

    m = make_task()
    tr = Trainer(m, num_training_steps=10, accumulate_grad_batches=2)
    tr.fit(iter(batches[i % len(batches)] for i in range(5)))
    assert tr.optimizers[0].state["group0"]["step"] == 3 and tr.schedulers[0]["scheduler"].last_epoch == 3


# ------------------------------------------------------------------------------------------ clipping
def test_default_first_moment_is_the_unclipped_gradient(default_first_step):
    d = default_first_step  # negative control of the clipping check below
    assert torch.equal(bits(d["m"]), bits(d["g"] * one_minus(d["b1"])))


def test_clipped_first_step(default_first_step, batches):
    from climsr_amd.core.optim import AdamW
    from climsr_amd.core.trainer import Trainer

    n0 = default_first_step["n0"]
    m = make_task()
    tr = Trainer(m, num_training_steps=10, gradient_clip_val=n0 / 2)
    assert type(tr.optimizers[0]) is AdamW
    b1 = beta1(tr)
    tr.training_batch(batches[0], 0)
    torch.cuda.synchronize()
    g = m.generator._flat_grad
    assert torch.equal(bits(g), bits(default_first_step["g"]))  # .grad keeps the unclipped gradient
    assert all(p.grad.data_ptr() == g.data_ptr() + 4 * off for p, off, _n in m.generator._flat_index)
    coef = m.logged["grad_clip_coef/generator"]
    assert coef.dtype == torch.float32 and coef.is_cuda
    norm = float(g.double().norm())
    assert ulp_close(coef.item(), np.float32((n0 / 2) / (norm + 1e-6))), (coef.item(), n0, norm)
    assert 0.49 < coef.item() < 0.51
    assert torch.equal(bits(moments(tr)), bits((g * coef) * one_minus(b1)))
    assert not torch.equal(bits(moments(tr)), bits(default_first_step["m"]))


def test_each_step_logs_its_own_coefficient(default_first_step, batches):
    from climsr_amd.core.trainer import Trainer

    clip = default_first_step["n0"] / 2
    m = make_task()
    tr = Trainer(m, num_training_steps=10, gradient_clip_val=clip)
    for i in range(3):
        tr.training_batch(batches[i], i)
        norm = float(m.generator._flat_grad.double().norm())
        want = np.float32(min(1.0, clip / (norm + 1e-6)))
        assert ulp_close(m.logged["grad_clip_coef/generator"].item(), want), (i, want)


def test_loose_clip_changes_nothing(default_first_step, batches):
    from climsr_amd.core.trainer import Trainer

    runs = []
    for kw in ({}, dict(gradient_clip_val=4 * default_first_step["n0"])):
        m = make_task()
        tr = Trainer(m, num_training_steps=10, **kw)
        for i in range(3):
            tr.training_batch(batches[i], i)
        if kw:
            assert m.logged["grad_clip_coef/generator"].item() == 1.0
        runs.append(m.generator._flat.clone())
    assert torch.equal(bits(runs[0]), bits(runs[1]))


def test_public_clip_grad_norm(default_first_step):
    from climsr_amd.core.optim import GradNorm, clip_grad_norm_

    gen = default_first_step["task"].generator  # its .grad is batch 0's gradient (the step does not touch it)
    g = default_first_step["g"]
    n0 = default_first_step["n0"]
    assert torch.equal(bits(gen._flat_grad), bits(g))
    total = clip_grad_norm_(gen, n0 / 2)
    torch.cuda.synchronize()
    assert total.dim() == 0 and total.is_cuda and abs(total.item() - n0) <= 1e-9 * n0
    coef = GradNorm.of(gen).clip[0]
    assert ulp_close(coef.item(), np.float32((n0 / 2) / (n0 + 1e-6)))
    assert torch.equal(bits(gen._flat_grad), bits(g * coef))
    assert torch.equal(bits(torch.cat([p.grad.reshape(-1) for p in gen.parameters()])), bits(g * coef))
    gen._flat_grad.copy_(g)  # leave the shared fixture as it was


# ------------------------------------------------------------------------------------------ tracking
@pytest.mark.parametrize("track, label", [(2, "2.0"), ("inf", "inf")])
def test_track_grad_norm(batches, monkeypatch, track, label):
    from climsr_amd import ops
    from climsr_amd.core.trainer import Trainer

    m = make_task()
    tr = Trainer(m, num_training_steps=10, track_grad_norm=track)
    labels = []
    monkeypatch.setattr(ops, "PROFILER", lambda name, flops, fn, tag, nbytes: (labels.append(name), fn()))
    tr.training_batch(batches[0], 0)
    monkeypatch.setattr(ops, "PROFILER", None)
    torch.cuda.synchronize()
    assert labels.count("grad_norm") == 1 and "adamw" in labels and "grad_scale" not in labels and "adamw_scaled" not in labels
    prefix = f"grad_{label}_norm/"
    names = [k for k, _p in m.generator.named_parameters()]
    assert sorted(k for k in m.logged if k.startswith("grad_")) == sorted([prefix + "generator." + k for k in names] +
                                                                          [f"grad_{label}_norm_total"])
    for k, p in m.generator.named_parameters():
        got = m.logged[prefix + "generator." + k]
        assert got.is_cuda and got.dtype == torch.float64
        if label == "inf":
            assert got.item() == float(p.grad.abs().max())
        else:
            want = float(p.grad.double().norm())
            assert abs(got.item() - want) <= 1e-9 * want, (k, got.item(), want)
    g = m.generator._flat_grad
    want = float(g.abs().max()) if label == "inf" else float(g.double().norm())
    assert abs(m.logged[f"grad_{label}_norm_total"].item() - want) <= (0.0 if label == "inf" else 1e-9 * want)


def test_clip_and_l2_tracking_share_one_norm_launch(default_first_step, batches, monkeypatch):
    from climsr_amd import ops
    from climsr_amd.core.trainer import Trainer

    m = make_task()
    tr = Trainer(m, num_training_steps=10, track_grad_norm=2.0, gradient_clip_val=default_first_step["n0"] / 2)
    labels = []
    monkeypatch.setattr(ops, "PROFILER", lambda name, flops, fn, tag, nbytes: (labels.append(name), fn()))
    tr.training_batch(batches[0], 0)
    monkeypatch.setattr(ops, "PROFILER", None)
    assert labels.count("grad_norm") == 1 and labels.count("adamw_scaled") == 1
    assert "adamw" not in labels and "grad_scale" not in labels
    assert abs(m.logged["grad_2.0_norm_total"].item() - default_first_step["n0"]) <= 1e-9 * default_first_step["n0"]


# ------------------------------------------------------------------------------------------ terminate_on_nan
def test_terminate_on_nan_stops_before_the_update(batches):
    from climsr_amd.core.trainer import Trainer

    m = make_task()
    tr = Trainer(m, num_training_steps=10, terminate_on_nan=True)
    tr.training_batch(batches[0], 0)  # a clean batch steps as usual
    before = m.generator._flat.clone()
    assert tr.optimizers[0].state["group0"]["step"] == 1
    bad = {k: v.clone() for k, v in batches[1].items()}
    bad["hr"][1, 0, 5, 7] = float("nan")
    with pytest.raises(ValueError, match="batch 1"):
        tr.training_batch(bad, 1)
    torch.cuda.synchronize()
    assert torch.equal(bits(m.generator._flat), bits(before))
    assert tr.optimizers[0].state["group0"]["step"] == 1 and tr.schedulers[0]["scheduler"].last_epoch == 1


# ------------------------------------------------------------------------------------------ defaults
def test_default_trainer_launches_nothing_new(batches, monkeypatch):
    from climsr_amd import ops
    from climsr_amd.core.trainer import Trainer

    m = make_task()
    tr = Trainer(m, num_training_steps=10)
    labels = []
    monkeypatch.setattr(ops, "PROFILER", lambda name, flops, fn, tag, nbytes: (labels.append(name), fn()))
    tr.training_batch(batches[0], 0)
    monkeypatch.setattr(ops, "PROFILER", None)
    assert labels.count("adamw") == 1
    assert not [k for k in labels if k in ("grad_norm", "grad_scale", "adamw_scaled")], labels
    assert not [k for k in m.logged if k.startswith("grad_")]


# ------------------------------------------------------------------------------------------ GAN
def test_gan_accumulate_clip_and_track():
    from climsr_amd.core.optim import flat_grad
    from climsr_amd.core.trainer import Trainer
    from climsr_amd.task.pl_gan import GANLightningModule

    m = GANLightningModule(
        generator={"_target_": "climsr_amd.models.esrgan.ESRGANGenerator", "in_channels": 3, "out_channels": 1, "nf": 64, "nb": 1,
                   "gc": 16, "scale_factor": 4},
        discriminator={"_target_": "climsr_amd.models.rfb_esrgan.RFBESRGANDiscriminator", "in_channels": 1})
    m.generator.load_state_dict(gen_params(1, torch.float32))
    m.discriminator.load_state_dict(rfb_d_params(torch.float32))
    m = m.to(DEV)
    tr = Trainer(m, num_training_steps=10, accumulate_grad_batches=2, gradient_clip_val=1.0, track_grad_norm=2)
    assert tr.schedulers[0]["scheduler"].total_steps == 5
    bts = [{k: v.to(DEV) for k, v in ref.synthetic_batch(2, 128, seed=s).items()} for s in (5, 6)]
    tr.training_batch(bts[0], 0)
    assert not any("group0" in o.state and "m" in o.state["group0"] for o in tr.optimizers)
    tr.training_batch(bts[1], 1)
    torch.cuda.synchronize()
    for o, s in zip(tr.optimizers, tr.schedulers):
        assert o.state["group0"]["step"] == 1 and s["scheduler"].last_epoch == 1
    d = m.discriminator
    assert max(n for _p, _o, n in d._flat_index) > 100_000_000  # fc.0.weight: one segment of 103 M elements
    assert d.bf16_mirror() is not None  # the scaled update took its mirror variant
    want = float(flat_grad(d).double().norm())
    got = m.logged["grad_2.0_norm_total"].item()  # the discriminator stepped last
    print("discriminator total grad norm", got, "torch fp64", want, "coef", m.logged["grad_clip_coef/discriminator"].item())
    assert abs(got - want) <= 1e-9 * want, (got, want)
    assert ulp_close(m.logged["grad_clip_coef/discriminator"].item(), np.float32(min(1.0, 1.0 / (want + 1e-6))))
    names = [k for k, _p in d.named_parameters()]
    assert all(f"grad_2.0_norm/discriminator.{k}" in m.logged for k in names)
    assert all(f"grad_2.0_norm/generator.{k}" in m.logged for k, _p in m.generator.named_parameters())
    assert torch.isfinite(m.generator._flat).all() and torch.isfinite(d._flat).all()


# ------------------------------------------------------------------------------------------ GraphedAdamW
def test_graphed_adamw_max_grad_norm_matches_eager_scaled_step():
    from climsr_amd.core.optim import AdamW, GradNorm, GraphedAdamW

    nets = []
    for _ in range(2):
        nets.append(make_task().generator)
    a, b = nets
    assert torch.equal(a._flat, b._flat)
    g = torch.randn(a._flat.numel(), generator=torch.Generator().manual_seed(9)).to(DEV) * 0.05
    for net in (a, b):
        net._flat_grad.copy_(g)
        net.grads_as_views()
    max_norm = float(g.double().norm()) / 3
    gopt = GraphedAdamW(a, lr=1e-4, total_steps=10, max_grad_norm=max_norm)
    gopt.step()
    hp = gopt.hp.clone()

    class Eager(AdamW):
        def _hparams(self, group, step, device):
            return hp  # the device schedule's scalars, copied

    eopt = Eager(b.parameters(), lr=1e-4, weight_decay=1e-4, owner=b)
    coef = GradNorm.of(b)(2, max_norm)[2]
    eopt.step(grad_scale=coef)
    torch.cuda.synchronize()
    assert 0.3 < coef.item() < 0.35
    st = eopt.state["group0"]
    assert torch.equal(bits(gopt.m), bits(st["m"])) and torch.equal(bits(gopt.v), bits(st["v"]))
    assert torch.equal(bits(a._flat), bits(b._flat))
    assert torch.equal(bits(a._flat_grad), bits(g)) and torch.equal(bits(b._flat_grad), bits(g))
    plain = GraphedAdamW(a, lr=1e-4, total_steps=10)
    assert plain.grad_norm is None and plain.max_grad_norm is None
