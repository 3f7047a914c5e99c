"""The stand-alone SRCNN through the task API (``generator_type: "srcnn"``, reference task.py:141,235-239): training
through the built-in Trainer against the reference's own float64 steps (tests/golden/srcnn_steps.npz,
make_srcnn_golden.py), the tile pipeline's "srcnn" batch, validation, checkpoints and whole-grid inference.

The training comparison fixes no number in advance: loss, first-step gradients and the three-step parameter update must
lie within 2x the spread of the oracle's own torch-autocast fp16 / bf16 runs of the same three steps
(helpers.update_envelope, its default floor; the biases pooled as in test_gpu_configs.py) -- the reference trains with
precision 16."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import climsr_ref as ref
from tests.helpers import gemm_conv, update_envelope

pytestmark = pytest.mark.gpu
DEV = "cuda"
ADAMW_YAML = {"_target_": "torch.optim.AdamW", "lr": 1e-4, "weight_decay": 1e-4}
ONE_CYCLE_YAML = {"_target_": "torch.optim.lr_scheduler.OneCycleLR", "max_lr": 1e-4, "num_training_steps": -1, "epochs": 1,
                  "pct_start": 0.05, "div_factor": 2, "final_div_factor": 100}
SRCNN_CFG = {"_target_": "climsr_amd.models.srcnn.SRCNN", "in_channels": 3}
POOL_BELOW = 256  # the biases (1 - 64 elements) are compared pooled (helpers.pool_small)
KEYS = [f"conv{k}.{t}" for k in (1, 2, 3) for t in ("weight", "bias")]


def srcnn_batch(b, hr, seed, dtype=torch.float32):
    """ref.synthetic_batch with ``lr`` as the tile pipeline's "srcnn" mode builds it: the LR tile upscaled back to HR
    size with nearest neighbour, then elevation and mask."""
    bt = ref.synthetic_batch(b, hr, seed=seed, dtype=dtype)
    up = bt["lr"][:, :1].repeat_interleave(4, dim=-2).repeat_interleave(4, dim=-1)
    bt["lr"] = torch.cat([up, bt["elevation"], bt["mask"]], 1).contiguous()
    return bt


def make_task(**kw):
    from climsr_amd.task.pl_generator_pre_training import SuperResolutionLightningModule

    torch.manual_seed(0)  # nn.Conv2d's default initialisation
    return SuperResolutionLightningModule(generator=dict(SRCNN_CFG), generator_type="srcnn",
                                          optimizers={"generator_optimizer": dict(ADAMW_YAML)},
                                          schedulers={"generator_scheduler": dict(ONE_CYCLE_YAML)}, **kw)


def oracle_amp_steps(init, batches, total_steps, dtype, scale):
    """The oracle's three steps under torch autocast ``dtype`` (fp32 master weights and MSE loss, the loss scaled as
    precision=16's GradScaler scales it), on the GPU: per-step losses, first-step gradients, the parameter update."""
    q = {"srcnn." + k: v.to(DEV, torch.float32).clone() for k, v in init.items()}
    keys = list(q)
    opt = ref.AdamWState(q, keys, lr=1e-4, total_steps=total_steps)
    losses, grads0 = [], None
    for i, bt in enumerate(batches):
        b_ = {k: v.to(DEV, torch.float32) for k, v in bt.items()}
        for k in keys:
            q[k].requires_grad_(True)
        with torch.autocast("cuda", dtype=dtype):
            sr = ref.srcnn_forward(q, b_["lr"])
        loss = ((sr.float() - b_["hr"]) ** 2).mean()
        gs = torch.autograd.grad(loss * scale, [q[k] for k in keys])
        grads = {k: g / scale for k, g in zip(keys, gs)}
        assert all(torch.isfinite(g).all() for g in grads.values()), "loss scale overflowed"
        for k in keys:
            q[k].requires_grad_(False)
        if i == 0:
            grads0 = {k[6:]: g.double().cpu() for k, g in grads.items()}
        losses.append(float(loss))
        opt.step(q, grads)
        opt.sched()
    upd = {k[6:]: q[k].double().cpu() - init[k[6:]].double() for k in keys}
    return torch.tensor(losses, dtype=torch.float64), grads0, upd


def test_srcnn_trainer_steps_vs_reference_golden(golden_dir, monkeypatch):
    from climsr_amd.core.optim import AdamW
    from climsr_amd.core.trainer import Trainer

    z = np.load(os.path.join(golden_dir, "srcnn_steps.npz"))
    meta = json.loads(str(z["meta"]))
    b, hr, total = meta["batch"], meta["hr_size"], meta["total_steps"]
    init = {k: torch.from_numpy(z[f"init.{k}"]) for k in KEYS}
    m = make_task()
    m.generator.load_state_dict({k: v.float() for k, v in init.items()})
    m = m.to(DEV)
    tr = Trainer(m, limit_train_batches=total, max_epochs=1)
    assert type(tr.optimizers[0]) is AdamW and tr.optimizers[0].owner is m.generator  # the fused flat-buffer update
    assert tr.schedulers[0]["scheduler"].total_steps == total
    assert type(m.loss).__name__ == "MSELoss"
    batches = [srcnn_batch(b, hr, s) for s in meta["seeds"]]
    losses, lrs, grads0 = [], [], None
    for i, bt in enumerate(batches):
        lrs.append(tr.optimizers[0].param_groups[0]["lr"])
        out = tr.training_batch({k: v.to(DEV) for k, v in bt.items()}, i)
        losses.append(float(out[0].detach()))
        if i == 0:
            grads0 = {k: p.grad.double().cpu().clone() for k, p in m.generator.named_parameters()}
    torch.cuda.synchronize()
    assert np.allclose(lrs, z["lr"], rtol=1e-9, atol=0), (lrs, z["lr"])
    assert "train/loss" in m.logged
    upd = {k: p.detach().double().cpu() - init[k] for k, p in m.generator.named_parameters()}
    want_upd = {k: torch.from_numpy(z[f"final.{k}"]) - init[k] for k in KEYS}
    want_g0 = {k: torch.from_numpy(z[f"grads0.{k}"]) for k in KEYS}
    with monkeypatch.context() as mp:
        mp.setattr(ref, "_conv", gemm_conv)  # rocBLAS GEMMs on the GPU (no MIOpen per-shape compiles)
        torch.backends.cuda.matmul.allow_tf32 = False
        amps = [oracle_amp_steps(init, batches, total, dt, sc) for dt, sc in ((torch.float16, 2.0 ** 16), (torch.bfloat16, 1.0))]
    print("srcnn losses", losses, "reference fp64", z["loss"].tolist(), "autocast", [a[0].tolist() for a in amps])
    failures = []
    for what, got, want, amp, pool in (
            ("loss", {"loss": torch.tensor(losses, dtype=torch.float64)}, {"loss": torch.from_numpy(z["loss"])},
             [{"loss": a[0]} for a in amps], 0),
            ("first-step gradients", grads0, want_g0, [a[1] for a in amps], POOL_BELOW),
            ("3-step update", upd, want_upd, [a[2] for a in amps], POOL_BELOW)):
        bad, worst, rows = update_envelope(got, want, amp, pool_below=pool)
        for k, (r, ra) in rows.items():
            print(f"srcnn {what} {k}: rel L2 vs fp64 {r:.3e}, autocast spread {ra:.3e}, native / (2 x spread) {r / (2 * ra):.3f}",
                  flush=True)
        if bad:
            failures.append((what, bad))
    assert not failures, failures


def _raw_tiles(n, h, w, seed):
    rs = np.random.RandomState(seed)
    raw = (rs.rand(n, h, w).astype(np.float32) * 30 - 5)
    raw[:, :6, :] = np.nan
    elev = (rs.rand(n, h, w) * 1000).astype(np.float32)
    return torch.from_numpy(raw).to(DEV), torch.from_numpy(elev).to(DEV)


def test_training_step_on_tile_pipeline_batch():
    from climsr_amd.core.trainer import Trainer
    from climsr_amd.data import DeviceTilePipeline
    from climsr_amd.losses.mse import mse_loss

    m = make_task().to(DEV)
    raw, elev = _raw_tiles(2, 64, 64, seed=31)
    batch = DeviceTilePipeline(generator_type="srcnn", stage="train", seed=5)(raw, elev, [-6.0, -6.0], [26.0, 26.0])
    assert batch["lr"].shape == (2, 3, 64, 64) and batch["hr"].shape == (2, 1, 64, 64)
    with torch.no_grad():
        want = mse_loss(m(batch["lr"], batch["elevation"], batch["mask"]), batch["hr"])
    before = m.generator._flat.clone()
    tr = Trainer(m, num_training_steps=10)
    out = tr.training_batch(batch, 0)
    torch.cuda.synchronize()
    assert torch.isfinite(out[0]).item() and torch.equal(out[0].detach(), want)
    assert not torch.equal(m.generator._flat, before)  # the step moved the weights ...
    with torch.no_grad():  # ... and the kernels see the moved weights (bf16 layouts repacked)
        assert not torch.equal(mse_loss(m(batch["lr"]), batch["hr"]), want)


def test_validation_step_metric_keys():
    from climsr_amd.data import DeviceTilePipeline

    m = make_task(normalization_method="minmax", normalization_range=(-1.0, 1.0)).to(DEV)
    raw, elev = _raw_tiles(2, 64, 64, seed=32)
    batch = DeviceTilePipeline(generator_type="srcnn", stage="val")(raw, elev, [-6.0, -6.0], [26.0, 26.0])
    with torch.no_grad():
        out = m.validation_step(batch, 0)
    for k in ("val/rmse", "val/psnr", "val/ssim", "val/acc@01.25", "val/r2", "val/loss", "val/normalized_loss"):
        assert k in out and torch.isfinite(out[k]).item(), k
    m.validation_epoch_end([out])
    assert abs(m.logged["hp_metric"].item() - out["val/rmse"].item()) < 1e-12


def test_checkpoint_round_trip_is_bit_identical(tmp_path):
    from climsr_amd.core.trainer import Trainer
    from climsr_amd.task.pl_generator_pre_training import SuperResolutionLightningModule

    m = make_task().to(DEV)
    tr = Trainer(m, num_training_steps=10)
    bt = {k: v.to(DEV) for k, v in srcnn_batch(2, 48, 41).items()}
    tr.training_batch(bt, 0)  # off the initial weights, optimizer state present
    path = str(tmp_path / "srcnn.ckpt")
    m.save_checkpoint(path, epoch=0, global_step=1, optimizers=tr.optimizers, schedulers=tr.schedulers)
    fresh = SuperResolutionLightningModule.load_from_checkpoint(path, strict=True).to(DEV)
    assert fresh._loaded_checkpoint_keys == ([], []) and type(fresh.loss).__name__ == "MSELoss"
    assert fresh.hparams.generator_type == "srcnn" and type(fresh.generator).__name__ == "SRCNN"
    with torch.no_grad():
        a = m(bt["lr"], bt["elevation"], bt["mask"])
        b = fresh(bt["lr"], bt["elevation"], bt["mask"])
    torch.cuda.synchronize()
    assert torch.equal(m.generator._flat, fresh.generator._flat) and torch.equal(a, b)


def test_whole_grid_inference_writes_denormalized_forward(tmp_path):
    from climsr_amd.inference import denormalize_mask, inference_on_full_images, npy_writer

    m = make_task().to(DEV)
    g = torch.Generator().manual_seed(51)
    h, w = 64, 96
    lr = (torch.rand((1, 3, h, w), generator=g) * 2 - 1).to(DEV)
    mask = (torch.rand((1, 1, h, w), generator=g) < 0.7).float().to(DEV)
    lr[:, 2:] = mask
    batch = {"lr": lr, "elevation": lr[:, 1:2].contiguous(), "mask": mask, "min": np.array([-7.25]), "max": np.array([31.0]),
             "filename": "grid.tif"}
    paths = inference_on_full_images(m, [batch], str(tmp_path), writer=npy_writer)
    with torch.no_grad():
        want = denormalize_mask(m(lr, batch["elevation"], mask), mask, batch["min"], batch["max"]).cpu().numpy()[0, 0]
    got = np.load(paths[0])
    assert len(paths) == 1 and got.shape == (h, w) and got.dtype == np.float32
    assert np.array_equal(np.isnan(got), mask.cpu().numpy()[0, 0] == 0)
    assert np.array_equal(np.nan_to_num(got).view(np.uint32), np.nan_to_num(want).view(np.uint32))
