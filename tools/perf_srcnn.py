"""Training-step time of the stand-alone SRCNN task (generator_type "srcnn", MSE) and its per-launch split.

The reference's config: B=128, HR 128x128, in_channels 3, AdamW + OneCycleLR through the built-in Trainer, bf16 compute.
Two passes over the same synthetic batch ("Stand-alone SRCNN"):
  1. whole steps, profiler off: warm-up, then HIP-event times of --steps steps, median / min / max;
  2. per launch, ops.PROFILER wrapping every launch in its own pair of events (this serialises the host, so the sum is
     not the step time): median per launch name over the same number of steps.
Also runs one no-grad forward of a whole 1440x2880 grid.  Prints one JSON line.

    python tools/perf_srcnn.py [--batch 128] [--hr 128] [--steps 50] [--warmup 10]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--hr", type=int, default=128)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_srcnn: no GPU (a timing needs the MI355X)")
    from climsr_amd import ops
    from climsr_amd.core.trainer import Trainer
    from climsr_amd.task.pl_generator_pre_training import SuperResolutionLightningModule

    dev = "cuda"
    torch.manual_seed(0)
    m = SuperResolutionLightningModule(
        generator={"_target_": "climsr_amd.models.srcnn.SRCNN", "in_channels": 3}, generator_type="srcnn",
        optimizers={"generator_optimizer": {"_target_": "torch.optim.AdamW", "lr": 1e-4, "weight_decay": 1e-4}},
        schedulers={"generator_scheduler": {"_target_": "torch.optim.lr_scheduler.OneCycleLR", "max_lr": 1e-4,
                                            "num_training_steps": -1, "epochs": 1, "pct_start": 0.05, "div_factor": 2,
                                            "final_div_factor": 100}}).to(dev)
    total = a.warmup * 2 + a.steps * 2 + 2
    tr = Trainer(m, num_training_steps=total)
    g = torch.Generator().manual_seed(42)
    shape = (a.batch, 1, a.hr, a.hr)
    hr = torch.rand(shape, generator=g) * 2 - 1
    elev = torch.rand(shape, generator=g) * 2 - 1
    mask = (torch.rand(shape, generator=g) < 0.7).float()
    up = hr[:, :, ::4, ::4].repeat_interleave(4, dim=-2).repeat_interleave(4, dim=-1)
    batch = {k: v.to(dev) for k, v in {"lr": torch.cat([up, elev, mask], 1).contiguous(), "hr": hr, "elevation": elev,
                                       "mask": mask}.items()}
    for i in range(a.warmup):
        tr.training_batch(batch, i)
    torch.cuda.synchronize()
    times = []
    for i in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = tr.training_batch(batch, i)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    loss = float(out[0].detach())
    per = {}

    def prof(name, flops, fn, tag="", nbytes=0):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        per.setdefault(name, []).append((e0, e1, nbytes))

    ops.PROFILER = prof
    try:
        for i in range(a.warmup + a.steps):
            if i == a.warmup:
                torch.cuda.synchronize()
                per.clear()
            tr.training_batch(batch, i)
        torch.cuda.synchronize()
    finally:
        ops.PROFILER = None
    launches = {}
    for name, evs in per.items():
        ms = [e0.elapsed_time(e1) for e0, e1, _b in evs]
        launches[name] = {"per_step": len(evs) / a.steps, "median_ms": round(statistics.median(ms), 4),
                          "algorithmic_MB": round(evs[0][2] / 1e6, 2)}
    grid = torch.rand((1, 3, 1440, 2880), generator=g).to(dev)
    with torch.no_grad():
        m(grid)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sr = m(grid)
        e1.record()
        e1.synchronize()
    assert sr.shape == (1, 1, 1440, 2880) and bool(torch.isfinite(sr).all())
    print(json.dumps({"config": {"batch": a.batch, "hr": a.hr, "in_channels": 3, "steps": a.steps, "warmup": a.warmup},
                      "device": torch.cuda.get_device_name(0), "loss": loss,
                      "step_ms": {"median": round(statistics.median(times), 4), "min": round(min(times), 4),
                                  "max": round(max(times), 4)},
                      "launches": launches, "whole_grid_1440x2880_forward_ms": round(e0.elapsed_time(e1), 4)}))


if __name__ == "__main__":
    main()
