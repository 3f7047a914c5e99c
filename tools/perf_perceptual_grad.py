"""What ``differentiable_perceptual_loss=True`` costs: the full GAN step at config 3 (ESRGAN nb 11 + RFB discriminator,
batch 32, 64 -> 256) with the option off and on, the two alternating step by step in one process on one GPU
(``Trainer(graph_steps=True)``, HIP events, --warmup steps first, then the median of --steps), and the per-kernel times
of one backward of the perceptual term at that shape from the launch observer (``ops.PROFILER``: HIP events around
each launch, so short kernels include their dispatch gap).  DESIGN.md, "Perceptual loss with a backward", holds the
numbers.  Prints one JSON line for the steps and one for the kernels.  Not a test.

    python tools/perf_perceptual_grad.py [--steps 50] [--warmup 10] [--batch 32] [--hr 256] [--nb 11]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

ADAMW = {"_target_": "torch.optim.AdamW", "lr": 1e-4, "weight_decay": 1e-4}
ONE_CYCLE = {"_target_": "torch.optim.lr_scheduler.OneCycleLR", "max_lr": 1e-4, "num_training_steps": -1, "pct_start": 0.05,
             "div_factor": 2, "final_div_factor": 100}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def make_task(option, nb):
    from climsr_amd.task.pl_gan import GANLightningModule

    gcfg = {"_target_": "climsr_amd.models.esrgan.ESRGANGenerator", "in_channels": 3, "out_channels": 1, "nf": 64, "nb": nb, "gc": 16,
            "scale_factor": 4}
    return GANLightningModule(
        generator=gcfg, discriminator={"_target_": "climsr_amd.models.rfb_esrgan.RFBESRGANDiscriminator", "in_channels": 1},
        optimizers={"generator_optimizer": dict(ADAMW), "discriminator_optimizer": dict(ADAMW)},
        schedulers={"generator_scheduler": dict(ONE_CYCLE), "discriminator_scheduler": dict(ONE_CYCLE)},
        differentiable_perceptual_loss=option)


def step_times(a, dev):
    from climsr_amd.core.trainer import Trainer
    from oracle import climsr_ref as ref

    batches = [{k: v.to(dev) for k, v in ref.synthetic_batch(a.batch, a.hr, seed=40 + i).items()} for i in range(4)]
    total = a.warmup + a.steps + 8
    sides = {}
    for name, option in (("off", False), ("on", True)):
        torch.manual_seed(0)
        sides[name] = [Trainer(make_task(option, a.nb).to(dev), num_training_steps=total, graph_steps=True), 0]

    def step(name):
        tr, i = sides[name]
        tr.training_batch(batches[i % len(batches)], i)
        sides[name][1] = i + 1

    for _ in range(max(a.warmup, 3)):  # graph mode: two eager steps, then the capture and its first replay
        for name in sides:
            step(name)
    torch.cuda.synchronize()
    ms = {name: [] for name in sides}
    for _ in range(a.steps):
        for name in ms:
            ms[name].append(timed(lambda: step(name)))
    out = {"off_step_ms": stats(ms["off"]), "on_step_ms": stats(ms["on"]),
           "added_ms": round(statistics.median(ms["on"]) - statistics.median(ms["off"]), 3),
           "graph_stats": {name: dict(s[0].graph_stats) for name, s in sides.items()},
           "peak_memory_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    del sides, batches
    torch.cuda.empty_cache()
    return out


def backward_kernels(a, dev):
    """One eager forward + backward of the term alone at (batch, hr): every launch of the backward under HIP events."""
    from climsr_amd import ops
    from climsr_amd.losses.perceptual import PerceptualLoss

    g = torch.Generator().manual_seed(1)
    hr = (torch.rand((a.batch, 1, a.hr, a.hr), generator=g) * 2 - 1).to(dev)
    sr = (hr + 0.2 * torch.randn(hr.shape, generator=g).to(dev)).requires_grad_(True)
    crit = PerceptualLoss(differentiable=True).to(dev)
    rec = []

    def observer(name, flops, fn, tag="", nbytes=0):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        rec.append((tag, name, flops, nbytes, s, e))

    # the forward alone, eager: the default module (one fused 2n batch, nothing kept) beside the differentiable one
    # (a fused constant half and a grad half that stores its 16 un-pooled maps)
    fwd = {}
    for name, m, x in (("default", PerceptualLoss().to(dev), sr.detach()), ("differentiable", crit, sr)):
        ms = []
        for _ in range(7):
            ms.append(timed(lambda: m(hr, x)))
        fwd[name + "_forward_ms"] = round(statistics.median(ms[2:]), 3)
    rows = {}
    for rep in range(3):  # the last repetition is reported (the first pays the kernels' one-time set-up)
        sr.grad = None
        loss = crit(hr, sr)
        torch.cuda.synchronize()
        rec.clear()
        ops.PROFILER = observer
        try:
            t = timed(loss.backward)
        finally:
            ops.PROFILER = None
        torch.cuda.synchronize()
        rows = dict(fwd, backward_ms=round(t, 3), launches=[])
        for tag, name, flops, nbytes, s, e in rec:
            us = s.elapsed_time(e) * 1e3
            rows["launches"].append({"what": tag, "kernel": name, "us": round(us, 1), "tflops": round(flops / us / 1e6, 1) if flops else None,
                                     "gb_s": round(nbytes / us / 1e3, 1) if nbytes else None})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hr", type=int, default=256)
    ap.add_argument("--nb", type=int, default=11)
    ap.add_argument("--skip-steps", action="store_true", help="only the per-kernel times of the backward")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_perceptual_grad: no GPU (a timing needs the MI355X)")
    dev = "cuda"
    cfg = {"net": f"esrgan nb{a.nb} + rfb d + vgg19", "batch": a.batch, "hr": a.hr, "steps": a.steps, "warmup": a.warmup}
    if not a.skip_steps:
        print(json.dumps(dict({"config": cfg, "device": torch.cuda.get_device_name(0)}, **step_times(a, dev))), flush=True)
    print(json.dumps({"config": cfg, "perceptual_backward": backward_kernels(a, dev)}), flush=True)


if __name__ == "__main__":
    main()
