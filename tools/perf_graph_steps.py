"""Time of one training step of the built-in Trainer, eager (``graph_steps=False``: every launch issued from Python, the
schedule on the host) beside graph mode (``graph_steps=True``: device-stepped optimizers, the step replayed as one
hipGraph), on one GPU, in one process, the two alternating step by step ("Captured training steps").

Workloads: RCAN 10x20 x4, 32 -> 128 at batch 32 and 96 (AdamW + OneCycleLR); the GAN step at the bench shape (ESRGAN
nb 11 + RFB discriminator, batch 32, 64 -> 256); the stand-alone SRCNN at batch 192, HR 128 (Adam + cosine warm-up).
Warm-up steps first (they include graph mode's eager steps and its capture), then HIP-event times of --steps steps
each; every step gets one of four different batches.  Prints one JSON line per workload.  Not a test.

    python tools/perf_graph_steps.py [--workloads rcan32,rcan96,gan,srcnn] [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

ADAMW = {"_target_": "torch.optim.AdamW", "lr": 1e-4, "weight_decay": 1e-4}
ADAM = {"_target_": "torch.optim.Adam", "lr": 1e-3, "weight_decay": 1e-4}
ONE_CYCLE = {"_target_": "torch.optim.lr_scheduler.OneCycleLR", "max_lr": 1e-4, "num_training_steps": -1, "pct_start": 0.05,
             "div_factor": 2, "final_div_factor": 100}
COSINE = {"_target_": "transformers.get_cosine_schedule_with_warmup", "num_training_steps": -1, "num_warmup_steps": 0.1}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def build(workload, dev):
    """(make_task, make_batch(seed), description) of one workload."""
    from climsr_amd.task.pl_gan import GANLightningModule
    from climsr_amd.task.pl_generator_pre_training import SuperResolutionLightningModule
    from oracle import climsr_ref as ref

    def to_dev(bt):
        return {k: v.to(dev) for k, v in bt.items()}

    if workload.startswith("rcan"):
        b = int(workload[4:])
        cfg = {"_target_": "climsr_amd.models.rcan.TrainableRCAN", "n_resgroups": 10, "n_resblocks": 20, "n_feats": 64,
               "reduction": 16, "scaling_factor": 4, "in_channels": 3, "out_channels": 1}
        task = lambda: SuperResolutionLightningModule(  # noqa: E731
            generator=dict(cfg), generator_type="rcan", optimizers={"generator_optimizer": dict(ADAMW)},
            schedulers={"generator_scheduler": dict(ONE_CYCLE)})
        return task, (lambda s: to_dev(ref.synthetic_batch(b, 128, seed=s, scale=4))), {"net": "rcan 10x20 x4", "batch": b, "hr": 128}
    if workload == "srcnn":
        def srcnn_batch(s):
            bt = ref.synthetic_batch(192, 128, seed=s)
            up = bt["lr"][:, :1].repeat_interleave(4, dim=-2).repeat_interleave(4, dim=-1)
            bt["lr"] = torch.cat([up, bt["elevation"], bt["mask"]], 1).contiguous()
            return to_dev(bt)

        task = lambda: SuperResolutionLightningModule(  # noqa: E731
            generator={"_target_": "climsr_amd.models.srcnn.SRCNN", "in_channels": 3}, generator_type="srcnn",
            optimizers={"generator_optimizer": dict(ADAM)}, schedulers={"generator_scheduler": dict(COSINE)})
        return task, srcnn_batch, {"net": "srcnn", "batch": 192, "hr": 128}
    if workload == "gan":
        gcfg = {"_target_": "climsr_amd.models.esrgan.ESRGANGenerator", "in_channels": 3, "out_channels": 1, "nf": 64, "nb": 11,
                "gc": 16, "scale_factor": 4}
        task = lambda: GANLightningModule(  # noqa: E731
            generator=dict(gcfg), discriminator={"_target_": "climsr_amd.models.rfb_esrgan.RFBESRGANDiscriminator", "in_channels": 1},
            optimizers={"generator_optimizer": dict(ADAMW), "discriminator_optimizer": dict(ADAMW)},
            schedulers={"generator_scheduler": dict(ONE_CYCLE), "discriminator_scheduler": dict(ONE_CYCLE)})
        return task, (lambda s: to_dev(ref.synthetic_batch(32, 256, seed=s))), {"net": "esrgan nb11 + rfb d", "batch": 32, "hr": 256}
    raise SystemExit(f"perf_graph_steps: unknown workload {workload!r}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="rcan32,rcan96,gan,srcnn")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_graph_steps: no GPU (a timing needs the MI355X)")
    from climsr_amd.core.trainer import Trainer

    dev = "cuda"
    total = a.warmup + a.steps + 8
    for workload in a.workloads.split(","):
        make_task, make_batch, cfg = build(workload, dev)
        batches = [make_batch(40 + i) for i in range(4)]
        sides = {}
        for name, kw in (("eager", {}), ("graph", {"graph_steps": True})):
            torch.manual_seed(0)
            tr = Trainer(make_task().to(dev), num_training_steps=total, **kw)
            sides[name] = [tr, 0]

        def step(name):
            tr, i = sides[name]
            tr.training_batch(batches[i % len(batches)], i)
            sides[name][1] = i + 1

        for _ in range(max(a.warmup, 3)):  # graph mode: two eager steps, then the capture and its first replay
            step("eager")
            step("graph")
        torch.cuda.synchronize()
        ms = {"eager": [], "graph": []}
        for _ in range(a.steps):
            for name in ms:
                ms[name].append(timed(lambda: step(name)))
        g = sides["graph"][0]
        print(json.dumps({"config": dict(cfg, steps=a.steps, warmup=a.warmup), "device": torch.cuda.get_device_name(0),
                          "eager_step_ms": stats(ms["eager"]), "graph_step_ms": stats(ms["graph"]), "graph_stats": g.graph_stats,
                          "graph_over_eager": round(statistics.median(ms["graph"]) / statistics.median(ms["eager"]), 3)}), flush=True)
        del sides, g, tr, batches
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
