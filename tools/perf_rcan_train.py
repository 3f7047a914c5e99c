"""Time of one RCAN L1 pre-training step (forward, backward, fused AdamW) of ``TrainableRCAN``, beside the same step done
by torch: ``oracle.climsr_ref.rcan_forward`` under ``torch.autocast(bf16)`` with torch autograd and ``torch.optim.AdamW``
on the same GPU, in the same process, the two alternating step by step ("RCAN training").

The reference's config (rcan_pre_training.yaml): RCAN 10x20, x4, LR 32x32, batch 96; also batch 32.  Warm-up first, then
HIP-event times of --steps (>= 20) steps each.  The native launch count is taken from one extra step with every C-ABI
entry point wrapped (kernels per call: 2 for the attention forward, 3 for its backward, 1 otherwise, 0 for the sizing /
query helpers); torch's own copies around it (the stream clone, the loss) are not in it.  Prints one JSON line per batch
size (a native-only line first, in case the torch side cannot run).

    python tools/perf_rcan_train.py [--batches 96,32] [--steps 20] [--warmup 5] [--groups 10] [--blocks 20] [--lr 32]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

QUERY = ("_workspace", "_splits", "_kernel", "fwd_bn_parts", "fwd_ch_parts", "_chunk", "_chunk_ex", "_packed_k", "_packed_rows", "_packed_elems", "_kp",
         "last_error", "_version")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def count_launches(fn):
    """Kernel launches libclimsr_hip.so issues while fn() runs, by C-ABI call."""
    from climsr_amd import _lib

    lib = _lib.load()
    calls = {}
    saved = {}

    def wrap(name, f):
        def g(*a):
            calls[name] = calls.get(name, 0) + 1
            return f(*a)
        return g

    for name in _lib.SIGNATURES:
        saved[name] = getattr(lib, name)
        setattr(lib, name, wrap(name, saved[name]))
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        for name, f in saved.items():
            setattr(lib, name, f)
    per = {}
    for name, k in calls.items():
        if name.endswith(QUERY):
            continue
        mult = 3 if name == "climsr_channel_attention_bwd" else 2 if name.startswith("climsr_channel_attention") else 1
        per[name] = k * mult
    return sum(per.values()), per


def stats(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="96,32")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--groups", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--lr", type=int, default=32)
    ap.add_argument("--no-torch", action="store_true", help="native side only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_rcan_train: no GPU (a timing needs the MI355X)")
    from climsr_amd.core.trainer import Trainer
    from climsr_amd.task.pl_generator_pre_training import SuperResolutionLightningModule
    from oracle import climsr_ref as ref

    dev, sf = "cuda", 4
    ng, nb = a.groups, a.blocks
    for batch_size in [int(b) for b in a.batches.split(",")]:
        torch.manual_seed(0)
        m = SuperResolutionLightningModule(
            generator={"_target_": "climsr_amd.models.rcan.TrainableRCAN", "n_resgroups": ng, "n_resblocks": nb, "n_feats": 64,
                       "reduction": 16, "scaling_factor": sf, "in_channels": 3, "out_channels": 1}, generator_type="rcan",
            optimizers={"generator_optimizer": {"_target_": "torch.optim.AdamW", "lr": 1e-4, "weight_decay": 1e-4}},
            schedulers={"generator_scheduler": {"_target_": "torch.optim.lr_scheduler.OneCycleLR", "max_lr": 1e-4,
                                                "num_training_steps": -1, "epochs": 1, "pct_start": 0.05, "div_factor": 2,
                                                "final_div_factor": 100}}).to(dev)
        total = 2 * (a.warmup + a.steps) + 8
        tr = Trainer(m, num_training_steps=total)
        batch = {k: v.to(dev) for k, v in ref.synthetic_batch(batch_size, a.lr * sf, seed=42, scale=sf).items()}
        cfg = {"n_resgroups": ng, "n_resblocks": nb, "scale": sf, "lr": a.lr, "batch": batch_size, "steps": a.steps,
               "warmup": a.warmup}
        step_no = [0]

        def native_step():
            out = tr.training_batch(batch, step_no[0])
            step_no[0] += 1
            return out

        for _ in range(a.warmup):
            native_step()
        torch.cuda.synchronize()
        pre = [timed(native_step)[0] for _ in range(3)]
        nlaunch, per_call = count_launches(native_step)
        print(json.dumps({"config": cfg, "native_only_preview_ms": stats(pre), "native_launches_per_step": nlaunch,
                          "launches_by_call": per_call}), flush=True)
        if a.no_torch:
            continue
        # ---- the same step in torch: fp32 master weights, autocast bf16 forward, autograd, torch.optim.AdamW + OneCycleLR
        q = {k: v.detach().clone().requires_grad_(True) for k, v in m.generator.state_dict().items()}
        opt = torch.optim.AdamW(list(q.values()), lr=1e-4, weight_decay=1e-4)
        sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-4, total_steps=total, pct_start=0.05, div_factor=2,
                                                  final_div_factor=100)

        def torch_step():
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                sr = ref.rcan_forward(q, batch["lr"], batch["elevation"], batch["mask"], ng, nb, sf)
            loss = ref.l1_loss(sr.float(), batch["hr"])
            loss.backward()
            opt.step()
            sch.step()
            return loss

        for _ in range(a.warmup):
            torch_step()
        torch.cuda.synchronize()
        nat, tor = [], []
        for _ in range(a.steps):
            nat.append(timed(native_step)[0])
            tor.append(timed(torch_step)[0])
        print(json.dumps({"config": cfg, "device": torch.cuda.get_device_name(0), "native_step_ms": stats(nat),
                          "torch_autocast_bf16_step_ms": stats(tor), "native_launches_per_step": nlaunch,
                          "native_over_torch": round(statistics.median(nat) / statistics.median(tor), 3)}), flush=True)
        del q, opt, sch, m, tr
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
