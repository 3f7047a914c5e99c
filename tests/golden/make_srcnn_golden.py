"""Stand-alone SRCNN golden fixture: the MSE task of ``generator_type: "srcnn"`` (task.py:141,235-239).

Run in the build container (needs the reference checkout make_golden.py imports from; never on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_srcnn_golden.py

The generator is the REFERENCE's own ``climsr/models/srcnn.py`` (imported read-only) in float64; the loss is
``torch.nn.MSELoss`` (task.py:141); the step is ``climsr/task/pl_generator_pre_training.py:18-33`` with
conf/optimizers/adamw.yaml (lr 1e-4, weight_decay 1e-4) and conf/schedulers/one_cycle_schedule.yaml (total_steps 10),
Lightning's automatic-optimisation order restated as in make_config1_golden.py.

The SRCNN batch is what the tile pipeline's "srcnn" mode produces (climate_dataset.py: the LR tile upscaled back to HR
size with nearest neighbour, then elevation and mask as channels): ``cat([nearest x4(lr[:, :1]), elevation, mask])``
of the synthetic batch.

Output: tests/golden/srcnn_steps.npz (all float64 unless noted)
  meta                      json string: shapes, seeds, total_steps, key order
  init.<key>                initial state (in_channels 3), deterministic (climsr_amd.core.init)
  loss, lr                  [3] per step (lr = the optimizer's lr the step was taken with)
  grads0.<key>              gradients of the first step
  final.<key>               parameters after the three steps
  fwd<c>.x, fwd<c>.sr, fwd<c>.<key>   forward-only records, in_channels c = 1, 2 at B=1, 33x40: input, output, state
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from make_golden import batch, det_state, load, to64  # noqa: E402

from climsr.models.srcnn import SRCNN  # noqa: E402  (reference)

SEEDS = (300, 301, 302)
TOTAL_STEPS = 10
B, HR = 2, 48
FWD_SEEDS = {1: 311, 2: 312}
FWD_HW = (33, 40)


def srcnn_input(bt, c=3):
    up = bt["lr"][:, :1].repeat_interleave(4, dim=-2).repeat_interleave(4, dim=-1)  # cv2 INTER_NEAREST x4
    return torch.cat([up, bt["elevation"], bt["mask"]], 1)[:, :c].contiguous()


def main():
    g = SRCNN(in_channels=3, out_channels=1)
    st = det_state(g)
    g = load(g, st).double().train()
    keys = list(st.keys())
    rec = {f"init.{k}": np.asarray(v, dtype=np.float64) for k, v in st.items()}
    opt = torch.optim.AdamW(g.parameters(), lr=1e-4, weight_decay=1e-4)
    sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-4, total_steps=TOTAL_STEPS, epochs=1, pct_start=0.05,
                                              div_factor=2, final_div_factor=100)
    crit = nn.MSELoss()
    losses, lrs = [], []
    for s, seed in enumerate(SEEDS):
        bt = to64(batch(B, HR, seed=seed))
        opt.zero_grad()
        sr = g(srcnn_input(bt))
        loss = crit(sr, bt["hr"])
        loss.backward()
        if s == 0:
            rec.update({f"grads0.{k}": p.grad.detach().numpy().copy() for k, p in g.named_parameters()})
        losses.append(float(loss))
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        sch.step()
        print("step", s, float(loss), flush=True)
    rec["loss"], rec["lr"] = np.asarray(losses), np.asarray(lrs)
    rec.update({f"final.{k}": p.detach().numpy().copy() for k, p in g.named_parameters()})
    for c, seed in FWD_SEEDS.items():
        gc = SRCNN(in_channels=c, out_channels=1)
        stc = det_state(gc)
        gc = load(gc, stc).double().eval()
        x = srcnn_input(to64(batch(1, HR, seed=seed)), c)[:, :, :FWD_HW[0], :FWD_HW[1]].contiguous()
        with torch.no_grad():
            sr = gc(x)
        rec[f"fwd{c}.x"], rec[f"fwd{c}.sr"] = x.numpy(), sr.numpy()
        rec.update({f"fwd{c}.{k}": np.asarray(v, dtype=np.float64) for k, v in stc.items()})
    rec["meta"] = np.asarray(json.dumps({
        "model": "climsr.models.srcnn.SRCNN(in_channels=3, out_channels=1), float64", "loss": "torch.nn.MSELoss",
        "optimizer": "torch.optim.AdamW(lr=1e-4, weight_decay=1e-4)",
        "scheduler": "OneCycleLR(max_lr=1e-4, total_steps=10, pct_start=0.05, div_factor=2, final_div_factor=100)",
        "input": "cat([nearest x4(lr[:, :1]), elevation, mask]) of synthetic_batch(batch, hr_size, seed)",
        "batch": B, "hr_size": HR, "seeds": list(SEEDS), "total_steps": TOTAL_STEPS, "keys": keys,
        "fwd": {str(c): {"seed": s, "hw": list(FWD_HW), "from_hr_size": HR} for c, s in FWD_SEEDS.items()}}))
    np.savez_compressed(os.path.join(HERE, "srcnn_steps.npz"), **rec)


if __name__ == "__main__":
    main()
