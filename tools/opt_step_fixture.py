"""Bit patterns of the optimizer kernels (csrc/elementwise.hip) on fixed inputs: tests/golden/opt_step_parent.npz.

Drives whichever library ``CLIMSR_HIP_LIB`` names (default: the tree's) through the C ABI and writes the inputs (``in_*``)
and what the library computed from them (``out_*``) into one file.  The committed file was written with the library of
the commit before the five update entries became one kernel; tests/test_gpu_opt_fixture.py replays its inputs through
the tree's library (``replay``) and asks for the same bits.  Nothing depends on an RNG version: the draws are in the file.

* update: n = 4*256 + 3 (16-byte body, a block boundary, a 3-element tail), three consecutive steps from m = v = 0 with
  hp rows of non-default betas, bf16 mirror window lo = 3, mn = 514 (unaligned scalar stores at both ends, 8-byte stores
  inside) with 8 guard words behind it, gscale 0.37; final p, m, v (and mirror) of each of the five entries.
* tail: n = 3, 40 draws, one step each from non-zero m, v, for ``climsr_adamw_step`` and ``climsr_adam_step``.
* schedules: the hp row of every step and the final counters of ``climsr_adamw_hparams`` and of ``climsr_opt_hparams``
  for each kind, on the two schedules tests/test_gpu_opt_kernels.py uses.

    CLIMSR_HIP_LIB=/path/to/parent/libclimsr_hip.so python tools/opt_step_fixture.py [--out tests/golden/opt_step_parent.npz]
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N, LO, MN, GUARD, STEPS, GSCALE = 4 * 256 + 3, 3, 514, 8, 3, 0.37
TAIL_N, TAIL_DRAWS = 3, 40
GUARD_WORD = 0x7FC1  # a bf16 NaN pattern no update writes
ENTRIES = ("adamw_step", "adamw_step_mirror", "adamw_step_scaled", "adam_step", "adam_step_scaled")


def _hp_row(lr, b1, b2, eps, wd, t):
    return np.array([lr, b1, b2, eps, wd, lr / (1 - b1 ** t), math.sqrt(1 - b2 ** t), 0.0], dtype=np.float32)


def make_inputs():
    gen = torch.Generator().manual_seed(20)
    lr, b1, b2, eps, wd = 2e-3, 0.85, 0.98, 1e-7, 3e-2
    inp = {
        "in_p0": (torch.randn(N, generator=gen) * 0.1).numpy(),
        "in_g": (torch.randn(STEPS, N, generator=gen) * 0.02).numpy(),
        "in_hp": np.stack([_hp_row(lr, b1, b2, eps, wd, t) for t in range(1, STEPS + 1)]),
        "in_gscale": np.array([GSCALE], dtype=np.float32),
        "in_window": np.array([LO, MN, GUARD], dtype=np.int64),
        "in_tail_p": (torch.randn(TAIL_DRAWS, TAIL_N, generator=gen) * 0.1).numpy(),
        "in_tail_g": (torch.randn(TAIL_DRAWS, TAIL_N, generator=gen) * 0.02).numpy(),
        "in_tail_m": (torch.randn(TAIL_DRAWS, TAIL_N, generator=gen) * 0.01).numpy(),
        "in_tail_v": (torch.randn(TAIL_DRAWS, TAIL_N, generator=gen) * 0.01).square().numpy(),
        "in_tail_hp": _hp_row(lr, b1, b2, eps, wd, 7),
        # lr, beta1, beta2, eps, wd, div_factor, final_div_factor; the counters start at (3, 0): a resumed optimizer
        "in_sched_scalars": np.array([1e-3, 0.9, 0.999, 1e-8, 1e-4, 2.0, 100.0], dtype=np.float64),
        "in_sched_state0": np.array([3.0, 0.0], dtype=np.float64),
        # kind (SCHED_*), warmup, total, cycles, steps run
        "in_sched_lambda": np.array([[k, w, t, c, s] for w, t, s in ((4.0, 60.0, 20), (2.5, 20.0, 21))
                                     for k, c in ((1, 0.0), (2, 0.0), (3, 0.0), (4, 0.0), (5, 0.5), (5, 1.5), (6, 3.0))], dtype=np.float64),
        # total_steps, pct_start, steps run
        "in_sched_onecycle": np.array([[60, 0.05, 20], [20, 0.3, 20]], dtype=np.float64),
    }
    return inp


def _call(lib, entry, n, p, g, m, v, hp, gscale, lo, mn, mirror, stream):
    from climsr_amd import _lib

    head = (n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), hp.data_ptr())
    window = (lo, mn, _lib.ptr(mirror), stream)
    if entry == "adamw_step":
        args = head + (stream,)
    elif entry.endswith("_scaled"):
        args = head + (_lib.ptr(gscale),) + window
    else:
        args = head + window
    _lib.check(getattr(lib, "climsr_" + entry)(*args), entry)


def replay(lib, inp, dev="cuda"):
    """``out_*`` arrays (numpy, integer views of the bit patterns; float64 for the counters) of ``lib`` on ``inp``."""
    from climsr_amd import _lib

    s = _lib.stream_ptr()
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in inp.items() if isinstance(v, np.ndarray) and v.dtype != np.int64}
    lo, mn, guard = (int(x) for x in inp["in_window"])
    n = inp["in_p0"].shape[0]
    out = {}
    for entry in ENTRIES:
        p, m, v = t["in_p0"].clone(), torch.zeros_like(t["in_p0"]), torch.zeros_like(t["in_p0"])
        mirror = None
        if entry != "adamw_step":
            mirror = torch.full((mn + guard,), GUARD_WORD, dtype=torch.int16, device=dev)
        for k in range(t["in_g"].shape[0]):
            g, hp = t["in_g"][k].clone(), t["in_hp"][k].clone()  # allocations of their own: 16-byte aligned
            _call(lib, entry, n, p, g, m, v, hp, t["in_gscale"], lo, mn, mirror, s)
        torch.cuda.synchronize()
        for name, x in (("p", p), ("m", m), ("v", v)):
            out[f"out_{entry}_{name}"] = x.view(torch.int32).cpu().numpy()
        if mirror is not None:
            out[f"out_{entry}_mirror"] = mirror.cpu().numpy()
    for entry in ("adamw_step", "adam_step"):
        p, m, v = t["in_tail_p"].clone(), t["in_tail_m"].clone(), t["in_tail_v"].clone()
        for d in range(p.shape[0]):
            _call(lib, entry, p.shape[1], p[d], t["in_tail_g"][d], m[d], v[d], t["in_tail_hp"], None, 0, 0, None, s)
        torch.cuda.synchronize()
        out[f"out_tail_{entry}"] = torch.stack([p, m, v]).view(torch.int32).cpu().numpy()
    lr, b1, b2, eps, wd, div, fdiv = (float(x) for x in inp["in_sched_scalars"])
    hp = torch.zeros(8, dtype=torch.float32, device=dev)

    def rows(steps, launch):
        state = t["in_sched_state0"].clone()
        got = []
        for _ in range(int(steps)):
            _lib.check(launch(state), "hparams")
            got.append(hp.clone())
        return torch.stack(got).view(torch.int32).cpu().numpy(), state.cpu().numpy()

    for i, (kind, warmup, total, cycles, steps) in enumerate(inp["in_sched_lambda"]):
        out[f"out_sched_lambda{i}_hp"], out[f"out_sched_lambda{i}_state"] = rows(steps, lambda st: lib.climsr_opt_hparams(
            st.data_ptr(), int(kind), lr, b1, b2, eps, wd, float(warmup), float(total), float(cycles), 0.0, 0.0, 0.0, hp.data_ptr(), s))
    for i, (total, pct, steps) in enumerate(inp["in_sched_onecycle"]):
        out[f"out_sched_onecycle{i}_hp"], out[f"out_sched_onecycle{i}_state"] = rows(steps, lambda st: lib.climsr_opt_hparams(
            st.data_ptr(), 0, lr, b1, b2, eps, wd, 0.0, float(total), 0.0, float(pct), div, fdiv, hp.data_ptr(), s))
        out[f"out_adamw_hparams{i}_hp"], out[f"out_adamw_hparams{i}_state"] = rows(steps, lambda st: lib.climsr_adamw_hparams(
            st.data_ptr(), int(total), lr, float(pct), div, fdiv, b2, eps, wd, hp.data_ptr(), s))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "opt_step_parent.npz"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("opt_step_fixture: no GPU (the fixture is what the kernels compute on the MI355X)")
    from climsr_amd import _lib

    inp = make_inputs()
    out = replay(_lib.load(), inp)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    np.savez_compressed(a.out, **inp, **out)
    print(f"opt_step_fixture: {len(inp)} inputs, {len(out)} outputs from {_lib.LIB_PATH} -> {a.out} "
          f"({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
