"""Time of the segmented gradient norm (climsr_grad_norm) and of the scaled AdamW beside the plain one.

Two flat gradient buffers ("Gradient norms and clipping"):
  - the RRDB generator's (nf 64, nb 11, gc 16; a few tens of MB: it stays in the caches between repeats), and
  - the RFB discriminator's (~107 M elements, ~430 MB: a pure HBM stream).
Each call is timed with its own pair of device events (the call's three launches together), after a warm-up; medians
over --reps calls.  GB/s counts the gradient read once; the ratio is against one read of the buffer at the achievable
HBM rate (--hbm-tbs, 6.3 TB/s).  On the discriminator's buffer climsr_adamw_step (mirror variant, as the trainer
launches it) and climsr_adamw_step_scaled are timed in alternating calls on the same buffers.  Prints one JSON line.

    python tools/perf_gradnorm.py [--reps 50] [--warmup 5] [--parent-lib /path/to/another/libclimsr_hip.so]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def summary(evs):
    ms = [e0.elapsed_time(e1) for e0, e1 in evs]
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hbm-tbs", type=float, default=6.3)
    ap.add_argument("--parent-lib", default=None, help="another libclimsr_hip.so: time its climsr_adamw_step_mirror beside the tree's")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_gradnorm: no GPU (a timing needs the MI355X)")
    from climsr_amd import _lib
    from climsr_amd.core.optim import GradNorm, _mirror_of
    from climsr_amd.models.esrgan import ESRGANGenerator
    from climsr_amd.models.rfb_esrgan import RFBESRGANDiscriminator

    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    out = {"device": torch.cuda.get_device_name(0), "chunk": lib.climsr_grad_norm_chunk(), "reps": a.reps, "norm": {}}
    nets = {"generator_nb11": ESRGANGenerator(in_channels=3, out_channels=1, nf=64, nb=11, gc=16, scale_factor=4).to("cuda"),
            "rfb_discriminator": RFBESRGANDiscriminator(in_channels=1).to("cuda")}
    for name, net in nets.items():
        g = net._flat_grad
        g.normal_(0.0, 1e-3, generator=torch.Generator(device="cuda").manual_seed(3))
        net.grads_as_views()
        gn = GradNorm(net)
        row = {"elements": g.numel(), "MB": round(4 * g.numel() / 1e6, 2), "segments": len(net._flat_index)}
        for kind in (2, "inf"):
            for _ in range(a.warmup):
                gn(kind, 1.0, gathered=True)
            torch.cuda.synchronize()
            evs = [timed(lambda: gn(kind, 1.0, gathered=True)) for _ in range(a.reps)]
            torch.cuda.synchronize()
            r = summary(evs)
            r["GBps"] = round(4 * g.numel() / (r["median_ms"] * 1e-3) / 1e9, 1)
            r["x_one_read_at_hbm_rate"] = round(r["median_ms"] * 1e-3 / (4 * g.numel() / (a.hbm_tbs * 1e12)), 2)
            row["l2" if kind == 2 else "inf"] = r
        total = float(gn(2, 1.0, gathered=True)[1])
        want = float(g.double().norm())
        row["total_rel_err_vs_torch_fp64"] = abs(total - want) / want
        out["norm"][name] = row
    # plain vs scaled AdamW on the discriminator's buffers, alternating
    d = nets["rfb_discriminator"]
    flat, g = d._flat, d._flat_grad
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    hp = torch.tensor([1e-4, 0.9, 0.999, 1e-8, 1e-4, 1e-3, 0.0316, 0.0], dtype=torch.float32, device="cuda")
    coef = torch.tensor([0.5], dtype=torch.float32, device="cuda")
    lo, mn, buf = _mirror_of(d)
    n = flat.numel()

    def plain():
        _lib.check(lib.climsr_adamw_step_mirror(n, flat.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), hp.data_ptr(), lo, mn,
                                                buf.data_ptr(), s), "adamw")

    def scaled():
        _lib.check(lib.climsr_adamw_step_scaled(n, flat.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), hp.data_ptr(),
                                                coef.data_ptr(), lo, mn, buf.data_ptr(), s), "adamw_scaled")

    for _ in range(a.warmup):
        plain()
        scaled()
    torch.cuda.synchronize()
    ev = {"adamw_step_mirror": [], "adamw_step_scaled": []}
    for _ in range(a.reps):
        ev["adamw_step_mirror"].append(timed(plain))
        ev["adamw_step_scaled"].append(timed(scaled))
    torch.cuda.synchronize()
    nbytes = 28 * n + 2 * mn
    out["adamw_on_discriminator"] = {"algorithmic_MB": round(nbytes / 1e6, 1)}
    for k, evs in ev.items():
        r = summary(evs)
        r["GBps"] = round(nbytes / (r["median_ms"] * 1e-3) / 1e9, 1)
        out["adamw_on_discriminator"][k] = r
    if a.parent_lib:  # the same entry of another build of the library (a parent commit's), alternating with the tree's
        import ctypes

        other = ctypes.CDLL(a.parent_lib)
        other.climsr_adamw_step_mirror.restype, other.climsr_adamw_step_mirror.argtypes = _lib.SIGNATURES["climsr_adamw_step_mirror"]

        def parent():
            assert other.climsr_adamw_step_mirror(n, flat.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), hp.data_ptr(), lo, mn,
                                                  buf.data_ptr(), s) == 0

        for _ in range(a.warmup):
            parent()
            plain()
        torch.cuda.synchronize()
        ev = {"parent": [], "tree": []}
        for _ in range(a.reps):
            ev["parent"].append(timed(parent))
            ev["tree"].append(timed(plain))
        torch.cuda.synchronize()
        out["adamw_step_mirror_parent_vs_tree"] = {k: summary(evs) for k, evs in ev.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
