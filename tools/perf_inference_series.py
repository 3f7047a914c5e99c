"""Times of the inference front end and of the series driver on whole CRU-TS grids (360 x 720 -> 1440 x 2880), run
on the GPU box:
    python tools/perf_inference_series.py [--n 8] [--grids 24] [--reps 20] [--skip-series]

* ``climsr_infer_prepare`` at ``--n`` whole grids, esrgan and srcnn layout, lookup route: median of ``--reps``
  HIP-event-timed launches after 5 warm-up launches.  Algorithmic bytes per launch: read the raw grids 4 B per LR pixel
  and the static planes once (8 B per LR pixel, or per HR pixel for srcnn); write ``nearest`` 4 B per HR pixel and ``lr``
  12 B per LR pixel (per HR pixel for srcnn).
* ``inference_on_series`` over ``--grids`` whole grids held on the host, batch size 1, to a writer that discards its
  input, with RCAN (10 x 20) and ESRGAN nb 11 initialised as ``bench.py --mode infer`` does: wall-clock milliseconds
  per grid (device synchronised at both ends, one 2-grid series as warm-up), and the pipeline's own time for one grid
  (both launches and its allocations, HIP events).  The bare model time to set it against is what
  ``bench.py --mode infer --model rcan|esrgan`` reports in the same session.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import climsr_amd  # noqa: E402,F401
from climsr_amd import _lib  # noqa: E402
from climsr_amd._lib import InferDesc, check, ptr  # noqa: E402
from climsr_amd.core.init import init_state, spec_from_shapes  # noqa: E402
from climsr_amd.data import DeviceInferencePipeline  # noqa: E402
from climsr_amd.inference import inference_on_series  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=8)
ap.add_argument("--grids", type=int, default=24)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--grid-h", type=int, default=360)
ap.add_argument("--grid-w", type=int, default=720)
ap.add_argument("--skip-series", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda:0")
S = 4
h, w = args.grid_h, args.grid_w
H, W = S * h, S * w


def event_median(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e))
    return statistics.median(times)  # ms


rs = np.random.RandomState(0)
elev = (rs.rand(H, W) * 5000 - 200).astype(np.float32)
land = rs.rand(H, W).astype(np.float32)
land[rs.rand(H, W) < 0.3] = np.nan


def raw_grids(n):
    g = rs.rand(n, h, w).astype(np.float32) * 55 - 25
    g[rs.rand(n, h, w) < 0.3] = np.nan
    return g


def show(row):
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)


def bench_prepare(gen):
    n = args.n
    p = DeviceInferencePipeline(torch.from_numpy(elev).to(dev), torch.from_numpy(land).to(dev), gen)
    raw = torch.from_numpy(raw_grids(n)).to(dev)
    mn = torch.full((n,), -31.5, dtype=torch.float64, device=dev)
    mx = torch.full((n,), 41.0, dtype=torch.float64, device=dev)
    srcnn = gen == "srcnn"
    lr = torch.empty((n, 3) + ((H, W) if srcnn else (h, w)), device=dev)
    nearest = torch.empty((n, 1, H, W), device=dev)
    omn, omx = torch.empty_like(mn), torch.empty_like(mx)
    d = InferDesc(lr_raw=ptr(raw), lr_min=ptr(mn), lr_max=ptr(mx), elev_hr=ptr(p.elevation), mask_hr=ptr(p.mask),
                  elev_lr=ptr(p.elevation_lr), mask_lr=ptr(p.mask_lr), lr=ptr(lr), nearest=ptr(nearest), out_min=ptr(omn),
                  out_max=ptr(omx), range_a=-1.0, range_b=1.0, eps=1e-8, nan_sub=0.0, zs_std=1.0, method=0, n=n, h=h, w=w, hr_h=H,
                  hr_w=W, scale=S, lr_c=3, srcnn=int(srcnn), use_elev=1, use_mask=1, flip_ud=1)
    L = _lib.load()
    ms = event_median(lambda: check(L.climsr_infer_prepare(ctypes.byref(d), _lib.stream_ptr(dev)), "infer_prepare"), args.reps)
    plane = (H * W) if srcnn else (h * w)
    nbytes = n * h * w * 4 + 8 * plane + n * H * W * 4 + n * 12 * plane
    own = torch.empty((n, 2), device=dev)
    ms_mm = event_median(lambda: check(L.climsr_tile_minmax_f32(ptr(raw), n, h * w, 0.0, 0, ptr(own), _lib.stream_ptr(dev)),
                                       "tile_minmax"), args.reps)
    show({"what": "infer_prepare", "layout": gen, "n": n, "lr": [h, w], "ms": ms, "bytes": nbytes, "GBps": nbytes / ms / 1e6,
          "ms_own_statistics_minmax": ms_mm})


def make_model(kind):
    if kind == "rcan":
        from climsr_amd.models.rcan import RCAN

        net = RCAN(n_resgroups=10, n_resblocks=20, n_feats=64, reduction=16, scaling_factor=4, in_channels=3, out_channels=1)
    else:
        from climsr_amd.models.esrgan import ESRGANGenerator

        net = ESRGANGenerator(in_channels=3, out_channels=1, nf=64, nb=11, gc=16, scale_factor=4)
    st = init_state(spec_from_shapes({k: tuple(v.shape) for k, v in net.state_dict().items()}))
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    return net.to(dev).eval()


def bench_series(kind):
    net = make_model(kind)
    p = DeviceInferencePipeline(torch.from_numpy(elev).to(dev), torch.from_numpy(land).to(dev), "esrgan", own_statistics=True)
    grids = raw_grids(args.grids)
    discard = lambda path, arr, profile=None: path  # noqa: E731
    with tempfile.TemporaryDirectory() as out_dir:
        inference_on_series(net, p, grids[:2], out_dir, writer=discard)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        inference_on_series(net, p, grids, out_dir, writer=discard)
        torch.cuda.synchronize()
        ms_grid = (time.perf_counter() - t0) * 1e3 / args.grids
    raw = torch.from_numpy(grids[:1]).to(dev)
    ms_front = event_median(lambda: p(raw), 10, warmup=3)
    show({"what": "inference_on_series", "model": kind, "grids": args.grids, "batch_size": 1, "ms_per_grid": ms_grid,
          "ms_pipeline_one_grid": ms_front})


bench_prepare("esrgan")
bench_prepare("srcnn")
if not args.skip_series:
    bench_series("rcan")
    bench_series("esrgan")
