"""Whole-image inference driver (mirror of ``climsr/inference/inference.py:27-113``).

``inference_on_full_images`` runs the generator on each full grid, denormalises the SR map with the grid's
min / max and puts NaN over the sea on the device (``climsr_denormalize_mask``), then hands the float32 raster
to a writer.  The reference writes GeoTIFFs through rasterio with the land-mask file's profile; rasterio is not
part of this image, so the default writer stores ``<filename>.npy`` and a rasterio writer is used when the
module is importable and a ``profile`` is given.

``inference_on_series`` is the same for a whole time series of raw grids: it prepares each chunk on the device with
``climsr_amd.data.DeviceInferencePipeline`` and overlaps the writing of one chunk with the device work of the next.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._lib import check, ptr


def denormalize_mask(sr: Tensor, mask: Optional[Tensor], mins, maxes, normalization_range=(-1.0, 1.0)) -> Tensor:
    """[n,1,h,w] fp32 SR map -> denormalised fp32 with NaN where mask == 0 (inference.py:73-76), on the device."""
    if not sr.is_cuda:
        raise RuntimeError("denormalize_mask runs in libclimsr_hip.so: CUDA tensors only")
    n = sr.shape[0]
    hw = sr[0].numel()
    s = sr.detach().float().contiguous()
    m = mask.detach().float().contiguous() if mask is not None else None
    mn = torch.as_tensor(mins, dtype=torch.float64).reshape(n).to(sr.device)
    mx = torch.as_tensor(maxes, dtype=torch.float64).reshape(n).to(sr.device)
    out = torch.empty_like(s)
    check(_lib.load().climsr_denormalize_mask(ptr(s), ptr(m), ptr(mn), ptr(mx), float(normalization_range[0]),
                                              float(normalization_range[1]), n, hw, ptr(out), _lib.stream_ptr(sr.device)),
          "denormalize_mask")
    return out


def npy_writer(path: str, arr: np.ndarray, profile: Optional[dict] = None) -> str:
    path = os.path.splitext(path)[0] + ".npy"
    np.save(path, arr)
    return path


def default_writer() -> Callable[..., str]:
    try:  # pragma: no cover - rasterio is not installed in the build image
        import rasterio as rio

        def tif_writer(path: str, arr: np.ndarray, profile: Optional[dict] = None) -> str:
            if profile is None:
                return npy_writer(path, arr)
            with rio.open(path, "w", **profile) as raster:
                raster.write(arr, 1)
            return path

        return tif_writer
    except ImportError:
        return npy_writer


def inference_on_full_images(model, batches: Iterable[Dict[str, Tensor]], out_dir: str,
                             normalization_range: Tuple[float, float] = (-1.0, 1.0), profile: Optional[dict] = None,
                             writer: Optional[Callable[..., str]] = None) -> list:
    """Batch keys as the reference's inference datasets: lr, elevation, mask (CUDA), min, max, filename."""
    os.makedirs(out_dir, exist_ok=True)
    writer = writer or default_writer()
    written = []
    with torch.no_grad():
        for batch in batches:
            sr = model(batch["lr"], batch["elevation"], batch["mask"])
            den = denormalize_mask(sr, batch["mask"], batch["min"], batch["max"], normalization_range).cpu().numpy()
            names = batch["filename"]
            names = [names] if isinstance(names, str) else list(names)
            for i, name in enumerate(names):
                written.append(writer(os.path.join(out_dir, name), den[i, 0], profile))
    return written


def series_chunks(total: int, batch_size: int, filenames: Optional[Sequence[str]] = None) -> List[Tuple[int, int, List[str]]]:
    """The chunks of a series of ``total`` grids in time order: ``(start, stop, names)`` with ``stop - start ==
    batch_size`` except for a short last chunk.  Default names are ``000000.tif``, ``000001.tif``, ..."""
    if total <= 0:
        raise ValueError(f"inference_on_series: empty series (T={total})")
    if batch_size <= 0:
        raise ValueError(f"inference_on_series: batch_size must be positive, got {batch_size}")
    names = [f"{i:06d}.tif" for i in range(total)] if filenames is None else [str(f) for f in filenames]
    if len(names) != total:
        raise ValueError(f"inference_on_series: {len(names)} filenames for {total} grids")
    return [(i, min(i + batch_size, total), names[i:min(i + batch_size, total)]) for i in range(0, total, batch_size)]


def inference_on_series(model, pipeline, grids, out_dir: str, filenames: Optional[Sequence[str]] = None, batch_size: int = 1,
                        lr_min=None, lr_max=None, normalization_range: Tuple[float, float] = (-1.0, 1.0),
                        profile: Optional[dict] = None, writer: Optional[Callable[..., str]] = None) -> list:
    """A whole time series of raw LR grids ``[T, h, w]`` (float32 numpy array, CPU tensor or CUDA tensor) -> one SR
    raster per grid, written in time order.  ``pipeline`` is a ``climsr_amd.data.DeviceInferencePipeline``; ``lr_min`` /
    ``lr_max`` are its per-grid float64 lookup statistics ``[T]`` (none with ``own_statistics=True``).

    Per chunk of ``batch_size`` grids: copy to the device (through one of two pinned staging buffers when the series is
    on the host), ``pipeline``, ``model(lr, elevation, mask)``, ``denormalize_mask`` with the batch's ``min`` / ``max``,
    then an asynchronous copy into one of two pinned host buffers followed by an event.  Chunk k+1 is enqueued before
    chunk k's event is waited on and its rasters go to ``writer``, so encoding and writing one chunk overlaps the device
    work of the next.  The rasters are bit-identical to ``inference_on_full_images`` over the same batches.
    """
    dev = getattr(pipeline, "device", None)
    if not isinstance(dev, torch.device) or dev.type != "cuda":
        raise RuntimeError("inference_on_series runs in libclimsr_hip.so: the pipeline must live on a CUDA device")
    if isinstance(grids, np.ndarray):
        grids = torch.from_numpy(grids)
    if not isinstance(grids, Tensor) or grids.dim() != 3 or grids.dtype != torch.float32:
        raise ValueError("inference_on_series: `grids` must be a float32 [T, h, w] numpy array or tensor")
    chunks = series_chunks(grids.shape[0], int(batch_size), filenames)
    stats = None
    if lr_min is not None or lr_max is not None:
        if lr_min is None or lr_max is None:
            raise ValueError("lr_min and lr_max come together")
        stats = tuple(torch.as_tensor(v, dtype=torch.float64).reshape(grids.shape[0]).to(dev) for v in (lr_min, lr_max))
    os.makedirs(out_dir, exist_ok=True)
    writer = writer or default_writer()
    on_host = not grids.is_cuda
    nmax = chunks[0][1] - chunks[0][0]
    pinned = lambda *shape: torch.empty(shape, dtype=torch.float32).pin_memory()  # noqa: E731
    stage_in = [pinned(nmax, *grids.shape[1:]) for _ in range(2)] if on_host else None
    stage_out: List[Optional[Tensor]] = [None, None]
    events = [torch.cuda.Event(), torch.cuda.Event()]
    written: list = []

    def drain(slot: int, names: List[str]) -> None:
        events[slot].synchronize()
        den = stage_out[slot].numpy()
        for i, name in enumerate(names):  # the writer gets its own array: the staging buffer is reused two chunks on
            written.append(writer(os.path.join(out_dir, name), den[i, 0].copy(), profile))

    pending = None
    with torch.no_grad(), torch.cuda.device(dev):
        for k, (i0, i1, names) in enumerate(chunks):
            slot, n = k & 1, i1 - i0
            if on_host:  # slot's previous upload (chunk k-2) finished before chunk k-2's event, already waited on
                stage_in[slot][:n].copy_(grids[i0:i1])
                raw = stage_in[slot][:n].to(dev, non_blocking=True)
            else:
                raw = grids[i0:i1]
            batch = pipeline(raw) if stats is None else pipeline(raw, stats[0][i0:i1], stats[1][i0:i1])
            if "min" not in batch:
                raise RuntimeError("inference_on_series denormalises with MinMaxScaler: the pipeline must return min / max "
                                   "(min-max normalisation with lookup or own statistics)")
            sr = model(batch["lr"], batch["elevation"], batch["mask"])
            den = denormalize_mask(sr, batch["mask"], batch["min"], batch["max"], normalization_range)
            if stage_out[slot] is None:
                stage_out[slot] = pinned(nmax, *den.shape[1:])
            stage_out[slot][:n].copy_(den, non_blocking=True)
            events[slot].record()
            if pending is not None:
                drain(*pending)
            pending = (slot, names)
        drain(*pending)
    return written
