"""On-device front end of whole-grid inference.

The reference prepares every inference grid on the CPU inside ``GeoTiffInferenceDataset`` /
``CRUTSInferenceDataset`` (climsr/data/sr/geo_tiff_inference_dataset.py, cruts_inference_dataset.py): flip the raw
LR grid, MinMax-normalise it (with looked-up float64 min / max, or with its own float32 nanmin / nanmax), NaN -> 0,
upscale with nearest for SRCNN and concatenate the static elevation and land-mask planes; once per dataset it masks
the HR elevation with the land raster, normalises it with its own nanmin / nanmax and decimates both planes to LR.
``DeviceInferencePipeline`` does the per-dataset part once in its constructor (``climsr_infer_static``) and the
per-grid part for a batch of raw grids in one launch (``climsr_infer_prepare``, after ``climsr_tile_minmax_f32`` in
the own-statistics route), bit for bit what the reference's scalers give.

No CPU fallback: inputs must be CUDA tensors and the HIP library must load.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Mapping, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from .. import _lib
from .._lib import InferDesc, check, ptr
from .tile_pipeline import ELEVATION_MISSING_INDICATOR

Stats = Optional[Union[Tensor, Sequence[float]]]


def _cuda_f32(t: Tensor, name: str) -> Tensor:
    if not isinstance(t, Tensor) or not t.is_cuda:
        raise RuntimeError(f"DeviceInferencePipeline: `{name}` must be a CUDA tensor (the pipeline runs in libclimsr_hip.so only)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"DeviceInferencePipeline: `{name}` must be float32 (raw grids), got {t.dtype}")
    return t.contiguous()


class DeviceInferencePipeline:
    """Raw LR grids ``[n, h, w]`` (NaN = sea) -> the reference's inference batch dict.

    ``elevation_raw`` and ``land_mask_raw`` are the raw HR rasters ``[H, W]`` the reference opens from
    ``elevation_file`` / ``land_mask_file`` (NaN in the land raster = sea; elevation ``-32768`` = missing), with
    ``H == scaling_factor * h``.  The other arguments mirror ``GeoTiffInferenceDataset.__init__``
    (geo_tiff_inference_dataset.py:21-38); ``standardize_stats`` is the mapping ``DeviceTilePipeline`` takes
    (``hr_mean, hr_std, hr_nan_sub, elev_mean, elev_std, elev_nan_sub``).

    Two statistics routes for min-max: by default each call takes looked-up float64 ``lr_min`` / ``lr_max`` (the GeoTIFF
    dataset: float64 arithmetic, one rounding); with ``own_statistics=True`` each grid is normalised with its own
    float32 nanmin / nanmax computed on the device (the CRU-TS dataset: float32 arithmetic throughout), and ``min`` /
    ``max`` are those statistics widened to float64.  ``flip_ud`` applies ``np.flipud`` to each raw grid first, as both
    reference datasets do.

    ``__call__`` returns ``lr``, ``elevation``, ``elevation_lr``, ``nearest``, ``mask``, ``min``, ``max`` (the last two
    only when a route gave them).  ``elevation`` and ``mask`` are ``[n, 1, H, W]`` copies of the static planes, made
    once per batch size and shared by later calls: treat them as read-only.  Nothing in ``__call__`` waits for the
    device when ``lr_min`` / ``lr_max`` are already CUDA tensors.

    Divergences from the reference, both declared: its CRU-TS dataset returns no ``mask`` item (so its own
    ``inference_on_full_images`` fails on it) and does not turn the elevation's missing indicator into NaN; this pipeline
    always returns the land mask and always treats ``-32768`` as missing, as the GeoTIFF dataset does.  In z-score mode
    the reference's GeoTIFF dataset raises (it passes ``missing_indicator`` to ``StandardScaler.normalize``), so there is
    no reference behaviour to match: the arithmetic is the training pipeline's (float64 ``(v - mean) / (std + eps)``
    rounded once, NaN replaced only by a non-zero ``nan_sub``).
    """

    def __init__(self, elevation_raw: Tensor, land_mask_raw: Tensor, generator_type: str, scaling_factor: int = 4,
                 normalize: bool = True, standardize: bool = False, standardize_stats: Optional[Mapping[str, float]] = None,
                 normalize_range: Tuple[float, float] = (-1.0, 1.0), use_elevation: bool = True, use_mask: bool = True,
                 own_statistics: bool = False, flip_ud: bool = True):
        elevation_raw = _cuda_f32(elevation_raw, "elevation_raw")
        land_mask_raw = _cuda_f32(land_mask_raw, "land_mask_raw")
        if elevation_raw.dim() != 2 or elevation_raw.shape != land_mask_raw.shape:
            raise ValueError(f"elevation_raw and land_mask_raw must be [H, W] rasters of one shape, got "
                             f"{tuple(elevation_raw.shape)} and {tuple(land_mask_raw.shape)}")
        if standardize and standardize_stats is None:
            raise ValueError("standardize=True needs standardize_stats (hr/elev mean, std, nan_sub)")
        self.generator_type = generator_type
        self.scaling_factor = s = int(scaling_factor)
        self.normalize = normalize
        self.standardize = standardize
        self.standardize_stats = dict(standardize_stats or {})
        self.normalize_range = tuple(float(v) for v in normalize_range)
        self.use_elevation = use_elevation
        self.use_mask = use_mask
        self.own_statistics = own_statistics
        self.flip_ud = flip_ud
        self.device = dev = elevation_raw.device
        H, W = elevation_raw.shape
        if s <= 0 or H % s or W % s:
            raise ValueError(f"raster {H}x{W} is not a multiple of scaling_factor {s}")
        self.hr_shape, self.lr_shape = (H, W), (H // s, W // s)
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        self.elevation, self.mask = new(1, 1, H, W), new(1, 1, H, W)
        self.elevation_lr, self.mask_lr = new(1, 1, H // s, W // s), new(1, 1, H // s, W // s)
        self.elevation_minmax = new(2)  # the masked elevation's own nanmin / nanmax (min-max mode)
        z = self.standardize_stats
        with torch.cuda.device(dev):
            check(_lib.load().climsr_infer_static(
                ptr(elevation_raw), ptr(land_mask_raw), H, W, s, self.normalize_range[0], self.normalize_range[1], self.method,
                ELEVATION_MISSING_INDICATOR, float(z.get("elev_mean", 0.0)), float(z.get("elev_std", 1.0)),
                float(z.get("elev_nan_sub", 0.0)), ptr(self.elevation_minmax), ptr(self.elevation), ptr(self.mask),
                ptr(self.elevation_lr), ptr(self.mask_lr), _lib.stream_ptr(dev)), "infer_static")
        self._expanded: Dict[int, Tuple[Tensor, Tensor, Tensor]] = {}

    @property
    def method(self) -> int:
        return 1 if self.standardize else (0 if self.normalize else 2)

    def _planes(self, n: int) -> Tuple[Tensor, Tensor, Tensor]:
        """[n,1,H,W] elevation and mask and [n,1,h,w] elevation_lr: the models' packers want contiguous planes, so the
        static ones are materialised once per batch size, not once per call."""
        if n not in self._expanded:
            self._expanded[n] = tuple(p.expand(n, -1, -1, -1).contiguous() for p in (self.elevation, self.mask, self.elevation_lr))
        return self._expanded[n]

    def __call__(self, lr_raw: Tensor, lr_min: Stats = None, lr_max: Stats = None) -> Dict[str, Tensor]:
        lr_raw = _cuda_f32(lr_raw, "lr_raw")
        if lr_raw.dim() == 4:
            lr_raw = lr_raw.reshape(lr_raw.shape[0], lr_raw.shape[2], lr_raw.shape[3])
        if lr_raw.dim() != 3 or tuple(lr_raw.shape[1:]) != self.lr_shape:
            raise ValueError(f"lr_raw must be [n, {self.lr_shape[0]}, {self.lr_shape[1]}] (the static rasters are "
                             f"{self.hr_shape[0]}x{self.hr_shape[1]} at scale {self.scaling_factor}), got {tuple(lr_raw.shape)}")
        if lr_raw.device != self.device:
            raise RuntimeError(f"DeviceInferencePipeline: `lr_raw` is on {lr_raw.device}, the static planes on {self.device}")
        n, h, w = lr_raw.shape
        H, W = self.hr_shape
        dev, method = self.device, self.method
        given = lr_min is not None or lr_max is not None
        if given and (lr_min is None or lr_max is None):
            raise ValueError("lr_min and lr_max come together")
        if self.own_statistics and given:
            raise ValueError("own_statistics=True normalises each grid with its own nanmin / nanmax: pass no lr_min / lr_max")
        if method == 0 and not self.own_statistics and not given:
            raise ValueError("min-max normalisation needs lr_min / lr_max (per-file or global stats), or own_statistics=True")
        L = _lib.load()
        mn = mx = own = out_mn = out_mx = None
        with torch.cuda.device(dev):
            stream = _lib.stream_ptr(dev)
            if given:
                mn = torch.as_tensor(lr_min, dtype=torch.float64).to(dev).reshape(n).contiguous()
                mx = torch.as_tensor(lr_max, dtype=torch.float64).to(dev).reshape(n).contiguous()
            elif self.own_statistics:
                own = torch.empty((n, 2), dtype=torch.float32, device=dev)
                check(L.climsr_tile_minmax_f32(ptr(lr_raw), n, h * w, 0.0, 0, ptr(own), stream), "tile_minmax")
            if given or self.own_statistics:
                out_mn = torch.empty(n, dtype=torch.float64, device=dev)
                out_mx = torch.empty(n, dtype=torch.float64, device=dev)
            srcnn = self.generator_type == "srcnn"
            lr_c = 1 + int(bool(self.use_elevation)) + int(bool(self.use_mask))
            lr = torch.empty((n, lr_c) + (self.hr_shape if srcnn else self.lr_shape), dtype=torch.float32, device=dev)
            nearest = torch.empty((n, 1, H, W), dtype=torch.float32, device=dev)
            z = self.standardize_stats
            d = InferDesc(lr_raw=ptr(lr_raw), lr_min=ptr(mn), lr_max=ptr(mx), lr_minmax=ptr(own), elev_hr=ptr(self.elevation),
                          mask_hr=ptr(self.mask), elev_lr=ptr(self.elevation_lr), mask_lr=ptr(self.mask_lr), lr=ptr(lr),
                          nearest=ptr(nearest), out_min=ptr(out_mn), out_max=ptr(out_mx), range_a=self.normalize_range[0],
                          range_b=self.normalize_range[1], eps=1e-8, nan_sub=0.0, zs_mean=float(z.get("hr_mean", 0.0)),
                          zs_std=float(z.get("hr_std", 1.0)), zs_nan_sub=float(z.get("hr_nan_sub", 0.0)), method=method, n=n,
                          h=h, w=w, hr_h=H, hr_w=W, scale=self.scaling_factor, lr_c=lr_c, srcnn=int(srcnn),
                          use_elev=int(bool(self.use_elevation)), use_mask=int(bool(self.use_mask)),
                          flip_ud=int(bool(self.flip_ud)))
            check(L.climsr_infer_prepare(ctypes.byref(d), stream), "infer_prepare")
            elevation, mask, elevation_lr = self._planes(n)
        out = {"lr": lr, "elevation": elevation, "elevation_lr": elevation_lr, "nearest": nearest, "mask": mask}
        if out_mn is not None:
            out["min"], out["max"] = out_mn, out_mx
        return out
