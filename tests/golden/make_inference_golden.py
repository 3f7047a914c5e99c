"""Generate tests/golden/inference_pipeline.npz with the REFERENCE's own scalers (climsr.data.normalization).

Run in the build container (needs /root/reference; never on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_inference_golden.py

``climsr.data.normalization`` imports only numpy/torch, so it runs here read-only.  The rest of the two inference
datasets (climsr/data/sr/geo_tiff_inference_dataset.py, cruts_inference_dataset.py) needs albumentations / cv2 / PIL /
xarray, which are absent, so their steps are written out below in the order the reference applies them:

* once per dataset (geo_tiff_inference_dataset.py:74-96): land mask = ~isnan(land raster), elevation masked with it,
  normalised with ``missing_indicator`` and its own nanmin / nanmax, both decimated with INTER_NEAREST at an integer
  ratio (== [::s, ::s]);
* per grid, lookup route (:153-176): flipud, ``scaler.normalize(img, min, max)`` with np.float64 min / max, nearest
  upscale (== np.repeat), ``_concat_if_needed`` (:98-116);
* per grid, own-statistics route (cruts_inference_dataset.py:77-94): flipud, np.nanmin / np.nanmax as the ``min`` /
  ``max`` items, ``scaler.normalize(img)``;
* z-score: the GeoTIFF dataset raises in this mode (it passes ``missing_indicator`` to ``StandardScaler.normalize``),
  so the case follows the training golden: StandardScaler with float64 statistics, the elevation's scaler holding the
  missing indicator.

The grids are non-square (6 x 10 at scale 4) so that a swapped stride or a flip along the wrong axis shows.
"""
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402

from climsr.data.normalization import MinMaxScaler, StandardScaler  # noqa: E402  (reference)

T, LH, LW, S = 5, 6, 10, 4
H, W = LH * S, LW * S
MISSING = -32768.0
RANGE = (-1.0, 1.0)
rs = np.random.RandomState(23)

lr_raw = rs.rand(T, LH, LW).astype(np.float32) * 45.0 - 15.0
yy, xx = np.mgrid[0:LH, 0:LW]
for t in range(T):
    lr_raw[t][xx + 2 * yy > 13 + t] = np.nan            # a NaN sea region in every grid, never symmetric in y
lr_raw[1][0:2, 0:3] = np.nan                            # a different NaN pattern in one grid
lr_raw[3] = np.nan                                      # one all-NaN grid
elev_raw = (rs.rand(H, W) * 4200.0 - 150.0).astype(np.float32)
elev_raw[:2, :] = MISSING                               # -32768 holes, partly over land
elev_raw[10:14, 25:33] = MISSING
land_raw = (rs.rand(H, W) * 5.0).astype(np.float32)
hy, hx = np.mgrid[0:H, 0:W]
land_raw[hx + 1.5 * hy > 46] = np.nan                  # sea, ~30 % of the raster, over valid elevation values
land_raw[5:9, 3:8] = np.nan
own = [(np.nanmin(g), np.nanmax(g)) if not np.all(np.isnan(g)) else (-15.0, 30.0) for g in lr_raw]
lr_min = np.array([m for m, _ in own], np.float64) - 1.75   # looked-up stats, not the grids' own extremes
lr_max = np.array([m for _, m in own], np.float64) + 2.5
zs = dict(hr_mean=3.25, hr_std=11.5, hr_nan_sub=-0.75, elev_mean=812.0, elev_std=640.5, elev_nan_sub=-1.25)


def static_planes(method):
    land_mask = ~np.isnan(land_raw)
    elev = np.where(land_mask, elev_raw, np.nan)  # mask Antarctica
    if method == "zscore":
        elev = StandardScaler(mean=np.float64(zs["elev_mean"]), std=np.float64(zs["elev_std"]), missing_indicator=MISSING,
                              nan_substitution=np.float64(zs["elev_nan_sub"])).normalize(arr=elev.copy())
    else:
        elev = MinMaxScaler(feature_range=RANGE).normalize(elev, missing_indicator=MISSING)
    assert elev.dtype == np.float32 and not np.isnan(elev).any()
    mask = land_mask.astype(np.float32)
    return elev, elev[::S, ::S], mask, mask[::S, ::S]


def batch(route, srcnn=False, use_elev=True, use_mask=True, flip=True):
    elev, elev_lr, mask, mask_lr = static_planes(route)
    keys = ("lr", "nearest", "elevation", "elevation_lr", "mask")
    out = {k: [] for k in keys}
    mins, maxes = [], []
    for t in range(T):
        img = (np.flipud(lr_raw[t]) if flip else lr_raw[t]).copy()
        if route == "lookup":
            mn, mx = np.float64(lr_min[t]), np.float64(lr_max[t])
            img = MinMaxScaler(feature_range=RANGE).normalize(img, mn, mx)
        elif route == "own":
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)  # the all-NaN grid
                mn, mx = np.nanmin(img), np.nanmax(img)
                img = MinMaxScaler(feature_range=RANGE).normalize(img)
            assert mn.dtype == np.float32
        else:
            mn = mx = None
            img = StandardScaler(mean=np.float64(zs["hr_mean"]), std=np.float64(zs["hr_std"]),
                                 nan_substitution=np.float64(zs["hr_nan_sub"])).normalize(arr=img)
        assert img.dtype == np.float32
        nearest = np.repeat(np.repeat(img, S, 0), S, 1)
        chans = [nearest if srcnn else img]
        if use_elev:
            chans.append(elev if srcnn else elev_lr)
        if use_mask:
            chans.append(mask if srcnn else mask_lr)
        for k, v in zip(keys, (np.stack(chans), nearest[None], elev[None], elev_lr[None], mask[None])):
            out[k].append(v)
        mins.append(mn)
        maxes.append(mx)
    res = {k: np.stack(v).astype(np.float32) for k, v in out.items()}
    if route != "zscore":
        res["min"], res["max"] = np.array(mins, np.float64), np.array(maxes, np.float64)
    return res


CASES = {"lookup_esrgan": dict(route="lookup"), "lookup_srcnn": dict(route="lookup", srcnn=True),
         "lookup_no_elev": dict(route="lookup", use_elev=False), "lookup_no_mask": dict(route="lookup", use_mask=False),
         "own_esrgan": dict(route="own"), "own_esrgan_noflip": dict(route="own", flip=False), "zscore_esrgan": dict(route="zscore")}

arrays = dict(lr_raw=lr_raw, elev_raw=elev_raw, land_raw=land_raw, lr_min=lr_min, lr_max=lr_max,
              zscore=np.array([zs[k] for k in ("hr_mean", "hr_std", "hr_nan_sub", "elev_mean", "elev_std", "elev_nan_sub")]))
for name, kw in CASES.items():
    for k, v in batch(**kw).items():
        arrays[f"{name}/{k}"] = v
own_case = {k: arrays[f"own_esrgan/{k}"] for k in ("lr", "min", "max")}
assert np.all(own_case["lr"][3, 0] == 0.0) and np.isnan(own_case["min"][3]) and np.isnan(own_case["max"][3])
assert not np.array_equal(arrays["own_esrgan/lr"], arrays["own_esrgan_noflip/lr"])
np.savez_compressed(os.path.join(HERE, "inference_pipeline.npz"), **arrays)
print("wrote", os.path.join(HERE, "inference_pipeline.npz"), sum(v.nbytes for v in arrays.values()) // 1024, "KiB raw")
