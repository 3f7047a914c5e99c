"""CPU checks of the inference front end (no GPU compute): ``climsr_infer_static`` / ``climsr_infer_prepare`` refuse bad
arguments before any launch and name the reason, the ctypes mirror of ``ClimsrInferDesc`` has gcc's layout, the Python
entry points refuse CPU tensors, and ``inference_on_series``' chunking and naming (``series_chunks``, pure host logic)
cover the short last chunk.  The driver itself needs pinned buffers and events, so its order of work is checked on the
GPU (tests/test_gpu_inference_pipeline.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "climsr_hip.h")
CSRC = os.path.join(ROOT, "climate-super-resolution_amd", "csrc")
FAKE = 64  # a non-null address that is never dereferenced: every call below must fail validation before a launch


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(CSRC, "libclimsr_hip.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-C", CSRC, "-j8"], check=True, capture_output=True)
    from climsr_amd import _lib

    return _lib.load()


def good_desc(**kw):
    """A lookup-route, esrgan-layout descriptor that passes validation; each case breaks it in one way."""
    from climsr_amd._lib import InferDesc

    f = dict(lr_raw=FAKE, lr_min=FAKE, lr_max=FAKE, lr_minmax=None, elev_hr=FAKE, mask_hr=FAKE, elev_lr=FAKE, mask_lr=FAKE,
             lr=FAKE, nearest=FAKE, out_min=FAKE, out_max=FAKE, range_a=-1.0, range_b=1.0, eps=1e-8, nan_sub=0.0, zs_mean=0.0,
             zs_std=1.0, zs_nan_sub=0.0, method=0, n=2, h=6, w=10, hr_h=24, hr_w=40, scale=4, lr_c=3, srcnn=0, use_elev=1,
             use_mask=1, flip_ud=1)
    f.update(kw)
    return InferDesc(**f)


PREPARE_CASES = {
    "null lr_raw": (dict(lr_raw=None), b"null pointer"),
    "null lr": (dict(lr=None), b"null pointer"),
    "null nearest": (dict(nearest=None), b"null pointer"),
    "null out_min": (dict(out_min=None), b"out_min"),
    "null static plane": (dict(elev_lr=None), b"static plane"),
    "null HR static plane for srcnn": (dict(srcnn=1, mask_hr=None), b"static plane"),
    "H != s*h": (dict(hr_h=25), b"is not scale"),
    "W != s*w": (dict(hr_w=36), b"is not scale"),
    "lr_c": (dict(lr_c=2), b"lr_c=2"),
    "lr_c without mask": (dict(use_mask=0), b"lr_c=3"),
    "both routes": (dict(lr_minmax=FAKE), b"2 statistics routes"),
    "neither route": (dict(lr_min=None, lr_max=None), b"0 statistics routes"),
    "half a lookup": (dict(lr_max=None), b"come together"),
    "both routes in z-score": (dict(method=1, lr_minmax=FAKE), b"2 statistics routes"),
    "method 3": (dict(method=3), b"method 3"),
    "method -1": (dict(method=-1), b"method -1"),
    "plane over 2^31 pixels": (dict(n=1, h=16384, w=16384, hr_h=65536, hr_w=65536), b"overflow"),
    "batch over 2^31 pixels": (dict(n=129, h=1024, w=1024, hr_h=4096, hr_w=4096), b"overflow"),
}


@pytest.mark.parametrize("case", list(PREPARE_CASES))
def test_prepare_validation_does_not_touch_the_gpu(lib, case):
    kw, reason = PREPARE_CASES[case]
    d = good_desc(**kw)
    assert lib.climsr_infer_prepare(ctypes.byref(d), None) == -1
    assert reason in lib.climsr_last_error(), lib.climsr_last_error()


def test_prepare_null_desc(lib):
    assert lib.climsr_infer_prepare(None, None) == -1
    assert b"null pointer" in lib.climsr_last_error()


def static_args(**kw):
    f = dict(elev_raw=FAKE, land_raw=FAKE, hr_h=24, hr_w=40, scale=4, range_a=-1.0, range_b=1.0, method=0, elev_missing=-32768.0,
             zs_mean=0.0, zs_std=1.0, zs_nan_sub=0.0, minmax=FAKE, elev_hr=2 * FAKE, mask_hr=FAKE, elev_lr=FAKE, mask_lr=FAKE,
             stream=None)
    f.update(kw)
    return list(f.values())


STATIC_CASES = {
    "null elevation": (dict(elev_raw=None), b"null pointer"),
    "null land raster": (dict(land_raw=None), b"null pointer"),
    "null output plane": (dict(mask_lr=None), b"null pointer"),
    "H not a multiple of scale": (dict(hr_h=25), b"multiples of scale"),
    "scale 0": (dict(scale=0), b"multiples of scale"),
    "method 3": (dict(method=3), b"method 3"),
    "no minmax scratch": (dict(minmax=None), b"minmax scratch"),
    "elev_hr aliases elev_raw": (dict(elev_hr=FAKE), b"alias"),
    "plane over 2^31 pixels": (dict(hr_h=65536, hr_w=65536), b"overflow"),
}


@pytest.mark.parametrize("case", list(STATIC_CASES))
def test_static_validation_does_not_touch_the_gpu(lib, case):
    kw, reason = STATIC_CASES[case]
    assert lib.climsr_infer_static(*static_args(**kw)) == -1
    assert reason in lib.climsr_last_error(), lib.climsr_last_error()


def test_infer_desc_offsets_match_gcc(lib, tmp_path):
    """The ctypes mirror has the size and field offsets gcc gives the header's ClimsrInferDesc."""
    from climsr_amd._lib import InferDesc

    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "climsr_hip.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(ClimsrInferDesc));']
    for f in InferDesc._fields_:
        lines.append(f'printf("{f[0]} %zu\\n", offsetof(ClimsrInferDesc, {f[0]}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    rows = [r.split() for r in filter(None, out)]
    assert len(rows) == 1 + len(InferDesc._fields_)
    for field, val in rows:
        got = ctypes.sizeof(InferDesc) if field == "size" else getattr(InferDesc, field).offset
        assert got == int(val), f"InferDesc.{field}: ctypes {got} != C {val}"


def test_pipeline_refuses_cpu_tensors():
    from climsr_amd.data import DeviceInferencePipeline

    with pytest.raises(RuntimeError, match="CUDA"):
        DeviceInferencePipeline(torch.zeros(24, 40), torch.zeros(24, 40), "esrgan")
    with pytest.raises(RuntimeError, match="CUDA"):
        DeviceInferencePipeline(np.zeros((24, 40), np.float32), np.zeros((24, 40), np.float32), "esrgan")


class HostPipeline:
    """What a pipeline on the host would look like: the driver has no such path."""
    device = torch.device("cpu")

    def __call__(self, lr_raw, lr_min=None, lr_max=None):  # pragma: no cover - must not be reached
        raise AssertionError("inference_on_series called a host pipeline")


def test_series_refuses_a_host_pipeline(tmp_path):
    from climsr_amd.inference import inference_on_series

    with pytest.raises(RuntimeError, match="CUDA"):
        inference_on_series(lambda lr, e, m: lr, HostPipeline(), np.zeros((3, 6, 10), np.float32), str(tmp_path))
    with pytest.raises(RuntimeError, match="CUDA"):
        inference_on_series(lambda lr, e, m: lr, object(), torch.zeros(3, 6, 10), str(tmp_path))
    assert os.listdir(tmp_path) == []


def test_series_chunks_and_names():
    from climsr_amd.inference import series_chunks

    assert series_chunks(5, 2) == [(0, 2, ["000000.tif", "000001.tif"]), (2, 4, ["000002.tif", "000003.tif"]),
                                   (4, 5, ["000004.tif"])]
    names = [f"cruts-tmp-1901-{m:02d}-16.tif" for m in range(1, 6)]
    assert series_chunks(5, 5, names) == [(0, 5, names)]
    assert series_chunks(5, 8, names) == [(0, 5, names)]
    assert [c[:2] for c in series_chunks(4, 1)] == [(0, 1), (1, 2), (2, 3), (3, 4)]
    got = series_chunks(5, 3, names)
    assert [n for _, _, ns in got for n in ns] == names  # time order, nothing lost or repeated
    for bad in (dict(total=0, batch_size=1), dict(total=3, batch_size=0), dict(total=3, batch_size=2, filenames=["a", "b"])):
        with pytest.raises(ValueError):
            series_chunks(**bad)
