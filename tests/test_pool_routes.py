"""The max-pool epilogue (ClimsrEpilogue.down2 == 2) in the dispatch, on the CPU.

climsr_conv2d_fwd_kernel formats the route climsr_conv2d_fwd launches from and answers "" for arguments it refuses, so
it is the query PerceptualLoss asks (ConvPlan.pool2_ok) before it drops a MaxPool2d kernel.  Asked here through
ConvPlan.fwd / pool2_ok with a launch observer that records the name and runs nothing: no device, placeholder tensors.
The four pooled VGG19 layers at the GAN-step shapes (64 images of 256^2) must name the two pooled kernels, everything the
epilogue is not defined for must be refused, and the same descriptors without the pool keep their kernels."""
import pytest
import torch

from climsr_amd import _lib, ops
from climsr_amd.ops import ACT_LRELU, ACT_NONE, ACT_RELU, OUT_F32, ConvPlan

B = 64
WR_POOL, DMA_POOL = "conv_wr_kernel<5>", "conv_fwd_dma_kernel<11, false>"
# conv1_2, conv2_2, conv3_4, conv4_4: (cin, cout, side), the pooled kernel, the un-pooled one
PRODUCT = [((64, 64, 256), WR_POOL, "conv_wr_kernel<0>"), ((128, 128, 128), DMA_POOL, "conv_fwd_dma_kernel<3, false>"),
           ((256, 256, 64), DMA_POOL, "conv_fwd_dma_kernel<3, false>"), ((512, 512, 32), DMA_POOL, "conv_fwd_dma_kernel<3, false>")]


@pytest.fixture
def routes(monkeypatch):
    try:
        _lib.load()
    except OSError as e:  # the built library is a prerequisite of the whole CPU suite (test_abi)
        pytest.skip(f"libclimsr_hip.so not loadable: {e}")
    names = []
    monkeypatch.setattr(ops, "PROFILER", lambda name, flops, fn, tag="", nbytes=0: names.append(name))
    monkeypatch.setattr(_lib, "stream_ptr", lambda: 0)  # (read before the recorded launches; no device here)
    return names


def t(dtype=torch.bfloat16):
    return torch.empty(8, dtype=dtype)


def plan(cin, cout, stride=1, bias=True):
    p = ConvPlan(cin, cout, 3, stride, None, "route")
    p.weight = torch.zeros(1)
    p.bias = torch.zeros(cout) if bias else None
    return p


@pytest.mark.parametrize("shape,pooled,plain", PRODUCT)
def test_product_shapes_take_the_pooled_kernels(routes, shape, pooled, plain):
    cin, cout, s = shape
    p = plan(cin, cout)
    assert p.pool2_ok(cin, 0, s, s, B, cout)
    p.fwd(t(), cin, 0, s, s, t(), cout, 0, B, act=ACT_RELU, pool2=True)
    p.fwd(t(), cin, 0, s, s, t(), cout, 0, B, act=ACT_RELU)
    assert routes == [pooled, plain]


# what the epilogue is not defined for (the GPU suite launches the same list and finds the output untouched):
# (cin, cout, stride, h, w, fwd keywords)
REFUSED = {
    "odd_h": (64, 64, 1, 7, 16, {}),
    "odd_w": (64, 64, 1, 8, 15, {}),
    "lrelu": (64, 64, 1, 8, 16, dict(act=ACT_LRELU)),
    "no_act": (64, 64, 1, 8, 16, dict(act=ACT_NONE)),
    "no_bias": (64, 64, 1, 8, 16, dict(use_bias=False)),
    "f32_out": (64, 64, 1, 8, 16, dict(out_mode=OUT_F32)),
    "res1": (64, 64, 1, 8, 16, dict(res1="bf16", res1_cs=64)),
    "bn_part": (64, 128, 1, 32, 32, dict(bn_part="f64")),
    "n16_family": (64, 16, 1, 8, 16, {}),
    "stride2": (64, 64, 2, 16, 32, {}),
    "dma_small_tile": (64, 128, 1, 16, 16, {}),
    "odd_h_dma": (64, 128, 1, 97, 32, {}),
}


def refused_kw(kw):
    kw = dict(kw)
    kw.setdefault("act", ACT_RELU)
    for k, dt in (("res1", torch.bfloat16), ("bn_part", torch.float64)):
        if k in kw:
            kw[k] = t(dt)
    return kw


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusals_answer_through_the_query(routes, case):
    cin, cout, stride, h, w, kw = REFUSED[case]
    p = plan(cin, cout, stride)
    kw = refused_kw(kw)
    y = t(torch.float32 if kw.get("out_mode") == OUT_F32 else torch.bfloat16)
    p.fwd(t(), cin, 0, h, w, y, cout, 0, 2, pool2=True, **kw)
    assert routes == [""], routes
    assert _lib.load().climsr_last_error().decode().startswith("conv2d_fwd: max-pool epilogue"), "its own message"
    if set(kw) <= {"act", "use_bias", "out_mode"}:  # what pool2_ok() itself can ask
        assert not p.pool2_ok(cin, 0, h, w, 2, cout, **kw)
    # the same conv without the pool is a valid launch (bn_part: asks for partials of a biased ReLU output, not one)
    if case != "bn_part":
        p.fwd(t(), cin, 0, h, w, y, cout, 0, 2, **kw)
        assert routes[-1] != "", case


def test_values_0_and_1_keep_their_checks(routes):
    """down2 = 1 (the 2x2 sum of a data gradient) still refuses a bias, with its own message; 0 is untouched."""
    lib = _lib.load()
    p = plan(64, 64)
    d = _lib.ConvDesc(2, 8, 16, 64, 64, 0, 1, 3, 1, 1, 8, 16, 64, 64, 0, p.cc)
    ep = _lib.Epilogue(ACT_RELU, 0.0, 1.0, None, 0, 0, 1.0, None, 0, 0, 0, 1)
    assert lib.climsr_conv2d_fwd_kernel(d, 1, ep) == b""
    assert lib.climsr_last_error().decode().startswith("conv2d_fwd: down2 epilogue")
    ep.down2 = 0
    assert lib.climsr_conv2d_fwd_kernel(d, 1, ep) == b"conv_wr_kernel<0>"
    ep.down2 = 2
    assert lib.climsr_conv2d_fwd_kernel(d, 1, ep) == WR_POOL.encode()
