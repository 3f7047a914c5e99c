"""Direct tests of the torch-boundary glue kernels of csrc/elementwise.hip against float64 torch: the two layout
conversions, axpby over channel slices and the activation gradient.

The whole-network tests run them at one fixed shape each inside bf16-sized tolerances.  Here each is called through
its ops.py wrapper on seeded operands rounded to the kernel's input type, with channel slices inside wider buffers
that start from a sentinel: channels outside the slice must keep it, channels the kernel must zero (act_grad's
c_real .. dz_cstride) must lose it.  Comparison rules, from the arithmetic alone:

* nchw_to_nhwc (one fp32 -> bf16 rounding), bf16-source nhwc_to_nchw (exact widening) and act_grad with scale 1 or
  0.5 (a select and one rounding of an fp32 product) are bit-identical to torch;
* fp32 results (axpby, fp32-source nhwc_to_nchw): test_gpu_bench_shapes.close(got, want64, rel=1e-5)."""
import numpy as np
import pytest
import torch

from climsr_amd import ops
from climsr_amd._lib import ClimsrError
from climsr_amd.ops import ACT_LRELU, ACT_NONE, ACT_RELU

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 0x7B7B  # bf16 bit pattern of the sentinel
SENT32 = -12345.0  # fp32 sentinel


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu()


def sentinel_bf16(shape):
    return torch.full(shape, SENT, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def close(got, want, rel=1e-5, what=""):
    """test_gpu_bench_shapes.close: max absolute error against the reference's max magnitude."""
    scale = float(want.abs().max()) + 1e-30
    err = float((got.double().cpu() - want.double()).abs().max())
    assert err <= rel * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.2e})"


def refused(call):
    with pytest.raises(ClimsrError, match=r"rc=-1"):
        call()


def rounding_edges():
    """fp32 values whose bf16 rounding is decided by the rule: ties to even in both directions, +-0, a carry into
    the next binade, +-inf (no NaN, no fp32 denormals)."""
    inf = float("inf")
    return torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 0.0, -0.0,
                         2 - 2.0 ** -10, -(2 - 2.0 ** -10), inf, -inf, 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -8 - 2.0 ** -20],
                        dtype=torch.float32)


N, H, W = 2, 5, 7
SLICES = [(c, cs, co) for c in (1, 3, 8) for cs in (8, 16) for co in (0, 5)]
SLICE_IDS = ["c%d-cs%d-co%d" % s for s in SLICES]


@pytest.mark.parametrize("c,cs,co", SLICES, ids=SLICE_IDS)
def test_nchw_to_nhwc(c, cs, co):
    src = torch.randn((N, c, H, W), generator=gen(700 + c + cs + co))
    e = rounding_edges()
    src.view(-1)[: len(e)] = e  # channel 0 of image 0; c * H * W >= 35 > len(e)
    src.view(-1)[-len(e):] = e.flip(0)
    dst = sentinel_bf16((N, H, W, cs))
    if co + c > cs:
        refused(lambda: ops.nchw_to_nhwc(src.to(DEV), dst, cs, co))
        torch.cuda.synchronize()
        assert bool((bits(dst) == SENT).all())
        return
    ops.nchw_to_nhwc(src.to(DEV), dst, cs, co)
    torch.cuda.synchronize()
    want = torch.full((N, H, W, cs), SENT, dtype=torch.int16)
    want[..., co:co + c] = bits(src.permute(0, 2, 3, 1).to(torch.bfloat16))
    assert torch.equal(bits(dst), want)


@pytest.mark.parametrize("src_dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("c,cs,co", SLICES, ids=SLICE_IDS)
def test_nhwc_to_nchw(c, cs, co, src_dtype):
    src = torch.randn((N, H, W, cs), generator=gen(800 + c + cs + co)).to(src_dtype)
    dst = torch.full((N, c, H, W), SENT32, dtype=torch.float32, device=DEV)
    if co + c > cs:
        refused(lambda: ops.nhwc_to_nchw(src.to(DEV), N, c, H, W, cs, co, dst))
        torch.cuda.synchronize()
        assert bool((dst == SENT32).all())
        return
    ops.nhwc_to_nchw(src.to(DEV), N, c, H, W, cs, co, dst)
    torch.cuda.synchronize()
    want = src[..., co:co + c].permute(0, 3, 1, 2).contiguous()
    if src_dtype == torch.bfloat16:
        assert torch.equal(bits(dst), bits(want.float()))  # widening is exact
    else:
        close(dst, want.double(), what="nhwc_to_nchw fp32 source")


# --------------------------------------------------------------------------------------------------------------
# axpby over channel slices
# --------------------------------------------------------------------------------------------------------------
NPIX = 37
A, B = float(np.float32(0.2)), float(np.float32(-1.7))  # the scalars as the C ABI's floats carry them


def axpby_case(route):
    """(c, x_cs, x_co, y_cs, y_co, x misalignment in floats)."""
    if route == "vector":
        return 8, 16, 4, 20, 8, 0  # c, strides and offsets multiples of 4, 16-byte aligned bases
    return 3, 7, 2, 9, 2, 1  # c = 3, offsets of 2, x starting 4 bytes past a 16-byte boundary


@pytest.mark.parametrize("mode", ["axpby", "x_none", "b_zero"])
@pytest.mark.parametrize("route", ["vector", "scalar"])
def test_axpby(route, mode):
    c, xcs, xco, ycs, yco, mis = axpby_case(route)
    g = gen(900 + c)
    xbuf = torch.randn((NPIX * xcs + 4,), generator=g)
    y0 = torch.randn((NPIX, ycs), generator=g)
    a, b = A, B
    if mode == "b_zero":
        b = 0.0
        y0[:, yco:yco + c] = float("nan")  # must not be read
    xd_buf = xbuf.to(DEV)
    assert xd_buf.data_ptr() % 16 == 0
    xd = xd_buf[mis:mis + NPIX * xcs]
    assert xd.data_ptr() % 16 == 4 * mis
    x = xbuf[mis:mis + NPIX * xcs].view(NPIX, xcs)
    y = y0.clone().to(DEV)
    ops.axpby(NPIX, c, a, None if mode == "x_none" else xd, xcs, xco, b, y, ycs, yco)
    torch.cuda.synchronize()
    xs = torch.zeros((NPIX, c), dtype=torch.float64) if mode == "x_none" else x[:, xco:xco + c].double()
    want = a * xs + (b * y0[:, yco:yco + c].double() if b != 0.0 else 0.0)
    got = y.cpu()
    assert bool(torch.isfinite(got[:, yco:yco + c]).all())
    close(got[:, yco:yco + c], want, what=f"axpby {route} {mode}")
    keep = torch.ones(ycs, dtype=torch.bool)
    keep[yco:yco + c] = False
    assert torch.equal(bits(got[:, keep]), bits(y0[:, keep])), "channels outside the slice changed"


# --------------------------------------------------------------------------------------------------------------
# activation gradient
# --------------------------------------------------------------------------------------------------------------
ACT_GRAD_CASES = [
    # c_real, g_cs, g_co, y_cs, y_co, dz_cs
    (1, 5, 1, 8, 2, 8),       # scalar route: c_real % 8 != 0, channels 1..7 of dz zeroed
    (3, 5, 1, 8, 2, 8),       # scalar route, channels 3..7 zeroed
    (16, 24, 2, 16, 0, 24),   # scalar route by g_coff % 4 != 0; channels 16..23 zeroed
    (16, 32, 8, 32, 16, 24),  # vector route (the existing test's, test_gpu_conv.test_act_grad); 16..23 zeroed
]


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("act", [ACT_NONE, ACT_LRELU, ACT_RELU], ids=["none", "lrelu", "relu"])
@pytest.mark.parametrize("c_real,gcs,gco,ycs,yco,dzcs", ACT_GRAD_CASES, ids=["c1", "c3", "c16-goff2", "c16-vec"])
def test_act_grad(c_real, gcs, gco, ycs, yco, dzcs, act, scale):
    """dz = bf16(g * scale * act'(y)): scale 1 or 0.5 is exact, so one fp32 product (by slope) and one rounding.
    The derivative at y == 0 is the negative branch (the kernel tests !(y > 0))."""
    npix = 301  # an odd count, more than one 256-thread block even at one group of 8 dz channels per pixel
    gg = gen(1000 + c_real + gco)
    g = torch.randn((npix, gcs), generator=gg)
    y = torch.randn((npix, ycs), generator=gg).to(torch.bfloat16)
    y[::3] = 0.0  # exact zeros
    y[1::7] = -0.0
    dz = sentinel_bf16((npix, dzcs))
    ops.act_grad(npix, c_real, g.to(DEV), gcs, gco, y.to(DEV), ycs, yco, act, dz, dzcs, scale=scale, slope=0.2)
    torch.cuda.synchronize()
    t = g[:, gco:gco + c_real] * scale  # fp32, exact
    pos = y[:, yco:yco + c_real].float() > 0
    if act == ACT_LRELU:
        t = torch.where(pos, t, t * torch.tensor(0.2, dtype=torch.float32))
    elif act == ACT_RELU:
        t = torch.where(pos, t, torch.zeros_like(t))
    got = bits(dz)
    assert torch.equal(got[:, :c_real], bits(t.to(torch.bfloat16)))
    assert int(got[:, c_real:].abs().max()) == 0, "channels c_real .. dz_cstride not zeroed"
