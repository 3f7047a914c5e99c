"""The epilogues whose activation kind is resolved once per launch / item instead of per accumulator element
(csrc/conv_wr.hip, the direct epilogue of csrc/conv_dma.hip, csrc/disc.hip bn_apply_kernel): every activation variant
of a kernel must produce, bit for bit, what the same kernel's fp32-output epilogue produces with the activation applied
to that fp32 value afterwards (torch fp32, then the RNE bf16 rounding) -- the MFMA order, the bias add, the select
`x > 0 ? x : x * slope` and the pack are the same instructions in every variant.  (The build before the activation
became a template argument satisfies every exact comparison here as well: none of them needed a tolerance.)

Shapes are the smallest that reach the ragged-tile and edge-tile paths: conv_wr tiles are 4 x 16 pixels (7 x 18: one
full and one 3-row tile, one full and one 2-column tile; 12 x 48: a 3 x 3 grid of tiles, so an interior tile and every
kind of border tile meet in one image), the LDS-DMA conv's are 32 x 16 (32 x 20: 16 + 4 columns), bn_apply walks
256 / (c / 8) pixel rows per pass (37 pixels: a ragged last pass for c = 64, a ragged only pass for c = 512)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from climsr_amd import ops
    from climsr_amd.ops import ACT_LRELU, ACT_NONE, ACT_RELU, OUT_BF16, OUT_F32, ConvPlan

DEV = "cuda"
# name -> (forward act, its backward act, slope)
ACTS = {"none": (0, None, 0.0), "lrelu0.2": (1, 3, 0.2), "lrelu0.01": (1, 3, 0.01), "relu": (2, 4, 0.0)}


def bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


def to_nhwc(x, cs=None, co=0):
    n, c, h, w = x.shape
    buf = torch.zeros((n, h, w, cs or c), dtype=torch.bfloat16, device=DEV)
    buf[..., co:co + c] = x.permute(0, 2, 3, 1).to(torch.bfloat16)
    return buf


def make_plan(cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    w = (torch.rand((cout, cin, 3, 3), generator=g) * 2 - 1) / (cin * 9) ** 0.5
    b = (torch.rand((cout,), generator=g) * 2 - 1) * 0.1
    p = ConvPlan(cin, cout, 3, 1, None, "t")
    p.bind(w.to(DEV).contiguous(), b.to(DEV))
    p.pack()
    return p, w, b


def run(p, route, *args, **kw):
    """p.fwd(*args, **kw) under the launch observer; the kernel name it reports must start with `route`."""
    names = []
    ops.PROFILER = lambda name, flops, fn, tag="", nbytes=0: (names.append(name), fn())
    try:
        p.fwd(*args, **kw)
    finally:
        ops.PROFILER = None
    assert names and names[-1].startswith(route), (names, route)


def act_f32(y, kind, slope):
    """The epilogue's activation on an fp32 tensor, in fp32: x > 0 ? x : x * slope (kind 1), x > 0 ? x : 0 (kind 2)."""
    if kind == 1:
        return torch.where(y > 0, y, y * torch.tensor(slope, dtype=torch.float32, device=y.device))
    if kind == 2:
        return torch.where(y > 0, y, torch.zeros_like(y))
    return y


def same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    iv = torch.int16 if got.dtype == torch.bfloat16 else torch.int32
    bad = int((got.contiguous().view(iv) != want.contiguous().view(iv)).sum())
    assert bad == 0, f"{what}: {bad} of {got.numel()} elements differ in their bits"


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("h,w,up", [(7, 18, 1), (4, 9, 2), (12, 48, 1)])
def test_conv_wr_epilogues_exact(h, w, up, act):
    """conv_wr_kernel<EP>: EP 0 (bf16), EP 3 (fp32), EP 4 (bf16 + channel sums) with each activation against EP 3
    without one; EP 2 (activation backward from the stored activation, no bias) against the no-bias fp32 output; EP 1
    (residual: its multiply-add may be contracted) against fp64 within test_conv_wr_matches_fp64's bound."""
    kind, bwd, slope = ACTS[act]
    p, wt, b = make_plan(64, 64, seed=31)
    g = torch.Generator().manual_seed(32 + h)
    x = bf(torch.rand((1, 64, h, w), generator=g) * 2 - 1)
    oh, ow = h * up, w * up
    xin = to_nhwc(x, cs=72, co=8)
    r = to_nhwc(bf(torch.rand((1, 64, oh, ow), generator=g) * 2 - 1))
    geo = (xin, 72, 8, h, w)

    def out(dtype):
        return torch.full((1, oh, ow, 64), 7.0, dtype=dtype, device=DEV)

    y32 = out(torch.float32)
    run(p, "conv_wr_kernel<3>", *geo, y32, 64, 0, 1, up=up, out_mode=OUT_F32)
    want32 = act_f32(y32, kind, slope)
    want16 = want32.to(torch.bfloat16)

    y0 = out(torch.bfloat16)
    run(p, "conv_wr_kernel<0>", *geo, y0, 64, 0, 1, up=up, act=kind, slope=slope)
    same_bits(y0, want16, f"EP 0 {act}")

    y3 = out(torch.float32)
    run(p, "conv_wr_kernel<3>", *geo, y3, 64, 0, 1, up=up, act=kind, slope=slope, out_mode=OUT_F32)
    same_bits(y3, want32, f"EP 3 {act}")

    rows = ((ow + 15) // 16) * ((oh + 3) // 4)  # one row of channel sums per 4 x 16 tile
    if up == 1:
        assert p.ch_parts(72, h, w, 1, 64) == (rows, rows)
    part = torch.full((rows, 64), 7.0, dtype=torch.float32, device=DEV)
    y4 = out(torch.bfloat16)
    run(p, "conv_wr_kernel<4>", *geo, y4, 64, 0, 1, up=up, act=kind, slope=slope, ch_part=part)
    same_bits(y4, y0, f"EP 4 {act}")
    # the sums are of the fp32 values, tile by tile in a fixed order: compare with fp64 sums of EP 3's output
    got = part.double().sum(0)
    ref = want32.double().sum((0, 1, 2))
    assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max()) + 1e-6, f"EP 4 {act}: channel sums"

    if bwd is not None:
        n32 = out(torch.float32)
        run(p, "conv_wr_kernel<3>", *geo, n32, 64, 0, 1, up=up, out_mode=OUT_F32, use_bias=False)
        rf = r.float()
        other = n32 * torch.tensor(slope, dtype=torch.float32, device=DEV) if bwd == 3 else torch.zeros_like(n32)
        y2 = out(torch.bfloat16)
        run(p, "conv_wr_kernel<2>", *geo, y2, 64, 0, 1, up=up, act=bwd, slope=slope, use_bias=False, res1=r, res1_cs=64, res1_co=0)
        same_bits(y2, torch.where(rf > 0, n32, other).to(torch.bfloat16), f"EP 2 {act}")
    else:
        y1 = out(torch.bfloat16)
        run(p, "conv_wr_kernel<1>", *geo, y1, 64, 0, 1, up=up, res1=r, res1_cs=64, res1_co=0, alpha1=0.2)
        xr = x.double()
        if up == 2:
            xr = F.interpolate(xr, scale_factor=2, mode="nearest")
        want = 0.2 * F.conv2d(xr, bf(wt).double(), b.double(), padding=1) + r.double().cpu().permute(0, 3, 1, 2)
        err = float((y1.double().cpu().permute(0, 3, 1, 2) - want).abs().max())
        assert err <= 2 ** -7 * float(want.abs().max()) + 1e-6, f"EP 1: err {err:.3e} vs {float(want.abs().max()):.3e}"
    torch.cuda.synchronize()


@pytest.mark.parametrize("act,bias", [("none", True), ("lrelu0.2", True), ("relu", True), ("lrelu0.2", False), ("relu", False)])
def test_conv_fwd_dma_direct_epilogue_exact(act, bias):
    """conv_fwd_dma_kernel's epilogue straight from the accumulators (EP 3: bias + activation, EP 6: activation only;
    without an activation the plan takes the staged EP 0) against the same plan's fp32-output run with the activation
    applied in fp32 and rounded to bf16: same kernel body, same chunk order, so bit for bit."""
    kind, _bwd, slope = ACTS[act]
    h, w = 32, 20
    p, _wt, _b = make_plan(64, 128, seed=41)
    g = torch.Generator().manual_seed(42)
    xin = to_nhwc(bf(torch.rand((1, 64, h, w), generator=g) * 2 - 1))
    y32 = torch.full((1, h, w, 128), 7.0, dtype=torch.float32, device=DEV)
    run(p, "conv_fwd_dma_kernel<", xin, 64, 0, h, w, y32, 128, 0, 1, out_mode=OUT_F32, use_bias=bias)
    y = torch.full((1, h, w, 128), 7.0, dtype=torch.bfloat16, device=DEV)
    route = "conv_fwd_dma_kernel<" + ("0" if kind == 0 else "3" if bias else "6") + ", false>"
    run(p, route, xin, 64, 0, h, w, y, 128, 0, 1, act=kind, slope=slope, out_mode=OUT_BF16, use_bias=bias)
    torch.cuda.synchronize()
    same_bits(y, act_f32(y32, kind, slope).to(torch.bfloat16), f"EP {'3' if bias else '6'} {act}")


@pytest.mark.parametrize("act", [ACT_LRELU, ACT_RELU, ACT_NONE] if torch.cuda.is_available() else [1, 2, 0])
@pytest.mark.parametrize("c", [64, 512])
@pytest.mark.parametrize("mode", ["forward", "inference"])
def test_bn_apply_ragged(mode, c, act):
    """bn_forward (batch statistics) and bn_inference (running statistics) + activation over a pixel count that is no
    multiple of the rows per workgroup, against fp64 BatchNorm + activation within the bf16 bound test_gpu_bn_fused.py
    uses (2^-7 of the scale); a rerun is bit-identical."""
    npix, eps, slope = 37, 1e-5, 0.2
    g = torch.Generator().manual_seed(50 + c)
    z = (torch.randn((npix, c), generator=g) * 1.5 + 0.3).to(torch.bfloat16).to(DEV)
    gamma = (torch.rand(c, generator=g) + 0.5).to(DEV)
    beta = (torch.rand(c, generator=g) - 0.5).to(DEV)
    rm = (torch.randn(c, generator=g) * 0.1).to(DEV)
    rv = (torch.rand(c, generator=g) + 0.5).to(DEV)
    z64 = z.double()
    outs = []
    for _ in range(2):
        y = torch.full((npix, c), 7.0, dtype=torch.bfloat16, device=DEV)
        if mode == "forward":
            mean, rstd = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
            ops.bn_forward(z, npix, c, gamma, beta, mean, rstd, y, ops.bn_workspace(npix, c, {}, torch.device(DEV)), act=act,
                           slope=slope, eps=eps)
        else:
            ops.bn_inference(z, npix, c, rm, rv, gamma, beta, y, act=act, slope=slope, eps=eps)
        outs.append(y)
    torch.cuda.synchronize()
    if mode == "forward":
        m, v = z64.mean(0), z64.var(0, unbiased=False)
    else:
        m, v = rm.double(), rv.double()
    want = (z64 - m) / torch.sqrt(v + eps) * gamma.double() + beta.double()
    want = F.leaky_relu(want, slope) if act == ACT_LRELU else F.relu(want) if act == ACT_RELU else want
    err = float((outs[0].double() - want).abs().max())
    scale = float(want.abs().max()) + 1e-30
    assert err <= 2 ** -7 * scale, f"bn {mode} c={c} act={act}: max err {err:.3e} vs scale {scale:.3e}"
    same_bits(outs[1], outs[0], "rerun")
