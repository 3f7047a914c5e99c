"""MaxPool2d(2, 2) in the conv epilogue (ConvPlan.fwd(pool2=True), ClimsrEpilogue.down2 == 2), bit for bit.

The reference of every case is the same ConvPlan.fwd without pool2 followed by ops.maxpool2 on the same inputs, and
the comparison is torch.equal on the raw bits: bias add, ReLU and the bf16 rounding are monotone, so the max of the
rounded values is the rounded value of the max and no tolerance exists.  Every pooled launch writes a channel slice
(offset 8) of a wider NaN-filled buffer whose other channels must stay NaN, is observed through ops.PROFILER (the
pooled kernel's name, no maxpool2 launch) and is repeated into a fresh buffer.  The shapes are the smallest that reach
a partial tile in x, a short last tile row, several tiles / items per wave / workgroup (where a wrong store count in
the hand-counted s_waitcnt would show: batch_for against the kernels' grid formulas) and every refusal."""
import pytest
import torch

from tests.test_gpu_conv import bf, make_plan
from tests.test_gpu_persistent_rounds import assert_rounds, batch_for, bits, cus, nhwc, observed, rand
from tests.test_pool_routes import DMA_POOL, REFUSED, WR_POOL, refused_kw

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from climsr_amd import ops
    from climsr_amd._lib import ClimsrError
    from climsr_amd.ops import ACT_RELU, OUT_F32

DEV = "cuda"
NAN = float("nan")
OUT_PAD, OUT_CO = 16, 8  # the pooled output: channel stride cout + 16, slice at channel 8


def nan_like(shape, dtype=torch.bfloat16):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def pooled_against_unfused(p, xin, in_cs, in_co, n, h, w, cout, name):
    """fwd(pool2=True) into a strided NaN buffer against fwd + ops.maxpool2 on the same operands; returns nothing"""
    y = nan_like((n, h, w, cout))
    ref = nan_like((n, h // 2, w // 2, cout))
    names = observed(lambda: (p.fwd(xin, in_cs, in_co, h, w, y, cout, 0, n, act=ACT_RELU),
                              ops.maxpool2(y, n, h, w, cout, ref)))
    assert len(names) == 2 and names[1] == "maxpool2" and "<5>" not in names[0] and "<11," not in names[0], names
    assert torch.isfinite(ref).all(), "the reference itself"
    out_cs = cout + OUT_PAD

    def launch():
        yp = nan_like((n, h // 2, w // 2, out_cs))
        got = observed(lambda: p.fwd(xin, in_cs, in_co, h, w, yp, out_cs, OUT_CO, n, act=ACT_RELU, pool2=True))
        assert got == [name], got  # the pooled kernel, and no maxpool2
        return yp

    yp = launch()
    guard = nan_like((1,)).expand_as(yp)
    assert torch.equal(bits(yp[..., OUT_CO:OUT_CO + cout]), bits(ref)), f"{name}: pooled bits differ from conv + maxpool2"
    assert torch.equal(bits(yp[..., :OUT_CO]), bits(guard[..., :OUT_CO])), "channels before the slice touched"
    assert torch.equal(bits(yp[..., OUT_CO + cout:]), bits(guard[..., OUT_CO + cout:])), "channels after the slice touched"
    assert torch.equal(bits(launch()), bits(yp)), "not deterministic"


# ---------------------------------------------------------------------------------------------------------------------
# conv_wr_kernel<5, 2>: 4 x 16 wave tiles.  8 x 16: one tile column; 20 x 40: 5 tile rows x 2.5 tile columns (a partial
# tile in x); 6 x 32: a short last tile row (its rows 2 / 3, the odd columns' window, are outside the image)
@pytest.mark.parametrize("n,h,w", [(2, 8, 16), (3, 20, 40), (2, 6, 32)])
def test_conv_wr_pooled(n, h, w):
    p, _w, _b = make_plan(64, 64, 3, seed=81)
    assert p.pool2_ok(72, 8, h, w, n, 64 + OUT_PAD, OUT_CO)
    xin = nhwc(bf(rand((n, 64, h, w), 82)), 72, 8)
    pooled_against_unfused(p, xin, 72, 8, n, h, w, 64, WR_POOL)


@pytest.mark.parametrize("rounds", ["mid", "many"])
def test_conv_wr_pooled_rounds(rounds):
    """Several tiles per wave: from a wave's second tile on the footprint wait counts the previous epilogue's stores."""
    h, w = 12, 24
    tiles = ((h + 3) // 4) * ((w + 15) // 16)
    # conv_wr.hip conv_wr_launch: ntiles = tiles_x * tiles_y * n; grid = min(ceil(ntiles / 4), device_cus()); a wave's
    # tiles are T = 4 block + wave, T + 4 grid, ...
    n = batch_for(tiles, 4 * cus(), rounds)
    ntiles = tiles * n
    grid = min((ntiles + 3) // 4, cus())
    if rounds == "mid":
        assert 4 * grid < ntiles < 8 * grid, (ntiles, grid)
    else:
        assert ntiles > 8 * grid and ntiles % (4 * grid) != 0, (ntiles, grid)
    p, _w, _b = make_plan(64, 64, 3, seed=83)
    xin = nhwc(bf(rand((n, 64, h, w), 84)), 72, 8)
    pooled_against_unfused(p, xin, 72, 8, n, h, w, 64, WR_POOL)


# ---------------------------------------------------------------------------------------------------------------------
# conv_fwd_dma_kernel<11, false>: 32 x 16 tiles x 64 channels.  64 -> 128 at 32 x 48: one tile row, 2 chunks;
# 128 -> 256 at 100 x 40: out_h >= 96 with a 4-row last tile row, a partial tile in x, 4 chunks, the input a
# 128-channel slice of a 192-channel buffer whose other channels are NaN
@pytest.mark.parametrize("cin,cout,n,h,w,in_cs,in_co", [(64, 128, 2, 32, 48, 64, 0), (128, 256, 2, 100, 40, 192, 32)])
def test_conv_dma_pooled(cin, cout, n, h, w, in_cs, in_co):
    p, _w, _b = make_plan(cin, cout, 3, seed=85)
    assert p.pool2_ok(in_cs, in_co, h, w, n, cout + OUT_PAD, OUT_CO)
    xin = nhwc(bf(rand((n, cin, h, w), 86)), in_cs, in_co)
    pooled_against_unfused(p, xin, in_cs, in_co, n, h, w, cout, DMA_POOL)


@pytest.mark.parametrize("rounds", ["mid", "many"])
def test_conv_dma_pooled_rounds(rounds):
    """Persistent rounds: a later item's chunk 0 is awaited with vmcnt(the previous item's store count)."""
    cin, cout, h, w = 64, 256, 32, 32
    tiles, ncob = ((w + 15) // 16) * ((h + 31) // 32), cout // 64
    # conv_dma.hip fwd_dma_launch: ncu = device_cus() / 8 * 8 (>= 8); nitem = tiles_x * tiles_y * n * ncob;
    # grid = min(nitem, ncu)
    cap = max(cus() // 8 * 8, 8)
    n = batch_for(tiles * ncob, cap, rounds)
    assert_rounds(tiles * n * ncob, cap, rounds)
    p, _w, _b = make_plan(cin, cout, 3, seed=87)
    xin = nhwc(bf(rand((n, cin, h, w), 88)), cin + 8, 8)
    pooled_against_unfused(p, xin, cin + 8, 8, n, h, w, cout, DMA_POOL)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refused_launch_writes_nothing(case):
    """tests/test_pool_routes.py's list, launched: CLIMSR_EINVAL, the query says no, the output stays NaN."""
    cin, cout, stride, h, w, kw = REFUSED[case]
    n = 2
    p, _w, _b = make_plan(cin, cout, 3, stride=stride, seed=89)
    kw = refused_kw(kw)
    oh, ow = p.out_hw(h, w)
    if "res1" in kw:
        kw["res1"] = torch.zeros((n, oh, ow, cout), dtype=torch.bfloat16, device=DEV)
    if "bn_part" in kw:
        kw["bn_part"] = nan_like((n * 64, 2, cout), torch.float64)
    f32 = kw.get("out_mode") == OUT_F32
    xin = nhwc(bf(rand((n, cin, h, w), 90)), cin, 0)
    y = nan_like((n, (oh + 1) // 2, (ow + 1) // 2, cout), torch.float32 if f32 else torch.bfloat16)
    asked = []
    ops.PROFILER = lambda name, flops, run, tag="", nbytes=0: asked.append(name)  # the query alone: nothing runs
    try:
        p.fwd(xin, cin, 0, h, w, y, cout, 0, n, pool2=True, **kw)
    finally:
        ops.PROFILER = None
    assert asked == [""], asked
    if set(kw) <= {"act", "use_bias", "out_mode"}:
        assert not p.pool2_ok(cin, 0, h, w, n, cout, **kw)
    with pytest.raises(ClimsrError, match=r"rc=-1\).*max-pool epilogue"):  # CLIMSR_EINVAL, with the epilogue's own text
        p.fwd(xin, cin, 0, h, w, y, cout, 0, n, pool2=True, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(y).all(), "a refused launch wrote to the output"
    if "bn_part" in kw:
        assert torch.isnan(kw["bn_part"]).all()


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vgg_pair():
    from climsr_amd.losses.perceptual import PerceptualLoss

    return PerceptualLoss().to(DEV), PerceptualLoss(fuse_pool=False).to(DEV)


@pytest.mark.parametrize("n,side,fused_wr,fused_dma,pools", [(2, 64, 1, 1, 2), (1, 256, 1, 3, 0)])
def test_perceptual_loss_fused_against_unfused(vgg_pair, n, side, fused_wr, fused_dma, pools):
    """N=2 at 64^2: conv3_4 (16^2) and conv4_4 (8^2) are below the LDS-DMA conv's tiles and keep conv + maxpool2 next to
    the two fused layers; N=1 at 256^2: all four pooled layers fused, no maxpool2 launch.  The loss is the same bits."""
    fused, unfused = vgg_pair
    sr, hr = rand((n, 1, side, side), 91), rand((n, 1, side, side), 92)
    out = {}
    names = observed(lambda: out.setdefault("fused", fused(sr, hr)))
    assert names.count(WR_POOL) == fused_wr and names.count(DMA_POOL) == fused_dma and names.count("maxpool2") == pools, names
    names = observed(lambda: out.setdefault("unfused", unfused(sr, hr)))
    assert names.count(WR_POOL) == 0 and names.count(DMA_POOL) == 0 and names.count("maxpool2") == 4, names
    assert torch.isfinite(out["fused"]) and float(out["fused"]) > 0
    assert torch.equal(bits(out["fused"]), bits(out["unfused"])), (float(out["fused"]), float(out["unfused"]))
    assert torch.equal(bits(fused(sr, hr)), bits(out["fused"]))
