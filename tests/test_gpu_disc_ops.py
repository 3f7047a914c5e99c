"""Direct tests of the small discriminator / perceptual-loss kernels of csrc/disc.hip against float64 torch.

The whole-network tests (test_gpu_gan.py, test_gpu_plain_d.py, the golden steps) run these kernels at one
architecture-fixed shape each and with tolerances sized for a bf16 network.  Here every kernel is called on its own
through its ops.py wrapper, on operands drawn from a seeded generator and rounded to the kernel's input type first;
the reference is plain torch in float64 on those same rounded operands.  Four comparison rules, all from the
arithmetic and none from the kernels' output:

* copies and selects (reflect pad forward, maxpool2, f32_to_bf16, the transposed copies, du0 / du0_t) are
  bit-identical, compared as int16 views: f2bf is the hardware round-to-nearest-even conversion, as is
  ``Tensor.to(torch.bfloat16)``;
* fp32 results of short sums (pool backward, reflect-pad backward, the d_head sums): ``close(got, want64, 1e-5)``,
  the maximum absolute error against the reference's maximum magnitude (test_gpu_bench_shapes.close);
* bf16 results of an fp32 computation (pool forward): inputs in [0.5, 1.5] (no cancellation),
  ``|got - want64| <= 2^-8 |want64|`` per element = one bf16 ulp (half an ulp of the final rounding, plus an fp32
  accumulation over at most 9 terms, far below the other half); windows of 1, 2 or 4 inputs that are multiples of
  2^-4 are exact;
* l1_loss_bf16: relative error <= 2^-22 (each difference rounded once to fp32, fp64 partials, one final rounding).

Output regions a kernel must not touch are pre-filled with a sentinel and must keep it; regions it must zero are
pre-filled with a non-zero sentinel.  The pool tests ask climsr_adaptive_pool_kernel which route the launcher takes
and assert it by name for every case."""
import pytest
import torch
import torch.nn.functional as F

from climsr_amd import _lib, ops
from climsr_amd._lib import ClimsrError

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 0x7B7B  # bf16 bit pattern of the sentinel (a large finite number no test value rounds to)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


def sentinel_bf16(shape):
    return torch.full(shape, SENT, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def close(got, want, rel=1e-5, what=""):
    """test_gpu_bench_shapes.close: max absolute error against the reference's max magnitude."""
    scale = float(want.abs().max()) + 1e-30
    err = float((got.double().cpu() - want.double()).abs().max())
    assert err <= rel * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.2e})"


def refused(call):
    """The wrapper raises on the C ABI's CLIMSR_EINVAL (-1)."""
    with pytest.raises(ClimsrError, match=r"rc=-1"):
        call()


# --------------------------------------------------------------------------------------------------------------
# adaptive average pool
# --------------------------------------------------------------------------------------------------------------
FT, FE = "adaptive_pool_fwd_tile_kernel", "adaptive_pool_fwd_kernel"
BT, BE = "adaptive_pool_bwd_tile_kernel", "adaptive_pool_bwd_kernel"
POOL_CASES = [
    # h, w, oh, ow, c, forward route, backward route
    (16, 16, 14, 14, 64, FT, BT),   # the RFB discriminator's shrink
    (4, 4, 4, 4, 64, FT, BT),       # the plain discriminator's identity pool
    (8, 8, 14, 14, 64, FT, BT),     # growing: an input row sits in up to 3 windows (AP_MAXC)
    (7, 5, 3, 3, 128, FT, BT),      # non-square, overlapping windows, 9 outputs over AP_SPLIT = 4, two channel blocks
    (5, 5, 10, 10, 64, FT, BT),     # oh == 2h: the bound of the tiled backward
    (5, 5, 11, 11, 64, FT, BE),     # just past it
    (3, 6, 2, 4, 64, FT, BE),       # h < AP_SPLIT
    (16, 16, 14, 14, 24, FE, BE),   # c % 64 != 0
    (23, 23, 14, 14, 64, FE, BT),   # h * w > 511: the staged input does not fit the forward's LDS tile
]
POOL_IDS = ["%dx%d-%dx%d-c%d" % c[:5] for c in POOL_CASES]


def pool_route(h, w, c, oh, ow, bwd):
    return _lib.load().climsr_adaptive_pool_kernel(h, w, c, oh, ow, bwd).decode()


def pool_ref(x_nhwc, oh, ow):
    """float64 AdaptiveAvgPool2d + flatten(1) from NCHW, and the leaf to differentiate."""
    x = x_nhwc.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    return x, F.adaptive_avg_pool2d(x, (oh, ow)).flatten(1)


def window_counts(h, w, oh, ow, c):
    """Elements per output window, in the flattened [c*oh*ow] order."""
    ky = torch.tensor([-((-(i + 1) * h) // oh) - (i * h) // oh for i in range(oh)])
    kx = torch.tensor([-((-(j + 1) * w) // ow) - (j * w) // ow for j in range(ow)])
    return (ky[:, None] * kx[None, :]).flatten().repeat(c)


def run_pool_fwd(x, n, h, w, c, oh, ow, n_pad, fill):
    """(out, out_t) of the wrapper; out_t starts from the sentinel (fill=True), zeros (False) or is absent (None)."""
    out = sentinel_bf16((n, c * oh * ow))
    out_t = None if fill is None else (sentinel_bf16((c * oh * ow, n_pad)) if fill else
                                      torch.zeros((c * oh * ow, n_pad), dtype=torch.bfloat16, device=DEV))
    ops.adaptive_pool_fwd(x.to(DEV), n, h, w, c, oh, ow, out, out_t, n_pad)
    torch.cuda.synchronize()
    return out, out_t


def check_pool_fwd(h, w, oh, ow, c, froute, n, n_pad, seed):
    """Forward and transposed copy.  The fallback kernel writes only the real columns of out_t: its callers hand it a
    zero-filled buffer, and the padding columns of that buffer must still be zero afterwards (the fc.0 weight gradient
    sums over all n_pad columns).  The tiled route's transpose writes the padding columns itself, so there a
    sentinel-filled buffer must come back with zero padding."""
    assert pool_route(h, w, c, oh, ow, 0) == froute
    tiled = froute == FT
    x = (torch.rand((n, h, w, c), generator=gen(seed)) + 0.5).to(torch.bfloat16)
    _, want = pool_ref(x, oh, ow)
    want = want.detach()
    out, out_t = run_pool_fwd(x, n, h, w, c, oh, ow, n_pad, fill=tiled)
    got = out.double().cpu()
    err = (got - want).abs()
    assert bool((err <= 2.0 ** -8 * want.abs()).all()), f"max rel err {float((err / want.abs()).max()):.3e} > 2^-8"
    assert torch.equal(bits(out_t[:, :n]), bits(out.t())), "out_t real columns != out.T"
    assert int(bits(out_t[:, n:]).abs().max()) == 0, "out_t padding columns not zero"
    out2, _ = run_pool_fwd(x, n, h, w, c, oh, ow, n_pad, fill=None)  # without the transposed copy
    assert torch.equal(bits(out2), bits(out))
    # windows of 1, 2 or 4 multiples of 2^-4: every fp32 sum, the division and the bf16 rounding are exact
    xe = (torch.randint(8, 25, (n, h, w, c), generator=gen(seed + 1)).float() / 16).to(torch.bfloat16)
    _, wante = pool_ref(xe, oh, ow)
    oute, _ = run_pool_fwd(xe, n, h, w, c, oh, ow, n_pad, fill=None)
    cnt = window_counts(h, w, oh, ow, c)
    exact = (cnt == 1) | (cnt == 2) | (cnt == 4)
    assert torch.equal(oute.double().cpu()[:, exact], wante.detach()[:, exact])


def check_pool_bwd(h, w, oh, ow, c, broute, n, seed):
    assert pool_route(h, w, c, oh, ow, 1) == broute
    dp = torch.randn((n, c * oh * ow), generator=gen(seed))
    x, y = pool_ref(torch.zeros((n, h, w, c)), oh, ow)
    y.backward(dp.double())
    want = x.grad.permute(0, 2, 3, 1).contiguous()
    dx = torch.full((n, h, w, c), float("nan"), dtype=torch.float32, device=DEV)  # every element is overwritten
    ops.adaptive_pool_bwd(dp.to(DEV), n, h, w, c, oh, ow, dx)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dx).all()), "pool backward left elements unwritten"
    close(dx, want, what="pool backward")


@pytest.mark.parametrize("h,w,oh,ow,c,froute,broute", POOL_CASES, ids=POOL_IDS)
def test_adaptive_pool_fwd(h, w, oh, ow, c, froute, broute):
    check_pool_fwd(h, w, oh, ow, c, froute, n=3, n_pad=32, seed=10)


@pytest.mark.parametrize("h,w,oh,ow,c,froute,broute", POOL_CASES, ids=POOL_IDS)
def test_adaptive_pool_bwd(h, w, oh, ow, c, froute, broute):
    check_pool_bwd(h, w, oh, ow, c, broute, n=3, seed=20)


@pytest.mark.parametrize("case", [POOL_CASES[3], POOL_CASES[7]], ids=[POOL_IDS[3], POOL_IDS[7]])
def test_adaptive_pool_two_batch_tiles(case):
    """n = 33 in n_pad = 64: more images than one 32-column group, a partly filled transpose tile."""
    h, w, oh, ow, c, froute, broute = case
    check_pool_fwd(h, w, oh, ow, c, froute, n=33, n_pad=64, seed=30)
    check_pool_bwd(h, w, oh, ow, c, broute, n=33, seed=31)


def test_adaptive_pool_routes_cover_both_kernels():
    """Each of the four kernels is reached by at least two of the cases above."""
    for name, col in ((FT, 5), (FE, 5), (BT, 6), (BE, 6)):
        assert sum(1 for case in POOL_CASES if case[col] == name) >= 2, name


def test_adaptive_pool_refuses_short_padding():
    x = torch.zeros((3, 4, 4, 64), dtype=torch.bfloat16, device=DEV)
    out, out_t = sentinel_bf16((3, 64 * 16)), sentinel_bf16((64 * 16, 2))
    refused(lambda: ops.adaptive_pool_fwd(x, 3, 4, 4, 64, 4, 4, out, out_t, 2))  # n_pad < n
    torch.cuda.synchronize()
    assert bool((bits(out) == SENT).all()) and bool((bits(out_t) == SENT).all())


# --------------------------------------------------------------------------------------------------------------
# discriminator head
# --------------------------------------------------------------------------------------------------------------
def f32(x):
    return x.to(torch.float32)


@pytest.mark.parametrize("n,n_pad", [(1, 32), (5, 32), (32, 32), (33, 64)])
@pytest.mark.parametrize("o", [96, 256, 1000])
def test_d_head_fwd_bwd(o, n, n_pad):
    """s = sigmoid?(h . w2 + b2) and its backward, h = the LeakyReLU output of fc.0 (lrelu' from the sign of h)."""
    g = gen(100 + o + n)
    h = torch.randn((n, o), generator=g)
    h[0, : min(o, 7)] = 0.0  # exact zeros take the negative branch (the kernel tests h > 0)
    w2 = torch.randn((o,), generator=g) / o ** 0.5
    b2 = torch.randn((1,), generator=g)
    ds = torch.randn((n,), generator=g)
    pre = {k: torch.randn(shape, generator=g) for k, shape in (("dw2", (o,)), ("db2", (1,)), ("db0", (o,)))}
    hd, w2d, b2d, dsd = h.to(DEV), w2.to(DEV), b2.to(DEV), ds.to(DEV)
    for sigmoid in (0, 1):
        h64 = h.double().requires_grad_(True)
        w64 = w2.double().requires_grad_(True)
        b64 = b2.double().requires_grad_(True)
        u = h64 @ w64 + b64
        s64 = torch.sigmoid(u) if sigmoid else u
        s64.backward(ds.double())
        s = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
        ops.d_head_fwd(hd, w2d, b2d, n, o, s, sigmoid=bool(sigmoid))
        torch.cuda.synchronize()
        close(s, s64.detach(), what=f"d_head_fwd sigmoid={sigmoid}")
        s_in = f32(s64.detach())  # the backward's operand: the reference score rounded to fp32
        for slope in (0.2, 1.0):
            sl32 = float(torch.tensor(slope, dtype=torch.float32))
            lr = torch.where(h > 0, 1.0, sl32)
            du0_64 = h64.grad * lr.double()
            # the kernel's fp32 expression, operation by operation: du = ds*s*(1-s); v = du*w2*lrelu'
            du = (ds * s_in) * (1.0 - s_in) if sigmoid else ds
            v32 = (du[:, None] * w2[None, :]) * lr
            want_bits = bits(v32.to(torch.bfloat16))
            for accumulate in (0, 1):
                for with_grads in ((True, False) if (sigmoid, slope, accumulate) == (1, 0.2, 0) else (True,)):
                    dw2, db2, db0 = (pre[k].clone().to(DEV) if with_grads else None for k in ("dw2", "db2", "db0"))
                    du0, du0_t = sentinel_bf16((n, o)), sentinel_bf16((o, n_pad))
                    ops.d_head_bwd(hd, s_in.to(DEV), dsd, w2d, n, o, n_pad, dw2, db2, db0, bool(accumulate), du0, du0_t,
                                   slope=slope, sigmoid=bool(sigmoid))
                    torch.cuda.synchronize()
                    tag = f"o={o} n={n} sigmoid={sigmoid} slope={slope} acc={accumulate}"
                    assert torch.equal(bits(du0), want_bits), "du0 " + tag
                    assert torch.equal(bits(du0_t[:, :n]), want_bits.t()), "du0_t " + tag
                    assert int(bits(du0_t[:, n:]).abs().max()) == 0 if n_pad > n else True, "du0_t padding " + tag
                    if not with_grads:
                        continue
                    base = {k: (pre[k].double() if accumulate else 0.0) for k in pre}
                    close(dw2, base["dw2"] + w64.grad, what="dw2 " + tag)
                    close(db2, base["db2"] + b64.grad, what="db2 " + tag)
                    close(db0, base["db0"] + du0_64.sum(0), what="db0 " + tag)


def test_d_head_bwd_argument_checks():
    n, o = 5, 96
    h = torch.zeros((n, o), device=DEV)
    s = torch.zeros((n,), device=DEV)
    w2 = torch.zeros((o,), device=DEV)
    for n_pad in (40, 4):  # not a multiple of 32; smaller than n (and not a multiple either)
        dw2 = torch.full((o,), 3.0, device=DEV)
        db2 = torch.full((1,), 3.0, device=DEV)
        db0 = torch.full((o,), 3.0, device=DEV)
        du0, du0_t = sentinel_bf16((n, o)), sentinel_bf16((o, 64))
        refused(lambda: ops.d_head_bwd(h, s, s, w2, n, o, n_pad, dw2, db2, db0, False, du0, du0_t))
        torch.cuda.synchronize()
        assert bool((bits(du0) == SENT).all()) and bool((bits(du0_t) == SENT).all())
        assert bool((dw2 == 3.0).all()) and bool((db2 == 3.0).all()) and bool((db0 == 3.0).all())
    du0, du0_t = sentinel_bf16((33, o)), sentinel_bf16((o, 64))
    h33 = torch.zeros((33, o), device=DEV)
    s33 = torch.zeros((33,), device=DEV)
    refused(lambda: ops.d_head_bwd(h33, s33, s33, w2, 33, o, 32, None, None, None, False, du0, du0_t))  # n_pad < n
    torch.cuda.synchronize()
    assert bool((bits(du0) == SENT).all()) and bool((bits(du0_t) == SENT).all())


# --------------------------------------------------------------------------------------------------------------
# reflection pad
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [8, 64])
@pytest.mark.parametrize("h,w", [(2, 2), (3, 3), (3, 7), (8, 5)])
def test_reflect_pad1_fwd(h, w, cs):
    n = 2
    x = torch.randn((n, h, w, cs), generator=gen(200 + h * w + cs)).to(torch.bfloat16)
    y = sentinel_bf16((n, h + 2, w + 2, cs))
    ops.reflect_pad1(x.to(DEV), n, h, w, cs, y)
    torch.cuda.synchronize()
    want = F.pad(x.float().permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect").permute(0, 2, 3, 1).to(torch.bfloat16)
    assert torch.equal(bits(y), bits(want))


@pytest.mark.parametrize("c", [1, 8, 3])
@pytest.mark.parametrize("h,w", [(3, 3), (3, 7), (4, 4), (8, 5)])
def test_reflect_pad1_bwd(h, w, c):
    """h == 3: the two mirrors (y == 1, y == h - 2) fall on the same row, which then folds three padded rows."""
    n = 2
    gp = torch.randn((n, h + 2, w + 2, c), generator=gen(300 + h * w + c))
    x = torch.zeros((n, c, h, w), dtype=torch.float64, requires_grad=True)
    F.pad(x, (1, 1, 1, 1), mode="reflect").backward(gp.double().permute(0, 3, 1, 2))
    want = x.grad.permute(0, 2, 3, 1).contiguous()
    g = torch.full((n, h, w, c), float("nan"), dtype=torch.float32, device=DEV)
    ops.reflect_pad1_bwd(gp.to(DEV), n, h, w, c, g)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(g).all())
    close(g, want, what="reflect pad backward")


def test_reflect_pad1_bwd_refuses_two_rows():
    gp = torch.zeros((2, 4, 6, 8), device=DEV)
    g = torch.full((2, 2, 4, 8), 3.0, device=DEV)
    refused(lambda: ops.reflect_pad1_bwd(gp, 2, 2, 4, 8, g))
    torch.cuda.synchronize()
    assert bool((g == 3.0).all())


# --------------------------------------------------------------------------------------------------------------
# VGG helpers: maxpool, bf16 L1, fp32 -> bf16
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,c", [(2, 2, 8), (6, 4, 24), (8, 8, 64)])
def test_maxpool2(h, w, c):
    """Negative values, ties inside a window and -0 / +0 pairs (either zero is a correct maximum: float compare)."""
    n = 2
    g = gen(400 + h + c)
    x = torch.randint(-4, 3, (n, h, w, c), generator=g).float() * 0.5  # few distinct values: many equal neighbours
    x[x == 0] = torch.where(torch.rand(x.shape, generator=g) < 0.5, 0.0, -0.0)[x == 0]
    x[0, 0, 0, :] = -0.0
    x[0, 0, 1, :] = 0.0  # a window whose maximum is a +0 / -0 pair
    x[0, 1, :2, :] = -1.0
    x = x.to(torch.bfloat16)
    y = sentinel_bf16((n, h // 2, w // 2, c))
    ops.maxpool2(x.to(DEV), n, h, w, c, y)
    torch.cuda.synchronize()
    want = F.max_pool2d(x.float().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    assert torch.equal(y.float().cpu(), want)


@pytest.mark.parametrize("h,w,c", [(3, 4, 8), (4, 3, 8), (4, 4, 12)])
def test_maxpool2_refuses(h, w, c):
    x = torch.zeros((2, h, w, c), dtype=torch.bfloat16, device=DEV)
    y = sentinel_bf16((2, h // 2 + 1, w // 2 + 1, c + 8))
    refused(lambda: ops.maxpool2(x, 2, h, w, c, y))
    torch.cuda.synchronize()
    assert bool((bits(y) == SENT).all())


@pytest.mark.parametrize("n", [8, 2048, 8 * (512 * 256) + 8, 1_000_000 - 1_000_000 % 8])
def test_l1_loss_bf16(n):
    """One vector; fewer vectors than the 512 blocks (most partials empty); one more than a grid pass; many passes.
    The workspace starts as NaN: every partial the final pass reads must have been written."""
    g = gen(500 + n % 97)
    a = torch.randn((n,), generator=g).to(torch.bfloat16)
    b = torch.randn((n,), generator=g).to(torch.bfloat16)
    ws = torch.full((512,), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.full((1,), float("nan"), dtype=torch.float32, device=DEV)
    ops.l1_bf16(a.to(DEV), b.to(DEV), n, ws, out)
    torch.cuda.synchronize()
    want = float((a.double() - b.double()).abs().mean())
    got = float(out.double().cpu())
    assert abs(got - want) <= 2.0 ** -22 * want, f"rel err {abs(got - want) / want:.3e}"


def test_l1_loss_bf16_refuses_ragged_length():
    a = torch.zeros((16,), dtype=torch.bfloat16, device=DEV)
    ws = torch.zeros((512,), dtype=torch.float64, device=DEV)
    out = torch.full((1,), 3.0, device=DEV)
    refused(lambda: ops.l1_bf16(a, a, 12, ws, out))
    torch.cuda.synchronize()
    assert float(out) == 3.0


def rounding_edges():
    """fp32 values whose bf16 rounding is decided by the rule: ties to even in both directions, +-0, a carry into
    the next binade, +-inf (no NaN, no fp32 denormals)."""
    inf = float("inf")
    return torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 0.0, -0.0,
                         2 - 2.0 ** -10, -(2 - 2.0 ** -10), inf, -inf, 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -8 - 2.0 ** -20],
                        dtype=torch.float32)


def with_edges(x):
    """x (flat fp32) with the rounding edge values at its head and, reversed, at its tail."""
    e = rounding_edges()
    k = min(len(e), x.numel())
    x[:k] = e[:k]
    if x.numel() >= 2 * len(e):
        x[-len(e):] = e.flip(0)
    return x


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 2055])
def test_f32_to_bf16(n):
    """Whole 8-element vectors, the scalar tail, and nothing written past the end."""
    x = with_edges(torch.randn((max(n, 1),), generator=gen(600 + n)))[:n].contiguous()
    buf = sentinel_bf16((n + 16,))
    if n:
        ops.f32_to_bf16(x.to(DEV), buf)
    else:  # an empty torch tensor has no address: n = 0 straight through the C ABI, with valid pointers
        src = torch.zeros((8,), device=DEV)
        assert _lib.load().climsr_f32_to_bf16(src.data_ptr(), 0, buf.data_ptr(), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(buf[:n]), bits(x.to(torch.bfloat16)))
    assert bool((bits(buf[n:]) == SENT).all()), "wrote past the end"
