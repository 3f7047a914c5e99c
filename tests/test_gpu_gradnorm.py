"""The gradient-norm kernels against torch on the GPU: the segmented fp64 norm (``climsr_grad_norm``) with segments of
every awkward size around the work-item chunk and a base moved off every vector alignment, its clip coefficient and
finite flag, the in-place scale, and the scaled AdamW's bit-identity with the plain one on a pre-multiplied gradient.

Tolerances: fp64 sums of n <= 2^20 addends taken in another order differ by at most n * 2^-53 ~ 1.2e-10 relative; the
L2 norms are held to 1e-9.  Maxima (inf kind), the scale and the AdamW comparisons are exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCALES = (1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2, 1e3)
ZERO_SEG = 7  # the 257-element segment is all zeros


@pytest.fixture(scope="module")
def lib():
    from climsr_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def chunk(lib):
    return lib.climsr_grad_norm_chunk()


def seg_sizes(c):
    big = 3 * c + 5
    sizes = [1, 1, 3, 63, 64, 65, 255, 257, 1, c - 1, c, c + 1, big, 2]
    if sum(sizes) >= 2 ** 20:
        sizes[12] = 2 * c + 5
    assert sum(sizes) < 2 ** 20
    return sizes


@pytest.fixture(scope="module")
def data(chunk):
    """One CPU fp32 buffer: segment k holds randn * SCALES[k % 7] (a sum credited to the wrong segment shows up)."""
    sizes = seg_sizes(chunk)
    g = torch.Generator().manual_seed(1234)
    parts = [torch.randn(n, generator=g) * SCALES[k % len(SCALES)] for k, n in enumerate(sizes)]
    parts[ZERO_SEG].zero_()
    return sizes, torch.cat(parts).float()


def offsets(sizes):
    return [0] + list(np.cumsum(sizes))


def reference(buf, sizes):
    """(L2 norms, inf norms) per segment and total, torch fp64 on the CPU."""
    segs = torch.split(buf.double(), sizes)
    l2 = [float(s.pow(2).sum().sqrt()) for s in segs] + [float(buf.double().pow(2).sum().sqrt())]
    inf = [float(s.abs().max()) for s in segs] + [float(buf.double().abs().max())]
    return np.array(l2), np.array(inf)


def run_norm(lib, g, sizes, kind, max_norm=0.0):
    assert g.is_cuda and g.dtype == torch.float32 and g.numel() == sum(sizes)
    nseg = len(sizes)
    seg = torch.tensor(offsets(sizes), dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.climsr_grad_norm_workspace(g.numel(), nseg), dtype=torch.uint8, device=DEV)
    norms = torch.full((nseg + 1,), -7.0, dtype=torch.float64, device=DEV)
    clip = torch.full((2,), -7.0, dtype=torch.float32, device=DEV)
    rc = lib.climsr_grad_norm(g.data_ptr(), g.numel(), seg.data_ptr(), nseg, kind, float(max_norm), ws.data_ptr(),
                              norms.data_ptr(), clip.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.climsr_last_error()
    torch.cuda.synchronize()
    return norms.cpu().numpy(), clip.cpu().numpy()


def check_against_reference(lib, g_dev, buf_cpu, sizes):
    l2, inf = reference(buf_cpu, sizes)
    got2, clip2 = run_norm(lib, g_dev, sizes, 0)
    rel = np.abs(got2 - l2) / np.maximum(l2, 1e-300)
    print("L2 worst relative error", rel.max(), "segments", len(sizes))
    assert (rel <= 1e-9).all(), (rel, got2, l2)
    goti, clipi = run_norm(lib, g_dev, sizes, 1)
    assert np.array_equal(goti, inf), (goti, inf)
    for clip in (clip2, clipi):
        assert clip[0] == np.float32(1.0) and clip[1] == np.float32(1.0)
    return got2, goti


def test_segmented_norm_fresh_allocation(lib, data):
    sizes, buf = data
    g = buf.to(DEV)
    assert g.data_ptr() % 16 == 0
    got2, goti = check_against_reference(lib, g, buf, sizes)
    assert got2[ZERO_SEG] == 0.0 and goti[ZERO_SEG] == 0.0


def test_segmented_norm_base_off_every_vector_alignment(lib, data):
    """The same allocation seen through buf[1:], the segments re-derived (the first 1-element segment is gone): every
    segment now starts 4 bytes later relative to the 16-byte grid."""
    sizes, buf = data
    g = buf.to(DEV)[1:]
    assert g.data_ptr() % 16 == 4
    got2, goti = check_against_reference(lib, g, buf[1:], sizes[1:])
    assert got2[ZERO_SEG - 1] == 0.0 and goti[ZERO_SEG - 1] == 0.0
    # and the whole layout shifted by one element into a larger allocation (all 14 segments, odd base)
    big = torch.empty(buf.numel() + 1, dtype=torch.float32, device=DEV)
    big[1:].copy_(buf)
    check_against_reference(lib, big[1:], buf, sizes)


def test_single_element_single_segment(lib):
    g = torch.tensor([-3.25], dtype=torch.float32, device=DEV)
    for kind in (0, 1):
        norms, clip = run_norm(lib, g, [1], kind, max_norm=1.0)
        assert norms.tolist() == [3.25, 3.25]
        assert abs(float(clip[0]) - np.float32(1.0 / (3.25 + 1e-6))) <= np.spacing(np.float32(1.0 / 3.25)) and clip[1] == 1.0


def test_rerun_is_bit_identical(lib, data):
    sizes, buf = data
    g = buf.to(DEV)
    for kind in (0, 1):
        a = run_norm(lib, g, sizes, kind, max_norm=0.5)
        b = run_norm(lib, g, sizes, kind, max_norm=0.5)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_clip_coefficient(lib, data):
    sizes, buf = data
    g = buf.to(DEV)
    total = reference(buf, sizes)[0][-1]
    for max_norm in (total / 2, total * 2):
        _norms, clip = run_norm(lib, g, sizes, 0, max_norm=max_norm)
        want = np.float32(min(1.0, max_norm / (total + 1e-6)))
        assert abs(np.float32(clip[0]) - want) <= np.spacing(want), (clip[0], want)
        assert clip[1] == 1.0
    assert run_norm(lib, g, sizes, 0, max_norm=total * 2)[1][0] == np.float32(1.0)
    for max_norm in (0.0, -1.0):
        assert run_norm(lib, g, sizes, 0, max_norm=max_norm)[1].tolist() == [1.0, 1.0]


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_finite_flag_and_untouched_segments(lib, data, chunk, bad):
    sizes, buf = data
    hit = sizes.index(chunk + 1)
    buf = buf.clone()
    buf[offsets(sizes)[hit] + chunk // 2 + 3] = bad
    g = buf.to(DEV)
    l2, inf = reference(buf, sizes)
    others = [k for k in range(len(sizes)) if k != hit]
    for kind, want in ((0, l2), (1, inf)):
        norms, clip = run_norm(lib, g, sizes, kind, max_norm=1.0)
        assert clip[1] == 0.0, (kind, clip)
        assert not np.isfinite(norms[hit]) and not np.isfinite(norms[-1])
        assert np.isnan(norms[hit]) == np.isnan(bad) and np.isnan(norms[-1]) == np.isnan(bad)
        # torch's arithmetic on the coefficient: max_norm / (NaN + 1e-6) stays NaN, max_norm / inf is 0
        assert np.isnan(clip[0]) if np.isnan(bad) else clip[0] == 0.0
        if kind == 0:
            assert (np.abs(norms[others] - want[others]) <= 1e-9 * want[others]).all()
        else:
            assert np.array_equal(norms[others], want[others])


@pytest.mark.parametrize("n", [1, 5, 1027])
def test_scale_f32(lib, n):
    g0 = torch.randn(n + 1, generator=torch.Generator().manual_seed(n)).to(DEV)
    coef = torch.tensor([0.37, 123.0], dtype=torch.float32, device=DEV)
    for base in (0, 1):  # 16-byte aligned and not
        g = g0.clone()
        view = g[base:base + n]
        want = g0[base:base + n] * coef[0]
        assert lib.climsr_scale_f32(view.data_ptr(), n, coef.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert torch.equal(view, want)
        keep = torch.ones(n + 1, dtype=torch.bool)
        keep[base:base + n] = False
        assert torch.equal(g.cpu()[keep], g0.cpu()[keep])  # nothing outside [base, base + n) moved


def hparams(step, lr=3e-4, b1=0.93, b2=0.997, eps=1e-8, wd=1e-2):
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    return torch.tensor([lr, b1, b2, eps, wd, lr / bc1, bc2 ** 0.5, 0.0], dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("n", [1, 5, 1027, 4096])
@pytest.mark.parametrize("c", [1.0, 0.37])
def test_adamw_step_scaled_matches_plain_on_premultiplied_gradient(lib, n, c):
    gen = torch.Generator().manual_seed(100 + n)
    s = torch.cuda.current_stream().cuda_stream
    coef = torch.tensor([c], dtype=torch.float32, device=DEV)
    pa = torch.randn(n, generator=gen).to(DEV)
    pb = pa.clone()
    ma, va, mb, vb = (torch.zeros(n, device=DEV) for _ in range(4))
    for step in (1, 2, 3):
        g = (torch.randn(n, generator=gen) * 0.1).to(DEV)
        g_before = g.clone()
        pre = g * coef[0] if c != 1.0 else g  # the fp32 product, rounded by torch
        hp = hparams(step)
        assert lib.climsr_adamw_step(n, pa.data_ptr(), pre.data_ptr(), ma.data_ptr(), va.data_ptr(), hp.data_ptr(), s) == 0
        assert lib.climsr_adamw_step_scaled(n, pb.data_ptr(), g.data_ptr(), mb.data_ptr(), vb.data_ptr(), hp.data_ptr(),
                                            coef.data_ptr(), 0, 0, None, s) == 0
        torch.cuda.synchronize()
        assert torch.equal(g, g_before)
        for what, a, b in (("p", pa, pb), ("m", ma, mb), ("v", va, vb)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (what, step, (a - b).abs().max())
    assert not torch.equal(ma, torch.zeros_like(ma))


def test_adamw_step_scaled_tail_path_many_draws(lib):
    """n = 3 is all tail (the scalar loop after the 16-byte path); three elements rarely expose a rounding that differs,
    so 40 seeded draws of three steps each."""
    s = torch.cuda.current_stream().cuda_stream
    coef = torch.tensor([0.37], dtype=torch.float32, device=DEV)
    gen = torch.Generator().manual_seed(4242)
    n = 3
    for draw in range(40):
        pa = torch.randn(n, generator=gen).to(DEV)
        pb = pa.clone()
        ma, va, mb, vb = (torch.zeros(n, device=DEV) for _ in range(4))
        for step in (1, 2, 3):
            g = (torch.randn(n, generator=gen) * 0.1).to(DEV)
            pre = g * coef[0]
            hp = hparams(step)
            assert lib.climsr_adamw_step(n, pa.data_ptr(), pre.data_ptr(), ma.data_ptr(), va.data_ptr(), hp.data_ptr(), s) == 0
            assert lib.climsr_adamw_step_scaled(n, pb.data_ptr(), g.data_ptr(), mb.data_ptr(), vb.data_ptr(), hp.data_ptr(),
                                                coef.data_ptr(), 0, 0, None, s) == 0
        torch.cuda.synchronize()
        for what, a, b in (("p", pa, pb), ("m", ma, mb), ("v", va, vb)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (what, draw)


@pytest.mark.parametrize("c", [1.0, 0.37])
def test_adamw_step_scaled_mirror_window(lib, c):
    n, lo, mn = 1027, 3, 514
    gen = torch.Generator().manual_seed(77)
    s = torch.cuda.current_stream().cuda_stream
    coef = torch.tensor([c], dtype=torch.float32, device=DEV)
    pa = torch.randn(n, generator=gen).to(DEV)
    pb = pa.clone()
    ma, va, mb, vb = (torch.zeros(n, device=DEV) for _ in range(4))
    mira = torch.full((mn + 8,), 0x7fc0, dtype=torch.int16, device=DEV)  # guard words after the window
    mirb = mira.clone()
    for step in (1, 2, 3):
        g = (torch.randn(n, generator=gen) * 0.1).to(DEV)
        pre = g * coef[0]
        hp = hparams(step)
        assert lib.climsr_adamw_step_mirror(n, pa.data_ptr(), pre.data_ptr(), ma.data_ptr(), va.data_ptr(), hp.data_ptr(), lo, mn,
                                            mira.data_ptr(), s) == 0
        assert lib.climsr_adamw_step_scaled(n, pb.data_ptr(), g.data_ptr(), mb.data_ptr(), vb.data_ptr(), hp.data_ptr(),
                                            coef.data_ptr(), lo, mn, mirb.data_ptr(), s) == 0
        torch.cuda.synchronize()
        for what, a, b in (("p", pa, pb), ("m", ma, mb), ("v", va, vb)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (what, step)
        assert torch.equal(mira, mirb)
        assert torch.equal(mirb[:mn].view(torch.bfloat16), pb[lo:lo + mn].to(torch.bfloat16))
        assert (mirb[mn:] == 0x7fc0).all()
