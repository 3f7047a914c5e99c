"""The native MSE loss (csrc/elementwise.hip climsr_mse_loss / climsr_mse_loss_grad, losses/mse.py) vs fp64 torch.

Bounds from the arithmetic: the forward takes differences, squares and sums in fp64 and rounds once to fp32 (2^-24
relative; bound 2^-22).  The gradient is ``gscale * 2 * (a-b) / n`` formed in fp64 from the fp32 operands and rounded
once to fp32 (2^-24 relative; bound 2^-21 |want| + 1e-12).  Lengths: 1, below a wave, below a block, a few blocks plus
a tail, and 256*1024+5 (every one of the 1024 workspace slots, more than one element per thread).  A view offset by
one element is 4-byte aligned only."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
LENGTHS = [1, 7, 255, 4096 + 3, 256 * 1024 + 5]


def _pair(n, seed, offset=0):
    g = torch.Generator().manual_seed(seed)
    a = (torch.rand(n + offset, generator=g) * 2 - 1).to(DEV)[offset:]
    b = (torch.rand(n + offset, generator=g) * 2 - 1).to(DEV)[offset:]
    if offset:
        assert a.data_ptr() % 8 == 4 and a.is_contiguous()
    return a, b


@pytest.mark.parametrize("n", LENGTHS)
def test_mse_forward_and_gradient_match_fp64(n):
    from climsr_amd.losses.mse import mse_loss

    a, b = _pair(n, seed=100 + n % 97)
    av = a.clone().requires_grad_()
    a64, b64 = a.double().cpu(), b.double().cpu()
    want = ((a64 - b64) ** 2).mean()
    want_g = 0.75 * 2.0 * (a64 - b64) / n
    loss = mse_loss(av, b)
    (loss * 0.75).backward()
    torch.cuda.synchronize()
    rel = abs(float(loss.detach().double().cpu()) - float(want)) / float(want)
    err = (av.grad.double().cpu() - want_g).abs()
    worst = float((err / (2.0 ** -21 * want_g.abs() + 1e-12)).max())
    print(f"mse n={n}: loss rel err {rel:.3e} (bound {2.0 ** -22:.3e}), worst gradient err / bound {worst:.3f}")
    assert loss.dtype == torch.float32 and loss.shape == () and av.grad.shape == a.shape
    assert rel <= 2.0 ** -22, (float(loss), float(want))
    assert worst <= 1.0, worst


@pytest.mark.parametrize("n", [7, 4096 + 3])
def test_mse_four_byte_aligned_views(n):
    """a, b and the gradient's destination reached through the C ABI at 4-byte (not 8- or 16-byte) alignment."""
    from climsr_amd import _lib
    from climsr_amd._lib import check, ptr

    a, b = _pair(n, seed=7, offset=1)
    ws = torch.empty(1024, dtype=torch.float64, device=DEV)
    out = torch.empty((), dtype=torch.float32, device=DEV)
    ga = torch.full((n + 2,), 9.0, device=DEV)
    gs = torch.tensor([0.5], device=DEV)
    L = _lib.load()
    check(L.climsr_mse_loss(ptr(a), ptr(b), n, ptr(ws), ptr(out), _lib.stream_ptr()), "mse_loss")
    check(L.climsr_mse_loss_grad(ptr(a), ptr(b), n, ptr(gs), ptr(ga[1:]), _lib.stream_ptr()), "mse_loss_grad")
    torch.cuda.synchronize()
    a64, b64 = a.double().cpu(), b.double().cpu()
    want = float(((a64 - b64) ** 2).mean())
    want_g = 0.5 * 2.0 * (a64 - b64) / n
    assert abs(float(out) - want) <= 2.0 ** -22 * want
    got = ga.double().cpu()
    assert got[0] == 9.0 and got[-1] == 9.0  # nothing written outside [1, n + 1)
    assert bool(((got[1:-1] - want_g).abs() <= 2.0 ** -21 * want_g.abs() + 1e-12).all())


def test_mse_reruns_are_bit_identical():
    from climsr_amd.losses.mse import mse_loss

    a, b = _pair(256 * 1024 + 5, seed=3)
    outs, grads = [], []
    for _ in range(2):
        av = a.clone().requires_grad_()
        loss = mse_loss(av, b)
        loss.backward()
        outs.append(loss.detach().clone())
        grads.append(av.grad.clone())
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(grads[0], grads[1])


def test_mse_module_autograd_only_for_arguments_that_need_it():
    """``MSELoss()(sr, hr)`` as the task calls it: only ``sr`` requires a gradient; with both requiring one, the target's
    is the negative."""
    from climsr_amd.losses import MSELoss

    g = torch.Generator().manual_seed(11)
    sr = (torch.rand((2, 1, 9, 13), generator=g) * 2 - 1).to(DEV).requires_grad_()
    hr = (torch.rand((2, 1, 9, 13), generator=g) * 2 - 1).to(DEV)
    names = []
    from climsr_amd import ops

    ops.PROFILER = lambda name, flops, fn, tag="", nbytes=0: (names.append(name), fn())
    try:
        loss = MSELoss()(sr, hr)
        loss.backward()
    finally:
        ops.PROFILER = None
    torch.cuda.synchronize()
    assert names == ["mse_loss", "mse_grad"], names  # one gradient launch: the target needs none
    want = torch.nn.functional.mse_loss(sr.detach().double().cpu().requires_grad_(), hr.double().cpu())
    assert abs(float(loss.detach()) - float(want)) <= 2.0 ** -22 * float(want)
    want_g = 2.0 * (sr.detach().double().cpu() - hr.double().cpu()) / sr.numel()
    assert bool(((sr.grad.double().cpu() - want_g).abs() <= 2.0 ** -21 * want_g.abs() + 1e-12).all())
    assert hr.grad is None
    sr2, hr2 = sr.detach().clone().requires_grad_(), hr.clone().requires_grad_()
    MSELoss()(sr2, hr2).backward()
    torch.cuda.synchronize()
    assert torch.equal(hr2.grad, -sr2.grad) and torch.equal(sr2.grad, sr.grad)
