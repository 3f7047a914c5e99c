"""MSE loss (mean) as a native autograd node: ``torch.nn.MSELoss`` of the SRCNN task (task.py:141).

Forward: deterministic two-pass reduction (fp64 differences, squares and partials) in libclimsr_hip;
backward: ``2 * (a-b) * g / n`` with the upstream gradient read from device memory (graph-capturable).
"""
import torch

from .. import _lib
from .._lib import ptr
from ..ops import _launch


class _MSEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a = a.contiguous().float()
        b = b.contiguous().float()
        assert a.shape == b.shape and a.is_cuda
        ws = torch.empty(1024, dtype=torch.float64, device=a.device)
        out = torch.empty((), dtype=torch.float32, device=a.device)
        _launch("mse_loss", lambda: _lib.load().climsr_mse_loss(ptr(a), ptr(b), a.numel(), ptr(ws), ptr(out), _lib.stream_ptr()),
                nbytes=8 * a.numel())
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous().float()
        ga = gb = None
        if ctx.needs_input_grad[0]:
            ga = torch.empty_like(a)
            _launch("mse_grad", lambda: _lib.load().climsr_mse_loss_grad(ptr(a), ptr(b), a.numel(), ptr(g), ptr(ga), _lib.stream_ptr()),
                    nbytes=12 * a.numel())
        if ctx.needs_input_grad[1]:
            gb = torch.empty_like(b)
            _launch("mse_grad", lambda: _lib.load().climsr_mse_loss_grad(ptr(b), ptr(a), b.numel(), ptr(g), ptr(gb), _lib.stream_ptr()),
                    nbytes=12 * b.numel())
        return ga, gb


def mse_loss(a, b):
    return _MSEFn.apply(a, b)


class MSELoss(torch.nn.Module):
    """Drop-in for torch.nn.MSELoss() (reduction='mean')."""

    def forward(self, input, target):
        return mse_loss(input, target)
