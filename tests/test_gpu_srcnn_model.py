"""The stand-alone SRCNN generator (models/srcnn.py: pack_planes8 + csrc/srcnn.hip's two fused launches + conv1's
weight gradient) vs fp64 torch on the same bf16 operands, with the intermediates rounded to bf16 where the kernels keep
them in bf16 -- the chains of test_srcnn_tail_matches_fp64 / test_srcnn_tail_backward_matches_fp64 and their bounds
(4e-3 of max-abs for the output; 2e-3 of max-abs for every weight / bias gradient, dW1 / db1 included: they are a
fp32-accumulated GEMM over the bf16 dz1, as dW2 is over the bf16 dz2).

Shapes: (2, 33x40) = 2x2 tiles of the 32x32 kernel tile, three of them ragged, two images; (1, 5x7) = smaller than a
tile.  Chunking: n = 5 run as 2 + 2 + 1."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import climsr_ref as ref
from tests.helpers import gemm_conv, update_envelope

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(2, 33, 40), (1, 5, 7)]
KEYS = [f"conv{k}.{t}" for k in (1, 2, 3) for t in ("weight", "bias")]


def bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


def check_close(got, want, tol, what):
    scale = want.abs().max().item() + 1e-12
    err = (got.double().cpu() - want.double()).abs().max().item()
    assert err <= tol * scale + 1e-7, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def make_net(c):
    from climsr_amd.core.init import init_state, spec_from_shapes
    from climsr_amd.models.srcnn import SRCNN

    net = SRCNN(in_channels=c)
    st = init_state(spec_from_shapes({k: tuple(v.shape) for k, v in net.state_dict().items()}))
    st = {k: torch.from_numpy(np.asarray(v)).float() for k, v in st.items()}
    net.load_state_dict(st)
    return net.to(DEV), st


def make_input(n, c, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((n, c, h, w), generator=g) * 2 - 1
    gout = torch.randn((n, 1, h, w), generator=g)
    return x, gout


def chain_fp64(st, x, gout=None):
    """Output (and, with gout, the six gradients) in fp64 from the bf16-rounded input and weights, fp32 biases, with
    relu(conv1), relu(conv2), gout, dz2 and dz1 rounded to bf16 as the kernels hold them."""
    d = torch.float64
    w1, w2, w3 = (bf(st[f"conv{k}.weight"]).to(d) for k in (1, 2, 3))
    b1, b2, b3 = (st[f"conv{k}.bias"].to(d) for k in (1, 2, 3))
    xb = bf(x).to(d)
    a1b = F.relu(F.conv2d(xb, w1, b1, padding=4)).to(torch.bfloat16).to(d)
    a2b = F.relu(F.conv2d(a1b, w2, b2)).to(torch.bfloat16).to(d)
    out = F.conv2d(a2b, w3, b3, padding=2)
    if gout is None:
        return out
    gb = bf(gout).to(d)
    a2v, w3v = a2b.clone().requires_grad_(), w3.clone().requires_grad_()
    F.conv2d(a2v, w3v, b3, padding=2).backward(gb)
    dz2b = (a2v.grad * (a2b > 0)).to(torch.bfloat16).to(d)
    a1v, w2v = a1b.clone().requires_grad_(), w2.clone().requires_grad_()
    F.conv2d(a1v, w2v, b2).backward(dz2b)
    dz1b = (a1v.grad * (a1b > 0)).to(torch.bfloat16).to(d)
    w1v = w1.clone().requires_grad_()
    F.conv2d(xb, w1v, b1, padding=4).backward(dz1b)
    grads = {"conv1.weight": w1v.grad, "conv1.bias": dz1b.sum((0, 2, 3)), "conv2.weight": w2v.grad,
             "conv2.bias": dz2b.sum((0, 2, 3)), "conv3.weight": w3v.grad, "conv3.bias": gb.sum().reshape(1)}
    return out, grads


def check_grads(net, want, scale=1.0, what=""):
    for k, p in net.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, k
        check_close(p.grad / scale, want[k], 2e-3, f"{what} d {k}")


def hooked(fn):
    from climsr_amd import ops

    names = []
    ops.PROFILER = lambda name, flops, f, tag="", nbytes=0: (names.append(name), f())
    try:
        res = fn()
    finally:
        ops.PROFILER = None
    return res, names


@pytest.mark.parametrize("c", [1, 2, 3])
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_forward_matches_fp64(c, n, h, w):
    net, st = make_net(c)
    x, _ = make_input(n, c, h, w, seed=60 + c)
    xd = x.to(DEV)
    with torch.no_grad():
        out = net(xd)
        out2, names = hooked(lambda: net(xd))
    torch.cuda.synchronize()
    assert out.shape == (n, 1, h, w) and out.dtype == torch.float32
    assert names == ["pack_planes8", "srcnn_tail_kernel"], names  # one layout launch, one MFMA launch
    assert torch.equal(out, out2)
    check_close(out, chain_fp64(st, x), 4e-3, "srcnn out")


@pytest.mark.parametrize("c", [1, 2])
def test_forward_matches_reference_golden(c, golden_dir, monkeypatch):
    """The reference's own SRCNN in float64 (tests/golden/srcnn_steps.npz, fwd<c> records): the native output's relative
    L2 distance from it stays within 2x that of the oracle's torch-autocast fp16 / bf16 runs (helpers.update_envelope,
    default floor) -- the reference runs with precision 16."""
    z = np.load(os.path.join(golden_dir, "srcnn_steps.npz"))
    from climsr_amd.models.srcnn import SRCNN

    st = {k: torch.from_numpy(z[f"fwd{c}.{k}"]) for k in KEYS}
    x, want = torch.from_numpy(z[f"fwd{c}.x"]), torch.from_numpy(z[f"fwd{c}.sr"])
    net = SRCNN(in_channels=c)
    net.load_state_dict({k: v.float() for k, v in st.items()})
    net = net.to(DEV)
    with torch.no_grad():
        got = net(x.float().to(DEV))
    torch.cuda.synchronize()
    p = {"srcnn." + k: v.float().to(DEV) for k, v in st.items()}
    amps = []
    with monkeypatch.context() as mp:
        mp.setattr(ref, "_conv", gemm_conv)  # rocBLAS GEMMs (no MIOpen per-shape compiles)
        torch.backends.cuda.matmul.allow_tf32 = False
        for dt in (torch.float16, torch.bfloat16):
            with torch.no_grad(), torch.autocast("cuda", dtype=dt):
                amps.append({"sr": ref.srcnn_forward(p, x.float().to(DEV)).double().cpu()})
    bad, worst, rows = update_envelope({"sr": got.double().cpu()}, {"sr": want}, amps)
    print(f"srcnn in_channels={c} forward vs reference fp64: rel L2 {rows['sr'][0]:.3e}, autocast spread {rows['sr'][1]:.3e}")
    assert got.shape == want.shape and not bad, bad


@pytest.mark.parametrize("c", [1, 2, 3])
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_backward_matches_fp64_and_accumulates(c, n, h, w):
    from climsr_amd import _lib

    net, st = make_net(c)
    x, gout = make_input(n, c, h, w, seed=70 + c)
    xd, gd = x.to(DEV), gout.to(DEV)
    _, want = chain_fp64(st, x, gout)
    ready = []
    net.set_grad_ready_hook(ready.append)
    out = net(xd)
    _, names = hooked(lambda: out.backward(gd))
    torch.cuda.synchronize()
    d = net.engine().plans[0].wgrad_desc(n, h, w, 8, 0, 1)
    wg = _lib.load().climsr_conv2d_wgrad_kernel(ctypes.byref(d)).decode()
    # the fused backward below conv1, conv1's weight gradient + its split reduction; no data-gradient launch
    assert names == ["srcnn_bwd_kernel", wg, "wgrad reduce conv1"], names
    assert ready == [0]
    check_grads(net, want, what="first backward")
    first = {k: p.grad.clone() for k, p in net.named_parameters()}
    base = net._flat_grad.data_ptr()
    assert all(p.grad.data_ptr() == base + 4 * off for p, off, _n in net._flat_index)  # written in place, flat
    net(xd).backward(gd)  # the grads are already views of the flat buffer: accumulates
    torch.cuda.synchronize()
    assert ready == [0, 0]
    for k, p in net.named_parameters():
        check_close(p.grad, 2.0 * first[k].double().cpu(), 1e-6, f"accumulated d {k}")
    for p in net.parameters():
        p.grad = None  # optimizer.zero_grad(set_to_none=True): the next backward relinks and overwrites
    net(xd).backward(gd)
    torch.cuda.synchronize()
    assert all(torch.equal(p.grad, first[k]) for k, p in net.named_parameters())
    with pytest.raises(NotImplementedError, match="input"):
        net(xd.clone().requires_grad_()).backward(gd)


def test_gradients_through_autograd_route():
    """The route torch DDP's reducer needs (core/flat.py): the same gradients, handed to autograd instead of written
    into the flat buffer; a grad-ready hook (the flat-buffer reducer) excludes it."""
    n, c, h, w = 2, 3, 33, 40
    net, _ = make_net(c)
    x, gout = make_input(n, c, h, w, seed=81)
    xd, gd = x.to(DEV), gout.to(DEV)
    net(xd).backward(gd)
    want = {k: p.grad.clone() for k, p in net.named_parameters()}
    for p in net.parameters():
        p.grad = None
    net.grads_through_autograd = True
    net(xd).backward(gd)
    torch.cuda.synchronize()
    base = net._flat_grad.data_ptr()
    for (k, p), (_q, off, _n) in zip(net.named_parameters(), net._flat_index):
        assert torch.equal(p.grad, want[k]) and p.grad.data_ptr() != base + 4 * off, k
    net(xd).backward(gd)  # AccumulateGrad adds
    torch.cuda.synchronize()
    for k, p in net.named_parameters():
        check_close(p.grad, 2.0 * want[k].double().cpu(), 1e-6, f"autograd-accumulated d {k}")
    net.set_grad_ready_hook(lambda lo: None)
    with pytest.raises(RuntimeError, match="one data-parallel route"):
        net(xd).backward(gd)


def test_batch_chunking_along_n():
    n, c, h, w = 5, 3, 33, 40
    net, st = make_net(c)
    x, gout = make_input(n, c, h, w, seed=91)
    xd, gd = x.to(DEV), gout.to(DEV)
    assert net._max_pixels_per_launch == (1 << 31) // 128 - 1  # dz1: 128 B / pixel under 2 GiB
    assert net._max_pixels_forward_only == (1 << 31) // 16 - 1  # the packed input: 16 B / pixel under 2 GiB
    with torch.no_grad():
        whole = net(xd)
    net._max_pixels_per_launch = 2 * h * w
    assert net.engine().chunks(n, h * w, net._max_pixels_per_launch) == [(0, 2), (2, 4), (4, 5)]
    out, names = hooked(lambda: net(xd))
    assert names == ["pack_planes8"] + ["srcnn_tail_kernel"] * 3, names
    _, names = hooked(lambda: out.backward(gd))
    assert [k for k in names if k == "srcnn_bwd_kernel"] == ["srcnn_bwd_kernel"] * 3 and len(names) == 9, names
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), whole)
    _, want = chain_fp64(st, x, gout)
    check_grads(net, want, what="chunked (overwrite)")
    net(xd).backward(gd)  # first chunk accumulates onto the existing gradients, as the later ones do
    torch.cuda.synchronize()
    check_grads(net, want, scale=2.0, what="chunked (accumulate)")
    net._max_pixels_forward_only = 2 * h * w  # the no-grad limit is its own
    with torch.no_grad():
        out2, names = hooked(lambda: net(xd))
    assert names == ["pack_planes8"] + ["srcnn_tail_kernel"] * 3 and torch.equal(out2, whole)
    net._max_pixels_per_launch = h * w - 1
    with pytest.raises(ValueError, match="one 1320-pixel image"):
        net(xd)


def test_esrgan_container_role_unchanged():
    """ESRGANGenerator still owns srcnn.conv{1,2,3} as plain parameters of ITS flat buffer: the reference's keys in the
    reference's order, the flat index in that order, and a forward."""
    from climsr_amd.models.esrgan import ESRGANGenerator

    shapes = ref.generator_shapes(in_channels=3, nb=1)
    g = ESRGANGenerator(in_channels=3, out_channels=1, nf=64, nb=1, gc=16)
    sd = g.state_dict()
    assert list(sd) == list(shapes) and all(tuple(sd[k].shape) == tuple(shapes[k]) for k in sd)
    names = {id(p): k for k, p in g.named_parameters()}
    assert [names[id(p)] for p, _o, _n in g._flat_index] == list(shapes)
    assert not hasattr(g.srcnn, "_flat_index")
    g = g.to(DEV)
    assert g._flat_intact() and [names[id(p)] for p, _o, _n in g._flat_index] == list(shapes)
    bt = {k: v.to(DEV) for k, v in ref.synthetic_batch(1, 32).items()}
    with torch.no_grad():
        sr = g(bt["lr"], bt["elevation"], bt["mask"])
    torch.cuda.synchronize()
    assert sr.shape == (1, 1, 32, 32) and bool(torch.isfinite(sr).all())
