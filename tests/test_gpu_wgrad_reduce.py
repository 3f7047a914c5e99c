"""The two reductions of the weight gradients' split partials (csrc/conv_wgrad.hip: climsr_conv2d_wgrad_reduce and
climsr_conv2d_wgrad_reduce_rows) against a NumPy float32 restatement of their summation order, bit for bit.

Slabs: part[nsplit][co_rows][kw], bpart[nsplit][co_rows].  One output element sums its nsplit partials in 8 split
groups: group sg keeps four accumulators, takes part[sp + 8u] into acc[u] (u = 0..3) for sp = sg, sg + 32, ... while
sp + 24 < nsplit, then the rest (sp, sp + 8, ...) into acc[0]; the group is (acc0 + acc1) + (acc2 + acc3); the element
is 0 + g0 + g1 + ... + g7 from left to right, added to what was there with `accumulate`.  Additions only, so there is
nothing for the compiler to contract.  Every slab position the reduction must not read (rows from out_c on, columns
from in_c_real * ks^2 on) holds NaN."""
import numpy as np
import pytest
import torch

from climsr_amd import _lib
from climsr_amd._lib import ReduceDesc, ptr

pytestmark = pytest.mark.gpu

DEV = "cuda"


def ordered_sum(p):
    """p[nsplit, ...] float32 -> the kernels' sum over axis 0, float32."""
    ns = p.shape[0]
    t = np.zeros(p.shape[1:], np.float32)
    for sg in range(8):
        acc = [np.zeros(p.shape[1:], np.float32) for _ in range(4)]
        sp = sg
        while sp + 24 < ns:
            for u in range(4):
                acc[u] = acc[u] + p[sp + 8 * u]
            sp += 32
        while sp < ns:
            acc[0] = acc[0] + p[sp]
            sp += 8
        t = t + ((acc[0] + acc[1]) + (acc[2] + acc[3]))
    return t


def slabs(seed, ns, co_rows, kw, used):
    """NaN slabs with random values (magnitudes over six decades, so the order of the sums shows) in `used`:
    (row0, rows, columns) blocks.  -> part, bpart (numpy float32)."""
    rng = np.random.default_rng(seed)
    part = np.full((ns, co_rows, kw), np.nan, np.float32)
    bpart = np.full((ns, co_rows), np.nan, np.float32)
    for r0, rows, cols in used:
        part[:, r0:r0 + rows, :cols] = (rng.standard_normal((ns, rows, cols)) * 10.0 ** rng.uniform(-3, 3, (ns, rows, cols))).astype(np.float32)
        bpart[:, r0:r0 + rows] = (rng.standard_normal((ns, rows)) * 10.0 ** rng.uniform(-3, 3, (ns, rows))).astype(np.float32)
    return part, bpart


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(got, want):
    got = got.cpu()
    assert torch.isfinite(got).all(), "a NaN position of the slabs was read"
    return torch.equal(got.view(torch.int32), torch.from_numpy(want).view(torch.int32))


def before(seed, shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def reduce_plain(part, bpart, ns, out_c, in_c_real, in_c, ks, wg, bg, accumulate):
    rc = _lib.load().climsr_conv2d_wgrad_reduce(ptr(part), ptr(bpart), ns, out_c, in_c_real, in_c, ks, ptr(wg), ptr(bg), accumulate,
                                                _lib.stream_ptr())
    assert rc == 0, _lib.load().climsr_last_error()
    torch.cuda.synchronize()


def reduce_rows(part, bpart, ns, co_rows, kw, ks, descs, max_elems, accumulate):
    arr = (ReduceDesc * len(descs))(*[ReduceDesc(ptr(w), ptr(b), r0, oc, icr, 0) for w, b, r0, oc, icr in descs])
    tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    rc = _lib.load().climsr_conv2d_wgrad_reduce_rows(ptr(part), ptr(bpart), ns, co_rows, kw, ks, ptr(tab), len(descs), max_elems,
                                                     accumulate, _lib.stream_ptr())
    assert rc == 0, _lib.load().climsr_last_error()
    torch.cuda.synchronize()


# out_c 5, in_c_real 3 of in_c 8, 3x3: co_rows 16, kw 72; 135 weights + 5 bias sums = 140 outputs, the last block ragged
OC, ICR, IC, KS, CO_ROWS, KW = 5, 3, 8, 3, 16, 72


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("ns", [1, 8, 9, 33, 57, 64])
def test_reduce(ns, accumulate, bias):
    part, bpart = slabs(ns, ns, CO_ROWS, KW, [(0, OC, ICR * KS * KS)])
    w0, b0 = before(1, (OC, ICR, KS, KS)), before(2, (OC,))
    wg, bg = dev(w0), dev(b0)
    reduce_plain(dev(part), dev(bpart) if bias else None, ns, OC, ICR, IC, KS, wg, bg if bias else None, accumulate)
    want_w = ordered_sum(part[:, :OC, :ICR * KS * KS]).reshape(w0.shape)
    want_b = ordered_sum(bpart[:, :OC])
    assert same_bits(wg, w0 + want_w if accumulate else want_w)
    assert same_bits(bg, (b0 + want_b if accumulate else want_b) if bias else b0)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("ns", [1, 9, 33])
def test_reduce_rows(ns, accumulate):
    co_rows, kw = 32, 144
    convs = [(0, 16, 16), (16, 16, 8)]  # row0, out_c, in_c_real
    part, bpart = slabs(100 + ns, ns, co_rows, kw, [(r0, oc, icr * 9) for r0, oc, icr in convs])
    w0 = [before(3 + i, (oc, icr, 3, 3)) for i, (_, oc, icr) in enumerate(convs)]
    b0 = [before(7 + i, (oc,)) for i, (_, oc, _) in enumerate(convs)]
    wg, bg = [dev(w) for w in w0], [dev(b) for b in b0]
    reduce_rows(dev(part), dev(bpart), ns, co_rows, kw, 3, [(wg[i], bg[i]) + convs[i] for i in range(2)], 16 * 16 * 9 + 16, accumulate)
    for i, (r0, oc, icr) in enumerate(convs):
        want_w = ordered_sum(part[:, r0:r0 + oc, :icr * 9]).reshape(w0[i].shape)
        want_b = ordered_sum(bpart[:, r0:r0 + oc])
        assert same_bits(wg[i], w0[i] + want_w if accumulate else want_w), f"conv {i} weights"
        assert same_bits(bg[i], b0[i] + want_b if accumulate else want_b), f"conv {i} bias"


def test_both_entries_same_partials():
    ns = 33
    part, bpart = slabs(5, ns, CO_ROWS, KW, [(0, OC, ICR * KS * KS)])
    p, b = dev(part), dev(bpart)
    wg1, bg1 = torch.zeros((OC, ICR, KS, KS), device=DEV), torch.zeros(OC, device=DEV)
    wg2, bg2 = torch.zeros_like(wg1), torch.zeros_like(bg1)
    reduce_plain(p, b, ns, OC, ICR, IC, KS, wg1, bg1, 0)
    reduce_rows(p, b, ns, CO_ROWS, KW, KS, [(wg2, bg2, 0, OC, ICR)], OC * ICR * KS * KS + OC, 0)
    assert same_bits(wg2, wg1.cpu().numpy()) and same_bits(bg2, bg1.cpu().numpy())
