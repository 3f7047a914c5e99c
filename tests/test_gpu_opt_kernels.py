"""GPU checks of the device-side schedules and the fused Adam update (csrc/elementwise.hip):

* ``climsr_opt_hparams``: every schedule kind, every step of two schedules that cross the warm-up boundary (integer and
  fractional warm-up; one run to its last step), within 1 ulp (fp32) of the float64 restatement
  (``core.optim.lr_lambda`` / ``onecycle_lr_beta1``, which tests/test_graph_steps_cpu.py holds to transformers and
  torch); the counters exact; the OneCycleLR kind bit-identical to ``climsr_adamw_hparams``.
* ``climsr_adam_step`` / ``climsr_adam_step_scaled``: three consecutive steps on n = 4*256*3 + 3 elements (vector body
  and tail) with the bf16 mirror window at an offset not divisible by 4, against a float64 restatement of
  ``torch.optim.Adam``.  The bound is twice the largest relative error of the parent's ``climsr_adamw_step`` update
  vector against the float64 AdamW restatement on the same inputs (Adam does one more rounded operation per element).
  The scaled entry is bit-identical to the plain one on a gradient pre-multiplied in fp32, and at gscale = 1.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ulps(got, want):
    return np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))


def _hp_row(lr, b1, b2, eps, wd, t):
    return np.array([lr, b1, b2, eps, wd, lr / (1 - b1 ** t), math.sqrt(1 - b2 ** t), 0.0], dtype=np.float32)


def _kinds():
    from climsr_amd.core import optim as O

    return [(O.SCHED_NONE, {}), (O.SCHED_CONSTANT, {}), (O.SCHED_CONSTANT_WARMUP, {}), (O.SCHED_LINEAR_WARMUP, {}),
            (O.SCHED_COSINE_WARMUP, dict(cycles=0.5)), (O.SCHED_COSINE_WARMUP, dict(cycles=1.5)),
            (O.SCHED_COSINE_RESTARTS_WARMUP, dict(cycles=3.0))]


@pytest.mark.parametrize("warmup,total,n_steps", [(4.0, 60.0, 20), (2.5, 20.0, 21)])
def test_opt_hparams_lambda_kinds(warmup, total, n_steps):
    from climsr_amd import _lib
    from climsr_amd.core import optim as O

    lib = _lib.load()
    lr, b1, b2, eps, wd = 1e-3, 0.9, 0.999, 1e-8, 1e-4
    for kind, kw in _kinds():
        cycles = kw.get("cycles", 0.0)
        state = torch.tensor([3.0, 0.0], dtype=torch.float64, device=DEV)  # a resumed optimizer: step count 3, last_epoch 0
        hp = torch.zeros(8, dtype=torch.float32, device=DEV)
        phases = set()
        for s in range(n_steps):
            _lib.check(lib.climsr_opt_hparams(state.data_ptr(), kind, lr, b1, b2, eps, wd, warmup, total, cycles, 0.0, 0.0, 0.0,
                                              hp.data_ptr(), _lib.stream_ptr()), "opt_hparams")
            lam = O.lr_lambda(kind, s, warmup=warmup, total=total, cycles=cycles)
            want = _hp_row(lr * lam, b1, b2, eps, wd, 3 + s + 1)
            got = hp.cpu().numpy()
            assert _ulps(got, want).max() <= 1, (kind, s, got, want)
            phases.add("warmup" if s < warmup else "decay")
            if s == 0 and kind >= O.SCHED_CONSTANT_WARMUP:
                assert got[0] == 0.0 and got[5] == 0.0  # lr = 0 at last_epoch 0: the step is still counted
        assert phases == {"warmup", "decay"}
        assert state.tolist() == [3.0 + n_steps, float(n_steps)], (kind, state.tolist())
        if n_steps > total and kind in (O.SCHED_LINEAR_WARMUP, O.SCHED_COSINE_RESTARTS_WARMUP):  # ran to the end
            assert float(hp[0]) == 0.0


@pytest.mark.parametrize("total_steps,pct_start,n_steps", [(60, 0.05, 20), (20, 0.3, 20)])
def test_opt_hparams_onecycle_is_adamw_hparams(total_steps, pct_start, n_steps):
    from climsr_amd import _lib
    from climsr_amd.core import optim as O

    lib = _lib.load()
    lr, div, fdiv, b2, eps, wd = 1e-4, 2.0, 100.0, 0.999, 1e-8, 1e-4
    sa, sb = (torch.zeros(2, dtype=torch.float64, device=DEV) for _ in range(2))
    ha, hb = (torch.zeros(8, dtype=torch.float32, device=DEV) for _ in range(2))
    for s in range(n_steps):
        _lib.check(lib.climsr_adamw_hparams(sa.data_ptr(), total_steps, lr, pct_start, div, fdiv, b2, eps, wd, ha.data_ptr(),
                                            _lib.stream_ptr()), "adamw_hparams")
        _lib.check(lib.climsr_opt_hparams(sb.data_ptr(), O.SCHED_ONECYCLE, lr, 0.9, b2, eps, wd, 0.0, float(total_steps), 0.0,
                                          pct_start, div, fdiv, hb.data_ptr(), _lib.stream_ptr()), "opt_hparams")
        assert torch.equal(ha.view(torch.int32), hb.view(torch.int32)), (s, ha, hb)
        lr_s, b1_s = O.onecycle_lr_beta1(s, total_steps, lr, pct_start, div, fdiv)
        assert _ulps(hb.cpu().numpy(), _hp_row(lr_s, b1_s, b2, eps, wd, s + 1)).max() <= 1, s
    assert torch.equal(sa, sb) and sb.tolist() == [float(n_steps), float(n_steps)]


def test_opt_hparams_and_adam_reject_bad_arguments():
    from climsr_amd import _lib

    lib = _lib.load()
    st = torch.zeros(2, dtype=torch.float64, device=DEV)
    hp = torch.full((8,), 7.0, dtype=torch.float32, device=DEV)
    good = (1e-3, 0.9, 0.999, 1e-8, 1e-4, 2.5, 20.0, 0.5, 0.0, 0.0, 0.0)
    bad = [(None, 5) + good + (hp.data_ptr(),), (st.data_ptr(), 5) + good + (None,), (st.data_ptr(), 7) + good + (hp.data_ptr(),),
           (st.data_ptr(), -1) + good + (hp.data_ptr(),), (st.data_ptr(), 5, 1e-3, 0.9, 0.999, 1e-8, 1e-4, -1.0, 20.0, 0.5, 0.0, 0.0, 0.0,
                                                           hp.data_ptr()),
           (st.data_ptr(), 0, 1e-4, 0.9, 0.999, 1e-8, 1e-4, 0.0, 1.0, 0.0, 0.05, 2.0, 100.0, hp.data_ptr()),   # total_steps < 2
           (st.data_ptr(), 0, 1e-4, 0.9, 0.999, 1e-8, 1e-4, 0.0, 20.0, 0.0, 0.05, 0.0, 100.0, hp.data_ptr())]  # div_factor 0
    for args in bad:
        assert lib.climsr_opt_hparams(*args, _lib.stream_ptr()) == -1
        assert b"opt_hparams" in lib.climsr_last_error()
    t = torch.zeros(8, dtype=torch.float32, device=DEV)
    mir = torch.zeros(8, dtype=torch.bfloat16, device=DEV)
    p = t.data_ptr()
    assert lib.climsr_adam_step(0, p, p, p, p, p, 0, 0, None, None) == -1 and b"adam_step" in lib.climsr_last_error()
    assert lib.climsr_adam_step(8, p, None, p, p, p, 0, 0, None, None) == -1
    assert lib.climsr_adam_step(8, p, p, p, p, p, 4, 8, mir.data_ptr(), None) == -1  # the mirror window leaves the buffer
    assert lib.climsr_adam_step_scaled(8, p, p, p, p, p, None, 0, 0, None, None) == -1
    assert b"adam_step_scaled" in lib.climsr_last_error()
    torch.cuda.synchronize()
    assert st.tolist() == [0.0, 0.0] and bool((hp == 7.0).all()) and bool((t == 0).all())  # nothing was launched


def test_fused_adam_vs_float64_and_scaled_bit_identity():
    from climsr_amd import _lib

    lib = _lib.load()
    n, lo = 4 * 256 * 3 + 3, 1026 + 3
    mn = n - 2 - lo  # the mirror window starts at an offset not divisible by 4, ends in the tail
    assert lo % 4 != 0 and lo + mn == n - 2
    gen = torch.Generator().manual_seed(11)
    p0 = (torch.randn(n, generator=gen) * 0.1).to(DEV)
    grads = [(torch.randn(n, generator=gen) * 0.02).to(DEV) for _ in range(3)]
    lr, b1, b2, eps, wd, c = 1e-3, 0.9, 0.999, 1e-8, 1e-4, 0.37
    s = _lib.stream_ptr()

    def run(entry, coupled_ref, check=True):
        """Three steps of ``entry`` from p0; returns the fp32 results and the worst relative error of each step's update
        vector against the float64 restatement run on the same fp32 inputs."""
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        worst = 0.0
        for t, g in enumerate(grads, 1):
            hp = torch.from_numpy(_hp_row(lr, b1, b2, eps, wd, t)).to(DEV)
            hp64 = hp.double()
            P, G, M, V = p.double(), g.double(), m.double(), v.double()  # this step's fp32 inputs, exactly
            if coupled_ref:
                G = G + hp64[4] * P
            else:
                P = P * (1 - hp64[0] * hp64[4])
            M = M + (G - M) * (1 - hp64[1])
            V = V * hp64[2] + G * G * (1 - hp64[2])
            want = P - hp64[5] * (M / (V.sqrt() / hp64[6] + hp64[3])) - p.double()
            before = p.clone()
            entry(p, g, m, v, hp)
            torch.cuda.synchronize()
            got = p.double() - before.double()
            worst = max(worst, float(((got - want).abs() / want.abs().max()).max()))
            if check:  # fp32 moments: a few roundings of 2^-24 each, relative to the largest element
                assert float((m.double() - M).abs().max()) <= 1e-6 * float(M.abs().max())
                assert float((v.double() - V).abs().max()) <= 1e-6 * float(V.abs().max())
        return (p, m, v), worst

    def adamw(p, g, m, v, hp):
        _lib.check(lib.climsr_adamw_step(n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), hp.data_ptr(), s), "adamw")

    mirror = torch.zeros(mn, dtype=torch.bfloat16, device=DEV)

    def adam(p, g, m, v, hp):
        _lib.check(lib.climsr_adam_step(n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), hp.data_ptr(), lo, mn,
                                        mirror.data_ptr(), s), "adam")

    _w, err_adamw = run(adamw, coupled_ref=False)
    (p, m, v), err_adam = run(adam, coupled_ref=True)
    print(f"update-vector max relative error: adamw {err_adamw:.3e}  adam {err_adam:.3e}  bound {2 * err_adamw:.3e}", flush=True)
    assert err_adamw > 0
    assert err_adam <= 2 * err_adamw, (err_adam, err_adamw)
    assert torch.equal(mirror.view(torch.int16), p[lo:lo + mn].to(torch.bfloat16).view(torch.int16))  # RNE, as torch's cast

    def bits(ts):
        return [t.view(torch.int32) for t in ts]

    # gscale = 1: the scaled entry is the plain one
    one = torch.ones(1, dtype=torch.float32, device=DEV)
    mir1 = torch.zeros_like(mirror)

    def adam_scaled(coef, mir):
        def entry(p, g, m, v, hp):
            _lib.check(lib.climsr_adam_step_scaled(n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), hp.data_ptr(),
                                                   coef.data_ptr(), lo, mn, mir.data_ptr() if mir is not None else None, s), "adam_scaled")
        return entry

    got1, _e = run(adam_scaled(one, mir1), coupled_ref=True)
    assert all(torch.equal(a, b) for a, b in zip(bits(got1), bits((p, m, v))))
    assert torch.equal(mir1.view(torch.int16), mirror.view(torch.int16))

    # a gradient pre-multiplied in fp32 through the plain entry == the scaled entry reading the coefficient
    coef = torch.tensor([c], dtype=torch.float32, device=DEV)
    keep = [g.clone() for g in grads]
    scaled, _e = run(adam_scaled(coef, None), coupled_ref=True, check=False)  # the reference here is unscaled
    assert all(torch.equal(a, b) for a, b in zip(grads, keep))  # g is only read
    grads[:] = [g * coef for g in keep]
    pre, _e = run(adam, coupled_ref=True)
    assert all(torch.equal(a, b) for a, b in zip(bits(scaled), bits(pre)))
