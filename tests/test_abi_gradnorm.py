"""CPU checks of the gradient-norm / clipping calls at the C ABI boundary (no GPU compute): the calls are declared,
exported and bound, bad arguments are refused before any launch, and the sizing helpers behave."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "climsr_hip.h")
CSRC = os.path.join(ROOT, "climate-super-resolution_amd", "csrc")
CALLS = {"climsr_grad_norm_chunk": 0, "climsr_grad_norm_workspace": 2, "climsr_grad_norm": 10, "climsr_scale_f32": 4,
         "climsr_adamw_step_scaled": 11}


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(CSRC, "libclimsr_hip.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-C", CSRC, "-j8"], check=True, capture_output=True)
    import climsr_amd  # noqa: F401
    from climsr_amd import _lib

    return _lib.load()


def test_calls_declared_exported_and_bound(lib):
    from climsr_amd import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, nargs in CALLS.items():
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, txt), f"{name} not in the header"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, f"{name} has no ctypes signature"


def test_grad_norm_bad_arguments_launch_nothing(lib):
    P = 8  # a valid-looking pointer: validation precedes the launch, nothing is dereferenced
    good = dict(g=P, n=4, seg_off=P, nseg=1, kind=0, max_norm=1.0, ws=P, norms=P, clip=P)

    def call(**kw):
        a = dict(good, **kw)
        return lib.climsr_grad_norm(a["g"], a["n"], a["seg_off"], a["nseg"], a["kind"], a["max_norm"], a["ws"], a["norms"],
                                    a["clip"], None)

    for bad in (dict(g=None), dict(seg_off=None), dict(ws=None), dict(norms=None), dict(clip=None), dict(n=0), dict(n=-5),
                dict(nseg=0), dict(nseg=-1), dict(kind=2), dict(kind=-1)):
        lib.climsr_scale_f32(None, 0, None, None)  # leaves another call's message behind
        assert call(**bad) == -1, bad
        assert lib.climsr_last_error().startswith(b"grad_norm:"), (bad, lib.climsr_last_error())


def test_scale_and_scaled_adamw_bad_arguments_launch_nothing(lib):
    P = 8
    for args in ((None, 4, P, None), (P, 4, None, None), (P, 0, P, None), (P, -1, P, None)):
        assert lib.climsr_scale_f32(*args) == -1, args
        assert lib.climsr_last_error().startswith(b"scale_f32:")
    ok = [4, P, P, P, P, P, P, 0, 0, None, None]  # n, p, g, m, v, hp, gscale, mirror_lo, mirror_n, mirror, stream
    for i, val in ((0, 0), (0, -2), (1, None), (2, None), (3, None), (4, None), (5, None), (6, None)):
        a = list(ok)
        a[i] = val
        assert lib.climsr_adamw_step_scaled(*a) == -1, (i, val)
        assert lib.climsr_last_error().startswith(b"adamw_step_scaled:")
    for lo, mn in ((-1, 2), (0, 0), (3, 2), (0, 5)):  # a mirror window outside [0, n)
        a = list(ok)
        a[7], a[8], a[9] = lo, mn, P
        assert lib.climsr_adamw_step_scaled(*a) == -1, (lo, mn)
        assert lib.climsr_last_error().startswith(b"adamw_step_scaled:")


def test_chunk_and_workspace_sizing(lib):
    c = lib.climsr_grad_norm_chunk()
    assert c > 0
    sizes = [(n, s) for n in (1, c - 1, c, c + 1, 10 * c + 3, 107_000_000) for s in (1, 2, 17, 600)]
    for n, s in sizes:
        w = lib.climsr_grad_norm_workspace(n, s)
        # room for at least one fp64 partial per work item (a segment of len elements takes ceil(len / chunk) items,
        # at most ceil(n / chunk) + nseg of them) and one fp64 value per segment
        assert w >= 8 * ((n + c - 1) // c + s) + 8 * s
        assert lib.climsr_grad_norm_workspace(n + c, s) >= w and lib.climsr_grad_norm_workspace(n + 1, s) >= w
        assert lib.climsr_grad_norm_workspace(n, s + 1) >= w
    assert lib.climsr_grad_norm_workspace(2 * c, 3) > lib.climsr_grad_norm_workspace(c, 3)
    assert lib.climsr_grad_norm_workspace(c, 4) > lib.climsr_grad_norm_workspace(c, 3)
