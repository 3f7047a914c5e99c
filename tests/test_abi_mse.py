"""CPU checks of the MSE loss at the C ABI boundary (no GPU compute): both calls are declared, exported and bound, and
bad arguments are refused before any launch."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "climsr_hip.h")
CSRC = os.path.join(ROOT, "climate-super-resolution_amd", "csrc")
CALLS = ("climsr_mse_loss", "climsr_mse_loss_grad")


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(CSRC, "libclimsr_hip.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-C", CSRC, "-j8"], check=True, capture_output=True)
    import climsr_amd  # noqa: F401
    from climsr_amd import _lib

    return _lib.load()


def test_mse_calls_declared_exported_and_bound(lib):
    from climsr_amd import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(const float\* a, const float\* b, int64_t n," % name, txt), f"{name} not in the header"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 6, f"{name} has no ctypes signature"


def test_mse_bad_arguments_launch_nothing(lib):
    assert lib.climsr_mse_loss(None, None, 0, None, None, None) == -1
    assert b"mse_loss:" in lib.climsr_last_error()
    assert lib.climsr_mse_loss_grad(None, None, 0, None, None, None) == -1
    assert b"mse_loss_grad:" in lib.climsr_last_error()
    # valid-looking pointers with n <= 0 are refused as well (validation precedes the launch; nothing is dereferenced)
    assert lib.climsr_mse_loss(8, 8, 0, 8, 8, None) == -1
    assert lib.climsr_mse_loss_grad(8, 8, -3, None, 8, None) == -1
    assert lib.climsr_mse_loss(8, None, 4, 8, 8, None) == -1
    assert lib.climsr_mse_loss_grad(8, 8, 4, None, None, None) == -1


def test_losses_package_exports():
    from climsr_amd.losses import L1Loss, MSELoss

    assert MSELoss.__name__ == "MSELoss" and L1Loss.__name__ == "L1Loss"
