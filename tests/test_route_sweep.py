"""Every route of the conv dispatch against the recorded answers of the library before the dispatch was rewritten.

tools/route_sweep.py walks a fixed grid of descriptors x epilogues through the dispatch's query entry points (kernel
names, refusals, partial-sum rows, weight-gradient splits and workspaces, packed sizes; nothing is launched, no device).
tests/golden/conv_routes.json is its summary from the parent library: a histogram of the kernel names and refusal
texts, and one SHA-256 per (in_c, out_c) block over every answer of the block.  A conv that changes kernel, error or
size changes its block's digest; the tool's docstring says how to find it (write both tables, diff them).
"""
import importlib.util
import json
import os

import pytest

from climsr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sweep():
    try:
        _lib.load()
    except OSError as e:  # the built library is a prerequisite of the whole CPU suite (test_abi)
        pytest.skip(f"libclimsr_hip.so not loadable: {e}")
    spec = importlib.util.spec_from_file_location("route_sweep", os.path.join(ROOT, "tools", "route_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(ROOT, "tests", "golden", "conv_routes.json")) as f:
        return mod.sweep(), json.load(f)


# every kernel name tests/test_dispatch_routes.py pins at the product's shapes
PINNED = ("conv_fwd_kernel<4, 4, false, 4, 6, 9, 1, 1>", "conv_wr_kernel<1>", "conv_wr_kernel<0>", "conv_co1m_kernel<3, 2>",
          "conv_pw_kernel<8, 2, 4, false, 2, 3, 2>", "conv_fwd_dma_kernel<3, false>", "conv_fwd_kernel<4, 4, false, 4, 6, 9, 3, 1>",
          "conv_fwd_s2_dma_kernel<true>", "conv_fwd_s2_dma_kernel<false>", "conv_fwd_dma_kernel<9, false>",
          "conv_wgrad64_glds_kernel", "conv_wgrad64_kernel<2, 1>", "conv_wgrad64_kernel<1, 2>")


@pytest.mark.parametrize("which", ["library", "fixture"])
def test_grid_reaches_the_dispatch(sweep, which):
    """The grid is wide enough to mean something, in what the library answers and in what was recorded: the kernel names
    of every family, every name test_dispatch_routes.py pins, each weight-gradient kind and each refusal
    climsr_conv2d_fwd can give."""
    have = sweep[0 if which == "library" else 1]
    fwd = [n for n in have["names"] if "wgrad" not in n]
    assert len(fwd) >= 145
    for family in ("conv_co1m_kernel", "conv_co1_kernel", "conv_n16_kernel", "conv_dgrad_s2_kernel", "conv_fwd_s2_dma_kernel",
                   "conv_pt_kernel", "conv_wr_kernel", "conv_pw_kernel", "conv_fwd_kernel", "conv_fwd_wide_kernel",
                   "conv_fwd_dma_kernel"):
        assert any(n.startswith(family) for n in fwd), family
    for kind in PINNED + ("conv_wgrad_pt_kernel<", "conv_wgrad_co1m_kernel<", "conv_wgrad_kernel<4, 9, 0, false>",
                          "conv_wgrad_kernel<4, 6, 1, true>"):
        assert any(n.startswith(kind) for n in have["names"]), kind
    assert len(have["refusals"]) == 11  # one per set_error of climsr_conv2d_fwd


def test_every_route_answers_as_recorded(sweep):
    got, want = sweep
    assert got["cases"] == want["cases"]
    assert got["names"] == want["names"]
    assert got["refusals"] == want["refusals"]
    moved = sorted(k for k in want["blocks"] if got["blocks"].get(k) != want["blocks"][k])
    assert not moved and got["blocks"].keys() == want["blocks"].keys(), f"(in_c>out_c) blocks whose answers moved: {moved}"
