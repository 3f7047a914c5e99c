"""The optimizer kernels against bit patterns recorded before the five update entries became one kernel.

tests/golden/opt_step_parent.npz (tools/opt_step_fixture.py, written on an MI355X with the library of the commit before
``opt_step_kernel``) holds fixed inputs and what that library computed from them: three steps of each update entry over
the 16-byte body, a block boundary, the tail and the bf16 mirror window with its guard words; 40 all-tail draws of
``climsr_adamw_step`` and ``climsr_adam_step``; every hp row and the counters of both schedule entries for each kind.
The tree's library must give the same bits -- no tolerance.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def recorded_and_replayed():
    from climsr_amd import _lib

    spec = importlib.util.spec_from_file_location("opt_step_fixture", os.path.join(ROOT, "tools", "opt_step_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with np.load(os.path.join(ROOT, "tests", "golden", "opt_step_parent.npz")) as f:
        data = {k: f[k] for k in f.files}
    inp = {k: v for k, v in data.items() if k.startswith("in_")}
    want = {k: v for k, v in data.items() if k.startswith("out_")}
    return want, mod.replay(_lib.load(), inp), mod


def _same_bits(want, got, keys):
    assert keys
    for k in keys:
        a, b = torch.from_numpy(want[k]), torch.from_numpy(got[k])
        if a.dtype == torch.float64:  # the schedule counters: whole numbers
            a, b = a.view(torch.int64), b.view(torch.int64)
        assert a.dtype in (torch.int32, torch.int16, torch.int64) and a.dtype == b.dtype, k
        assert torch.equal(a, b), f"{k}: {int((a != b).sum())} of {a.numel()} words differ from the recorded bits"


def test_fixture_is_complete(recorded_and_replayed):
    want, got, mod = recorded_and_replayed
    assert set(want) == set(got)
    for entry in mod.ENTRIES:
        assert {f"out_{entry}_{x}" for x in "pmv"} <= set(want)
        assert (f"out_{entry}_mirror" in want) == (entry != "adamw_step")
    assert len([k for k in want if k.startswith("out_sched_lambda") and k.endswith("_hp")]) == 14
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "opt_step_parent.npz")) < 200 * 1024


@pytest.mark.parametrize("entry", ["adamw_step", "adamw_step_mirror", "adamw_step_scaled", "adam_step", "adam_step_scaled"])
def test_update_entry_bits(recorded_and_replayed, entry):
    want, got, _mod = recorded_and_replayed
    _same_bits(want, got, [f"out_{entry}_{x}" for x in ("p", "m", "v") + (("mirror",) if entry != "adamw_step" else ())])


@pytest.mark.parametrize("entry", ["adamw_step", "adam_step"])
def test_all_tail_bits(recorded_and_replayed, entry):
    want, got, _mod = recorded_and_replayed
    _same_bits(want, got, [f"out_tail_{entry}"])


def test_mirror_window_and_guard(recorded_and_replayed):
    """What the recorded mirror must itself satisfy: bf16 (RNE) of p inside the window, the guard words untouched."""
    want, _got, mod = recorded_and_replayed
    for entry in mod.ENTRIES[1:]:
        p = torch.from_numpy(want[f"out_{entry}_p"]).view(torch.float32)
        mirror = torch.from_numpy(want[f"out_{entry}_mirror"])
        assert torch.equal(mirror[:mod.MN], p[mod.LO:mod.LO + mod.MN].to(torch.bfloat16).view(torch.int16)), entry
        assert bool((mirror[mod.MN:].to(torch.int32) & 0xFFFF == mod.GUARD_WORD).all()) and mirror.numel() == mod.MN + mod.GUARD


def test_schedule_bits(recorded_and_replayed):
    want, got, _mod = recorded_and_replayed
    _same_bits(want, got, [k for k in want if k.startswith(("out_sched_", "out_adamw_hparams"))])
