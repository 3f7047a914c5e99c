"""bench.py's command line: a plain run measures the headline step only, ``--full`` adds the other measurements,
``--dump-outputs DIR`` writes the last timed step's outputs."""
import json
import os

import numpy as np
import pytest
import torch

LINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")


def test_parse_full_and_dump_default_off():
    import bench

    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = bench.parse(["--full", "--dump-outputs", "somewhere"])
    assert a.full and a.dump_outputs == "somewhere"


def test_dump_outputs_writes_float32_and_samples_large_arrays(tmp_path):
    import bench

    small = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    big = torch.arange(bench.DUMP_MAX_ELEMS + 1000, dtype=torch.float32)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), {"small": small, "big": big})
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.shape == (3, 4) and np.array_equal(s, small.numpy())
    b = np.load(tmp_path / "a" / "big.npy")
    assert b.dtype == np.float32 and b.shape == (bench.DUMP_MAX_ELEMS,)
    assert np.all(np.diff(b) >= 0) and b[-1] > bench.DUMP_MAX_ELEMS // 2  # sorted positions over the whole array
    assert np.array_equal(b, np.load(tmp_path / "b" / "big.npy"))  # the same positions every time
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64e6


@pytest.mark.gpu
def test_plain_run_measures_only_the_headline_and_dumps_outputs(tmp_path, capsys):
    """A plain run of the GAN step at a small shape (nb 1, batch 2, 16 -> 64): no median steps, kernel profile, CPU
    baseline or config-2 record; the dump holds the losses of the line, the SR batch and both parameter buffers, and
    a second run with the same arguments starts from the same inputs and initial state."""
    import bench

    argv = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--nb", "1", "--batch", "2", "--lr-size", "16"]
    dumps = []
    for sub in ("a", "b"):
        assert bench.main(argv + ["--dump-outputs", str(tmp_path / sub)]) == 0
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        for k in LINE_KEYS:
            assert k in line, k
        assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(2 * 64 * 64 / 1e6 / (line["ms_per_step"] / 1e3), rel=1e-2)
        assert line["median"] is None and line["cpu_baseline"] is None and line["config2"] is None
        assert line["roofline"] is None and line["profile"] is None and line["kernels"] == {}
        d = {f[:-4]: np.load(tmp_path / sub / f) for f in sorted(os.listdir(tmp_path / sub))}
        assert sorted(d) == ["discriminator_params", "generator_params", "loss", "sr"]
        assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in d.values())
        assert d["sr"].shape == (2, 1, 64, 64) and d["loss"].shape == (2,)
        assert np.allclose(d["loss"], line["loss_last"], rtol=1e-5, atol=1e-6)
        dumps.append(d)
    a, b = dumps
    # same inputs and initial state from run to run; the kernels' atomic float sums may order differently, and an AdamW
    # step moves a weight by about lr <= 1e-4 at the most, so the five steps of a run (2 eager, 1 warm-up, 2 timed)
    # cannot take two runs' weights further apart than 1e-3; the SR batch is computed in bf16, where such a difference
    # can also flip a rounding: one bf16 ulp, at most 2^-7 of the largest magnitude
    for k in a:
        assert a[k].shape == b[k].shape
        assert np.abs(a[k] - b[k]).max() <= 1e-3 + 2.0 ** -7 * np.abs(a[k]).max(), k
