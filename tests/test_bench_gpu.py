"""bench.py with a caller's arguments: --steps sets the number of timed steps, and --dump-outputs writes the outputs of the
last timed forward, which depend on the arguments only - two runs give the same files bit for bit."""
import json
import os
import sys

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu


def _bench(monkeypatch, capfd, dump_dir, steps):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--batch", "4", "--frames", "40",
                                      "--tokens", "24", "--no-extra", "--no-cpu-baseline", "--dump-outputs", dump_dir])
    bench.main()
    out, err = capfd.readouterr()
    return json.loads(out.strip().splitlines()[-1]), err


def test_bench_dumps_the_last_timed_forward_reproducibly(tmp_path, monkeypatch, capfd):
    shapes = {"mel_outputs": (4, 80, 40), "mel_outputs_postnet": (4, 80, 40), "gate_outputs": (4, 40), "alignments": (4, 40, 24)}
    dumps = []
    for name, steps in (("a", 3), ("b", 5)):
        line, err = _bench(monkeypatch, capfd, str(tmp_path / name), steps)
        assert line["steps"] == steps and f"for {steps} steps" in err
        assert sorted(os.listdir(tmp_path / name)) == sorted(k + ".npy" for k in shapes)
        dumps.append({k: np.load(tmp_path / name / f"{k}.npy") for k in shapes})
    for k, shape in shapes.items():
        a, b = dumps[0][k], dumps[1][k]
        assert a.dtype == np.float32 and a.shape == shape and np.isfinite(a).all()
        assert np.array_equal(a, b), k   # the last timed forward is the same computation whatever the step count
    assert np.abs(dumps[0]["mel_outputs_postnet"]).max() > 0
    assert np.allclose(dumps[0]["alignments"].sum(-1), 1.0, atol=1e-4)   # attention rows of a real forward
