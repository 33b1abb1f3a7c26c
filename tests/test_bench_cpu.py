"""bench.py's command line and output dump (host only; the timed run itself needs the GPU)."""
import os
import sys

import numpy as np
import torch

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default_and_full_is_opt_in(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert a.full and a.dump_outputs == "somewhere"


def test_dump_outputs_is_float32_and_repeatable(tmp_path):
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(96, 64), torch.nn.Linear(64, 3))   # 6144 > DUMP_SAMPLE: sampled
    model(torch.randn(5, 96)).square().mean().backward()
    losses = {"contrastive_loss": torch.tensor(1.5), "loss": torch.tensor(1.5, dtype=torch.bfloat16)}
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, losses, model)
    bench.dump_outputs(b, losses, model)
    assert sorted(os.listdir(a)) == ["contrastive_loss.npy", "grads_sample.npy", "loss.npy", "params_sample.npy"]
    n = bench.DUMP_SAMPLE + 64 + 64 * 3 + 3
    for name in os.listdir(a):
        x, y = np.load(os.path.join(a, name)), np.load(os.path.join(b, name))
        assert x.dtype == np.float32 and np.array_equal(x, y)
        assert x.shape == ((n,) if name.endswith("_sample.npy") else (1,))
    # the small tensors are kept whole, in named_parameters() order
    params = np.load(os.path.join(a, "params_sample.npy"))
    assert np.array_equal(params[bench.DUMP_SAMPLE:bench.DUMP_SAMPLE + 64], model[0].bias.detach().numpy())
    assert np.array_equal(params[-3:], model[1].bias.detach().numpy())
