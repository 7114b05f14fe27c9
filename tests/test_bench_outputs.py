"""bench.py's plain run and --dump-outputs: the dump holds the step's loss, logits, flat gradient and
flat parameters as float32 .npy within the byte budget (CPU, on stand-in tensors); on the GPU a plain
run prints the headline line without the --full legs, times exactly --steps steps and writes a dump
that agrees with the line."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("loss", "logits", "grads", "params")


def _stand_in(nparam):
    g = torch.Generator().manual_seed(0)
    step = types.SimpleNamespace(loss=torch.rand(1, generator=g), out=torch.randn(4, 11, generator=g),
                                 grads=torch.randn(nparam, generator=g))
    flat = torch.randn(nparam, generator=g)
    return step, types.SimpleNamespace(flat_parameters=lambda: flat), flat


def test_dump_outputs_writes_the_steps_arrays(tmp_path):
    step, model, flat = _stand_in(1000)
    bench.dump_outputs(str(tmp_path), step, model)
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in NAMES)
    got = {n: np.load(tmp_path / (n + ".npy")) for n in NAMES}
    assert all(a.dtype == np.float32 for a in got.values())
    np.testing.assert_array_equal(got["loss"], step.loss.numpy())
    np.testing.assert_array_equal(got["logits"], step.out.numpy())
    np.testing.assert_array_equal(got["grads"], step.grads.numpy())
    np.testing.assert_array_equal(got["params"], flat.numpy())


def test_dump_outputs_samples_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096)
    step, model, flat = _stand_in(5000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), step, model)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 4096
    a, b = (np.load(tmp_path / d / "grads.npy") for d in ("a", "b"))
    np.testing.assert_array_equal(a, b)  # the same sample from run to run
    assert 0 < a.size < 5000 and np.isin(a, step.grads.numpy()).all()
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "loss.npy"), step.loss.numpy())  # small arrays whole


@pytest.mark.gpu
def test_plain_run_is_the_headline_only_and_dumps_its_last_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["unit"] == "clips/s" and rec["higher_is_better"] is True
    assert rec["dtype"] == "bf16x3" and rec["ms_per_step"] > 0
    assert abs(rec["value"] - 256 / (rec["ms_per_step"] * 1e-3)) <= 1e-3 * rec["value"]
    assert not set(rec) & set(bench.FULL_KEYS)
    got = {n: np.load(tmp_path / (n + ".npy")) for n in NAMES}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert got["logits"].shape == (256, 11) and got["grads"].shape == got["params"].shape
    assert got["grads"].size > 1_000_000 and np.abs(got["grads"]).max() > 0
    assert abs(float(got["loss"][0]) - rec["config"]["final_loss"]) <= 1e-5
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_BYTES
