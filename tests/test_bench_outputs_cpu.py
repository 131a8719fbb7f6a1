"""bench.py on the CPU stand-ins of the kernels (tests/ops_emulation.py): `--steps` sets the number of timed pipeline calls, `ms_per_step`
is the timed region over them, and `--dump-outputs DIR` writes what the last timed call returned -- the same arrays, float32, from run to
run on the same arguments -- plus the fixed, seeded sample that bounds a large output."""
import numpy as np
import pytest
import torch

import bench
import ops_emulation
from diffusers_amd import ops
from diffusers_amd.pipelines import StableDiffusionXLPipeline


@pytest.fixture
def cpu_bench(monkeypatch):
    ops_emulation.install(monkeypatch, ops)
    monkeypatch.setattr(ops, "TUNING", False)
    monkeypatch.setattr(bench, "_device", lambda local: torch.device("cpu"))
    monkeypatch.setattr(bench, "_sync", lambda: None)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    calls = {"n": 0, "last": None}
    real_call = StableDiffusionXLPipeline.__call__

    def counting_call(self, *a, **kw):
        out = real_call(self, *a, **kw)
        calls["n"] += 1
        calls["last"] = out.images.detach().float().clone()
        return out
    monkeypatch.setattr(StableDiffusionXLPipeline, "__call__", counting_call)
    return calls


def _run(tmp_path, name, steps, warmup=1):
    return bench.main(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--tiny", "--no-graph", "--denoise-steps", "2",
                       "--dump-outputs", str(tmp_path / name)])


def test_steps_and_dumped_outputs(cpu_bench, tmp_path):
    rec = _run(tmp_path, "a", steps=3, warmup=2)
    assert cpu_bench["n"] == 2 + 3, "warm-up + timed pipeline calls"
    assert rec["steps"] == 3 and rec["warmup"] == 2
    assert rec["ms_per_step"] > 0 and abs(rec["ms_per_step"] * rec["value"] - 1000.0) < 1e-6 * 1000.0
    a = np.load(tmp_path / "a" / "images.npy")
    assert rec["dumped_outputs"] == {"images.npy": [1, 3, 32, 32]}
    assert a.dtype == np.float32 and a.shape == (1, 3, 32, 32) and np.isfinite(a).all()
    assert np.array_equal(a, cpu_bench["last"].numpy()), "the dump is the last timed call's output"
    _run(tmp_path, "b", steps=1)
    assert cpu_bench["n"] == 5 + 1 + 1
    assert np.array_equal(a, np.load(tmp_path / "b" / "images.npy")), "same arguments, different outputs: the inputs are not fixed"


def test_large_output_is_a_fixed_seeded_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_ELEMS", 1000)
    big = torch.randn(3, 50, 70)
    w1 = bench.dump_outputs(tmp_path / "1", {"video": big, "small": big[0, :10]})
    w2 = bench.dump_outputs(tmp_path / "2", {"video": big})
    assert w1 == {"video_sample.npy": [1000], "small.npy": [10, 70]} and w2 == {"video_sample.npy": [1000]}
    s1, s2 = np.load(tmp_path / "1" / "video_sample.npy"), np.load(tmp_path / "2" / "video_sample.npy")
    assert s1.dtype == np.float32 and np.array_equal(s1, s2)
    assert np.isin(s1, big.numpy().reshape(-1)).all()
    assert np.array_equal(np.load(tmp_path / "1" / "small.npy"), big[0, :10].numpy())
