"""CPU: the path of every SD / SDXL ``__call__`` from its arguments to the denoising loop, bit for bit against a recording.

tests/sd_call_paths.py holds the table and says how a call is recorded; tests/golden/sd_call_paths.npz / .json were written by
tools/record_sd_call_paths.py before the six ``__call__`` bodies were folded into shared ones.  Per valid call: the scheduler's
class, the ``set_timesteps`` / ``set_begin_index`` calls it got, its timesteps and begin index; every ``torch.randn`` / ``_randn``
draw in order (shape, dtype, device, generator or not) and the generator's state afterwards; what ``encode_prompt`` was handed; the
tensors handed to ``precompute_conditioning``; and, as ``_denoise`` sees them, the start latents, step count, begin, guidance
scale, CFG flag, ``_eta``, ``_guidance_rescale``, the noise table and every ``_inpaint`` entry; the return type; the capture key
(call_sequences.graph_key_of) without its addresses.  Per refused call: the exception's type and message.  No tolerance: nothing
here depends on a reduction order or on the number of threads."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import inpaint_emulation
import ops_emulation
import sd_call_paths as S
from diffusers_amd import ops

GOLDEN = Path(__file__).parent / "golden"


@pytest.fixture(autouse=True)
def _emulated_kernels(monkeypatch):
    ops_emulation.install(monkeypatch, ops)
    inpaint_emulation.install(monkeypatch, ops)
    monkeypatch.setattr(ops, "TUNING", False)


@pytest.fixture(scope="module")
def recorded():
    with np.load(GOLDEN / "sd_call_paths.npz") as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def recorded_errors():
    return json.loads((GOLDEN / "sd_call_paths.json").read_text())


def test_the_recording_holds_exactly_the_table(recorded, recorded_errors):
    assert {k.split("/")[0] for k in recorded} == {c.name for c in S.CASES}
    assert set(recorded_errors) == {c.name for c in S.ERRORS}
    assert all(v["type"] is not None for v in recorded_errors.values())


@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_valid_call_matches_the_recording(case, recorded):
    arrays, meta = S.record(case)
    want = {k.split("/", 1)[1]: v for k, v in recorded.items() if k.startswith(case.name + "/")}
    want_meta = json.loads(str(want.pop("meta")))
    for k in sorted(set(meta) | set(want_meta)):
        assert meta.get(k) == want_meta.get(k), f"{case.name}: {k}"
    assert sorted(arrays) == sorted(want)
    for k, v in arrays.items():
        assert v.dtype == want[k].dtype and torch.equal(torch.from_numpy(v), torch.from_numpy(want[k])), f"{case.name}: {k}"


@pytest.mark.parametrize("case", S.ERRORS, ids=[c.name for c in S.ERRORS])
def test_refused_call_matches_the_recording(case, recorded_errors):
    assert S.record_error(case) == recorded_errors[case.name]
