"""CPU: what the seven schedulers compute on the host and hand to their fused-step kernels, bit for bit against a recording.

tests/scheduler_paths.py holds the table and says how a case is recorded; tests/golden/scheduler_paths.npz / .json were written by
tools/record_scheduler_paths.py before the schedulers' shared code (ladders, timestep spacing, the add_noise index rule, the tail of
``set_timesteps``, in-place device refreshes, the fused-step entry points) was folded.  Per valid case: schedules and tables as
bytes (NaN-safe), which buffers kept their addresses, the log of every sampler-op call (scalars, which buffer each tensor is, the
bits of fresh tensors, the device counters), return types, and the indices after every call.  Per refusal: the exception's type and
message.

The golden file also holds the recording host's ``scheduler_paths.libm_probe()``: fp32 ``pow`` / ``log`` / ``expm1`` results on fixed
inputs, which this test recomputes without schedulers.py.  Where the host reproduces the probe, EVERY array and number has to match
bit for bit.  Those three functions are not correctly rounded, though, and torch picks their implementation by CPU: where the probe
differs, the fp32 arrays of the five classes that call them (Euler, Euler a, DDIM, DDPM, UniPC) cannot match in the last place, and
an array that is not bit-equal must satisfy |got - want| <= LIBM_TOL * max(|want|, 1) with the same non-finite entries: two libm
results each within 1 ulp of the true value are within 2 ulp = 2^-22 relative of each other, and an entry is at most about a dozen
correctly rounded fp32 operations away from them, on operands no larger than the entry or than 1 (the alpha-bar rows subtract
numbers below 1) -- 16 * 2^-22.  DPM-Solver++ and FlowMatch compute in float64 numpy and round once: bit for bit on every host,
like every integer, index, address identity, logged call, generator draw and message of all seven."""
import json
from pathlib import Path

import numpy as np
import pytest

import scheduler_paths as SP

GOLDEN = Path(__file__).parent / "golden"
LIBM_KINDS = ("euler", "euler_a", "ddim", "ddpm", "unipc")
LIBM_TOL = 16 * 2.0 ** -22


def _same(name, got, want, same_libm):
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.tobytes() == want.tobytes():
        return True
    if not same_libm and name.split("/")[0] in LIBM_KINDS and got.dtype == np.float32:
        g, w = got.astype(np.float64), want.astype(np.float64)
        fin = np.isfinite(w)        # (UniPC's bh1 rows hold inf / NaN on the last step, h = inf: those must be the same ones)
        if not np.array_equal(fin, np.isfinite(g)) or not np.array_equal(g[~fin], w[~fin], equal_nan=True):
            return False
        return bool(np.all(np.abs(g[fin] - w[fin]) <= LIBM_TOL * np.maximum(np.abs(w[fin]), 1.0)))
    return False


def _same_meta(name, got, want, same_libm):
    """JSON values: equal, or (another libm, the five kinds) floats within LIBM_TOL -- ``init_noise_sigma`` is a sigma."""
    if got == want or same_libm or name.split("/")[0] not in LIBM_KINDS:
        return got == want
    if isinstance(got, float) and isinstance(want, float):
        return abs(got - want) <= LIBM_TOL * max(abs(want), 1.0)
    if isinstance(got, list) and isinstance(want, list) and len(got) == len(want):
        return all(_same_meta(name, g, w, same_libm) for g, w in zip(got, want))
    if isinstance(got, dict) and isinstance(want, dict) and sorted(got) == sorted(want):
        return all(_same_meta(name, got[k], want[k], same_libm) for k in got)
    return False


@pytest.fixture(autouse=True)
def _logging_standins(monkeypatch):
    SP.install(monkeypatch)


@pytest.fixture(scope="module")
def recorded():
    with np.load(GOLDEN / "scheduler_paths.npz") as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def same_libm(recorded):
    """This host's fp32 pow / log / expm1 give the recording host's bits: then so must every table."""
    probe = SP.libm_probe()
    return all(v.tobytes() == recorded[f"{SP.PROBE}:{k}"].tobytes() for k, v in probe.items())


@pytest.fixture(scope="module")
def recorded_errors():
    return json.loads((GOLDEN / "scheduler_paths.json").read_text())


def test_the_recording_holds_exactly_the_table(recorded, recorded_errors):
    assert {k.split(":")[0] for k in recorded} == set(SP.CASES) | {SP.PROBE}
    assert {k.split(":")[1] for k in recorded if k.startswith(SP.PROBE + ":")} == set(SP.libm_probe())
    assert set(recorded_errors) == set(SP.ERRORS)
    assert all(v["type"] is not None for v in recorded_errors.values())


@pytest.mark.parametrize("name", list(SP.CASES))
def test_case_matches_the_recording(name, recorded, same_libm):
    arrays, meta = SP.record(name)
    want = {k.split(":", 1)[1]: v for k, v in recorded.items() if k.startswith(name + ":")}
    want_meta = json.loads(str(want.pop("meta")))
    for k in sorted(set(meta) | set(want_meta)):
        if k == "log":
            assert len(meta[k]) == len(want_meta[k]), f"{name}: {len(meta[k])} logged calls, recorded {len(want_meta[k])}"
            for i, (got, exp) in enumerate(zip(meta[k], want_meta[k])):
                assert got == exp, f"{name}: log entry {i}"
        elif k.endswith(".state"):
            assert _same_meta(name, meta.get(k), want_meta.get(k), same_libm), f"{name}: {k}: {meta.get(k)} != {want_meta.get(k)}"
        else:
            assert meta.get(k) == want_meta.get(k), f"{name}: {k}"
    assert sorted(arrays) == sorted(want)
    for k, v in arrays.items():
        assert _same(name, v, want[k], same_libm), f"{name}: {k} (same libm as the recording: {same_libm})"


@pytest.mark.parametrize("name", list(SP.ERRORS))
def test_refusal_matches_the_recording(name, recorded_errors):
    assert SP.record_error(name) == recorded_errors[name]
