"""The one denoising loop of the pipelines (pipelines._CapturedStepLoop) and the per-step noise table of the SD / SDXL family, on
``device="cpu"`` pipelines over the kernel stand-ins (the GPU half is tests/test_step_loop_gpu.py)."""
import pytest
import torch

import call_sequences as CS
import inpaint_emulation
import ops_emulation
from diffusers_amd import factory, ops, pipelines as P
from diffusers_amd.schedulers import DDIMScheduler

bf16 = torch.bfloat16


@pytest.fixture(autouse=True)
def _emulated_kernels(monkeypatch):
    ops_emulation.install(monkeypatch, ops)
    inpaint_emulation.install(monkeypatch, ops)
    monkeypatch.setattr(ops, "TUNING", False)


def _gen(seed):
    return torch.Generator("cpu").manual_seed(seed)


# ----------------------------------------------------------------------------------------------------------------------
# the noise table
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def sd15():
    return factory.build_sd15_pipeline(device="cpu", tiny=True, seed=0)


def test_noise_table_rows_are_the_generators_draws_in_step_order(sd15):
    lat = torch.zeros((1, 4, 16, 16), dtype=bf16)
    sd15._fill_noise_table(lat, _gen(11), 6, 4, 2)
    table = sd15._noise_table
    assert tuple(table.shape) == (6, 1, 4, 16, 16) and table.dtype == bf16
    g = _gen(11)
    for row in range(2, 6):
        assert torch.equal(table[row], torch.randn(lat.shape, generator=g, dtype=bf16)), row
    assert not table[:2].any()                  # (a new table: the rows no step reads are zero)


def test_noise_table_is_refilled_in_place_while_its_shape_holds(sd15):
    lat = torch.zeros((1, 4, 16, 16), dtype=bf16)
    sd15._fill_noise_table(lat, _gen(1), 6, 4, 2)
    ptr, first = sd15._noise_table.data_ptr(), sd15._noise_table.clone()
    sd15._fill_noise_table(lat, _gen(2), 6, 4, 2)
    assert sd15._noise_table.data_ptr() == ptr and not torch.equal(sd15._noise_table, first)
    keep = sd15._noise_table                    # (alive: the allocator cannot hand its address to the next table)
    sd15._fill_noise_table(torch.zeros((1, 4, 16, 24), dtype=bf16), _gen(2), 6, 4, 2)
    assert sd15._noise_table.data_ptr() != ptr and tuple(sd15._noise_table.shape) == (6, 1, 4, 16, 24)
    sd15._fill_noise_table(lat, _gen(2), 5, 4, 1)
    assert sd15._noise_table.data_ptr() not in (ptr, keep.data_ptr()) and sd15._noise_table.shape[0] == 5


def test_noise_table_takes_one_generator_per_sample(sd15):
    lat = torch.zeros((2, 4, 16, 16), dtype=bf16)
    sd15._fill_noise_table(lat, [_gen(5), _gen(6)], 3, 3, 0)
    gens = [_gen(5), _gen(6)]
    for row in range(3):
        assert torch.equal(sd15._noise_table[row], P._randn(lat.shape, gens, torch.device("cpu"), bf16)), row
    ga, gb = _gen(5), _gen(6)
    want = torch.cat([torch.randn((1, 4, 16, 16), generator=g, dtype=bf16) for g in (ga, gb)], 0)
    assert torch.equal(sd15._noise_table[0], want)


def test_text_to_image_eta_and_set_eta_fill_the_same_table(sd15):
    kw = dict(CS.FAMILIES["sd15"].kwargs, eta=0.5)
    CS.graph_key_of(sd15, dict(kw, generator=lambda: _gen(9)))       # the call up to the key: the table is drawn by then
    N = kw["num_inference_steps"]
    called, eta = sd15._noise_table.clone(), sd15._eta
    assert eta == 0.5 and tuple(called.shape) == (N, 1, 4, 16, 16)
    other = factory.build_sd15_pipeline(device="cpu", tiny=True, seed=0)
    lat = torch.zeros((1, 4, 16, 16), dtype=bf16)
    g = _gen(9)
    other._set_eta(0.5, lat, g, N, N, 0)
    assert other._eta == 0.5 and torch.equal(other._noise_table, called)
    g = _gen(9)
    assert torch.equal(called, torch.stack([torch.randn(lat.shape, generator=g, dtype=bf16) for _ in range(N)]))


def test_eta_on_a_scheduler_without_it_is_refused_with_both_texts(sd15):
    euler = factory.build_sdxl_pipeline(device="cpu", tiny=True, seed=0).scheduler
    sd15.scheduler = euler
    with pytest.raises(ValueError, match="pipeline_stable_diffusion.py:608-625"):
        sd15(use_graph=False, **CS.materialise(dict(CS.FAMILIES["sd15"].kwargs, eta=0.5), "cpu"))
    with pytest.raises(ValueError, match="eta > 0 is a DDIMScheduler option$"):
        sd15._set_eta(0.5, torch.zeros((1, 4, 16, 16), dtype=bf16), None, 4, 4, 0)


# ----------------------------------------------------------------------------------------------------------------------
# the loop
# ----------------------------------------------------------------------------------------------------------------------
class _Stub(P._StepCallbacks, P._CapturedStepLoop):
    """The smallest pipeline the loop runs: a step that adds 1 and advances the scheduler's host-side step index."""

    def __init__(self, n=5):
        self.scheduler = DDIMScheduler()
        self.scheduler.set_timesteps(n, device="cpu")

    def _step(self, latents):
        latents.add_(1.0)
        self.scheduler._step_index += 1
        return latents


def test_eager_loop_runs_num_steps_from_begin():
    pipe = _Stub(5)
    x0 = torch.randn(2, 3, generator=_gen(0))
    x = x0.clone()
    seen = []

    def cb(p, i, t, kw):
        assert p is pipe and kw["latents"] is x
        seen.append((i, int(t)))
        return {}

    pipe._arm_callback(cb, None)
    out = pipe._denoise(x, (), 3, False, begin=2)
    assert out is x and torch.equal(x, x0 + 3)
    assert pipe.scheduler._step_index == 5                       # reset(2), then three steps
    assert seen == [(i, int(t)) for i, t in enumerate(pipe.scheduler.timesteps[2:5])]
    assert pipe._graph is None and pipe._graph_key is None       # nothing was captured


def test_eager_loop_stops_after_the_step_that_interrupts():
    pipe = _Stub(5)
    x = torch.zeros(2, 3)
    calls = []

    def cb(p, i, t, kw):
        calls.append(i)
        p._interrupt = True
        return {}

    pipe._arm_callback(cb, None)
    pipe._denoise(x, (), 3, False, begin=2)
    assert calls == [0] and torch.equal(x, torch.ones(2, 3)) and pipe.scheduler._step_index == 3


def test_a_pipeline_without_callbacks_runs_every_step():
    class Plain(P._CapturedStepLoop):
        scheduler = _Stub(4).scheduler
        _step = _Stub._step

    x = torch.zeros(3)
    Plain()._denoise(x, (), 4, False)
    assert torch.equal(x, torch.full((3,), 4.0))


class _Replays:
    """Stands in for a captured step: counts its replays."""

    def __init__(self):
        self.n = 0

    def replay(self):
        self.n += 1


def _static_tensors(family, step_args):
    """The tensors of ``step_args`` a later call's contents are copied into."""
    if family == "sd15":
        cond = step_args[0]
        return [t for layer in cond["kvs"] for kv in layer for t in (kv.k, kv.vt)]
    if family == "flux":
        return [step_args[0], step_args[1]["pooled_emb"]]
    if family == "wan":
        return [t for pair in step_args[0]["kvs"] for t in pair]
    return [step_args[0]]                                        # ddpm: the noise table


@pytest.mark.parametrize("family", ["sd15", "flux", "wan", "ddpm"])
def test_refresh_static_runs_once_per_replayed_call_and_never_on_a_capture(family, monkeypatch):
    fam = CS.FAMILIES[family]
    pipe = fam.build("cpu")
    refreshed, keyed = [], []
    refresh, make = pipe._refresh_static, pipe._make_graph_key

    def counting(captured, new):
        refreshed.append((captured, new))
        return refresh(captured, new)

    def recording(latents, *step_args):
        keyed.append((latents, step_args, make(latents, *step_args)))
        return keyed[-1][2]

    def no_device(kind):
        raise CS._KeyTaken

    pipe._refresh_static, pipe._make_graph_key = counting, recording
    monkeypatch.setattr(P, "_side_stream", no_device)

    # first call: no captured step, so the loop goes on to warm up and capture -- which is where a device is needed
    with pytest.raises(CS._KeyTaken):
        pipe(use_graph=True, **CS.materialise(fam.kwargs, "cpu"))
    assert len(keyed) == 1 and refreshed == [] and pipe._graph is None

    # what a capture leaves behind, with static buffers whose contents are not the next call's
    latents, step_args, key = keyed[0]
    held = _static_tensors(family, step_args)
    assert held
    for t in held:
        t.zero_()
    pipe._graph, pipe._graph_key = _Replays(), key + (False,)
    pipe._static = {"latents": torch.zeros_like(latents), "step_args": step_args}

    out = pipe(use_graph=True, **CS.materialise(fam.kwargs, "cpu")).images
    n = fam.kwargs["num_inference_steps"]
    assert len(keyed) == 2 and keyed[1][2] == key
    assert len(refreshed) == 1 and refreshed[0][0] is step_args
    assert len(refreshed[0][1]) == len(keyed[1][1]) and all(a is b for a, b in zip(refreshed[0][1], keyed[1][1]))
    assert pipe._graph.n == n and pipe.scheduler._step_index == n
    new = _static_tensors(family, keyed[1][1])
    assert all(a is not b and torch.equal(a, b) for a, b in zip(held, new)) and any(t.any() for t in held)
    # the loop's own job: the new call's latents copied into the buffer the captured step reads, which is what comes back
    assert torch.equal(pipe._static["latents"], keyed[1][0]) and pipe._static["latents"].any()
    if family != "ddpm":                                         # (ddpm post-processes its image; the others return the buffer)
        assert out.data_ptr() == pipe._static["latents"].data_ptr()
