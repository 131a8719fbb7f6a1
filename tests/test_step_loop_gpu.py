"""The one denoising loop of the pipelines (pipelines._CapturedStepLoop) on the GPU, in both capture modes: warm-up and capture
leave no extra step behind, a later call replays the captured step from any begin index, and an interrupted loop leaves the
scheduler where it stopped.  Tiny SD1.5 pipeline, 4 steps; every result is held bit for bit to the eager loop of a second, freshly
built pipeline (the CPU half is tests/test_step_loop_cpu.py)."""
import pytest
import torch

from diffusers_amd import factory

pytestmark = pytest.mark.gpu
DEV = "cuda"
bf16 = torch.bfloat16
STEPS, GUIDANCE = 4, 5.0


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator("cpu").manual_seed(seed)).to(bf16)


LAT_A, LAT_B = _rand((1, 4, 16, 16), 5), _rand((1, 4, 16, 16), 6)
PROMPT = torch.cat([_rand((1, 7, 64), 2), _rand((1, 7, 64), 1)], 0)           # [negative ; positive]


def _pipeline():
    pipe = factory.build_sd15_pipeline(device=DEV, tiny=True, seed=0)
    pipe.scheduler.set_timesteps(STEPS, device=DEV)
    return pipe


def _step_args(pipe):
    """The conditioning of one call, in buffers of its own."""
    return (pipe.unet.precompute_conditioning(PROMPT.to(DEV).contiguous(), None), GUIDANCE, True)


@pytest.fixture(scope="module")
def eager():
    """What a freshly built pipeline computes eagerly: computed once, never written again."""
    with torch.no_grad():
        pipe = _pipeline()
        args = _step_args(pipe)
        return {"a": pipe._denoise(LAT_A.to(DEV), args, STEPS, False).clone(),
                "b": pipe._denoise(LAT_B.to(DEV), args, STEPS, False).clone(),
                "b_from_1": pipe._denoise(LAT_B.to(DEV), args, STEPS - 1, False, begin=1).clone(),
                "b_from_1_two_steps": pipe._denoise(LAT_B.to(DEV), args, 2, False, begin=1).clone()}


@pytest.mark.parametrize("mode", [True, "plan"], ids=["graph", "plan"])
def test_capture_replay_begin_and_interrupt(mode, eager):
    assert all(torch.isfinite(v.float()).all() for v in eager.values())
    assert not torch.equal(eager["a"], eager["b"]) and not torch.equal(eager["b"], eager["b_from_1"])
    assert not torch.equal(eager["b_from_1"], eager["b_from_1_two_steps"])
    with torch.no_grad():
        pipe = _pipeline()
        sch = pipe.scheduler
        # first call: warm-up and capture leave no extra step in the result
        out = pipe._denoise(LAT_A.to(DEV), _step_args(pipe), STEPS, mode)
        assert torch.equal(out, eager["a"]) and sch._step_index == STEPS
        g = pipe._graph
        assert g is not None

        # second call, other latent contents (and conditioning buffers of its own): the captured step is replayed
        out = pipe._denoise(LAT_B.to(DEV), _step_args(pipe), STEPS, mode)
        assert pipe._graph is g and out is pipe._static["latents"]
        assert torch.equal(out, eager["b"]) and sch._step_index == STEPS

        # begin offset: the step reads its row through the device counter, so the same captured step serves
        out = pipe._denoise(LAT_B.to(DEV), _step_args(pipe), STEPS - 1, mode, begin=1)
        assert pipe._graph is g
        assert torch.equal(out, eager["b_from_1"]) and sch._step_index == STEPS

        # interrupt after two replays
        seen = []

        def cb(p, i, t, kw):
            seen.append((i, int(t)))
            p._interrupt = i == 1
            return {}

        pipe._arm_callback(cb, None)
        out = pipe._denoise(LAT_B.to(DEV), _step_args(pipe), STEPS - 1, mode, begin=1)
        assert pipe._graph is g and seen == [(0, int(sch.timesteps[1])), (1, int(sch.timesteps[2]))]
        assert sch._step_index == 1 + 2
        assert torch.equal(out, eager["b_from_1_two_steps"])
