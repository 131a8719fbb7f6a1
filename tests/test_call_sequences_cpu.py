"""The capture keys of the pipelines, on ``device="cpu"`` pipelines over the kernel stand-ins (the GPU half is
tests/test_call_sequences_gpu.py; tests/call_sequences.py holds the table).

Whether a swapped scheduler is mistaken for the old one on the GPU depends on where the caching allocator puts its table and its
step counter, so a green GPU run is weak evidence.  Here the unlucky placement is FORCED -- the new scheduler's device buffers are
the old one's tensors, holding the new contents -- and the key must still differ; likewise a reloaded model and two models
reporting one ``id()``.  The other direction is checked too: a change that only alters the contents of static buffers leaves the
key alone, so it costs no capture."""
import builtins

import pytest
import torch

import call_sequences as CS
import inpaint_emulation
import ops_emulation
from diffusers_amd import ops, pipelines as P

CPU_FAMILIES = ("sd15", "sdxl", "sdxl_img2img", "sd15_inpaint", "flux", "wan", "ddpm")   # (no stand-in for the Flux image encoder path)


@pytest.fixture(autouse=True)
def _emulated_kernels(monkeypatch):
    ops_emulation.install(monkeypatch, ops)
    inpaint_emulation.install(monkeypatch, ops)
    monkeypatch.setattr(ops, "TUNING", False)


def _cases(pick):
    cases = [(f, m) for f, m in CS.CASES if f in CPU_FAMILIES and pick(m)]
    return dict(argvalues=cases, ids=[f"{f}-{m.name}" for f, m in cases])


def _first_call(family, mut):
    fam = CS.FAMILIES[family]
    pipe = fam.build("cpu")
    mut.setup(pipe)
    A = mut.base(fam.kwargs)
    return pipe, A, CS.graph_key_of(pipe, A)


@pytest.mark.parametrize("family,mut", **_cases(lambda m: hasattr(m, "dst")))
def test_a_new_scheduler_at_the_old_addresses_changes_the_key(family, mut):
    """Every hop of the scheduler chains and every same-class swap of the table, with the new scheduler's buffers forced onto the
    old one's addresses: `_table`, `_step_dev` and whatever `graph_buffers` names (DPM-Solver++: begin word and history; UniPC:
    coefficients and history), as far as the two kinds share them."""
    pipe, A, key_old = _first_call(family, mut)
    old = pipe.scheduler
    n = len(old.timesteps)
    mut(pipe, A)
    new = pipe.scheduler
    assert new is not old
    new.set_timesteps(n, device="cpu")
    assert new.device_table.shape == old.device_table.shape          # (DDIM builds its table on first use)
    aliased = CS.alias_scheduler_buffers(new, old)
    assert {"_table", "_step_dev"} <= set(aliased)
    key_new = CS.graph_key_of(pipe, A)
    # the call's own set_timesteps refreshed the aliased buffers in place: the addresses the key reads are the old scheduler's
    assert new.device_table.data_ptr() == old._table.data_ptr() and new.device_step.data_ptr() == old._step_dev.data_ptr()
    assert key_new != key_old, f"{family}: {type(old).__name__} -> {type(new).__name__} at the same addresses replays the old step"
    assert new.graph_token() != old.graph_token()


@pytest.mark.parametrize("family,mut", **_cases(lambda m: m.expect == "recapture" and not hasattr(m, "dst")))
def test_a_change_the_step_bakes_in_changes_the_key(family, mut):
    """Arguments passed by value, shapes, step counts, another model, the same model loaded again."""
    pipe, A, key_a = _first_call(family, mut)
    keep = CS.hold_packed(pipe)              # (a reload must not get its old addresses back by luck)
    key_b = CS.graph_key_of(pipe, mut(pipe, A))
    assert key_b != key_a
    del keep


@pytest.mark.parametrize("family,mut", **_cases(lambda m: m.expect == "replay"))
def test_a_change_of_contents_keeps_the_key(family, mut):
    """The CPU half of "no needless capture": prompt contents, SDXL size conditioning, pooled embeddings, a transposed Flux id grid,
    a LoRA fused in place -- and the key of the first call comes back when the change is undone."""
    pipe, A, key_a = _first_call(family, mut)
    assert CS.graph_key_of(pipe, A) == key_a, "the same call twice"
    B = mut(pipe, A)
    assert CS.graph_key_of(pipe, B) == key_a
    mut.undo(pipe)
    assert CS.graph_key_of(pipe, A) == key_a


@pytest.mark.parametrize("family", ["sd15", "flux", "wan", "ddpm"])
def test_set_timesteps_of_an_unchanged_step_count_keeps_the_key_and_the_addresses(family):
    """What every call does first must stay an in-place refresh: same table, same counter, same key."""
    fam = CS.FAMILIES[family]
    pipe = fam.build("cpu")
    key = CS.graph_key_of(pipe, fam.kwargs)
    sch = pipe.scheduler
    ptrs = (sch.device_table.data_ptr(), sch.device_step.data_ptr())
    assert CS.graph_key_of(pipe, fam.kwargs) == key
    assert (sch.device_table.data_ptr(), sch.device_step.data_ptr()) == ptrs and pipe.scheduler is sch


def _replace(sch, name):
    t = getattr(sch, name)
    setattr(sch, name, tuple(h.clone() for h in t) if isinstance(t, tuple) else t.clone())


@pytest.mark.parametrize("family,kind,buffers", [
    ("sd15", "ddim", ("_table", "_step_dev")), ("sdxl", "euler", ("_table", "_step_dev")),
    ("sdxl", "dpm", ("_table", "_step_dev", "_begin_dev", "_hist")), ("flux", "flowmatch", ("_table", "_step_dev")),
    ("wan", "flowmatch", ("_table", "_step_dev")), ("wan", "unipc", ("_table", "_step_dev", "_coef", "_hist")),
    ("ddpm", "ddpm", ("_table", "_step_dev"))], ids=lambda v: v if isinstance(v, str) else "")
def test_every_device_buffer_of_the_scheduler_is_in_the_key(family, kind, buffers):
    """A captured step holds the raw address of the table, of the step counter and of the sampler's own state (DPM-Solver++: begin
    word and x0 history; UniPC: coefficient table and the three history tensors): whichever of them moves, the key moves."""
    fam = CS.FAMILIES[family]
    pipe = fam.build("cpu")
    table = "sd15" if family == "sd15" else "sdxl" if family == "sdxl" else family
    pipe.scheduler = CS.SCHEDULERS[table][kind]()
    key = CS.graph_key_of(pipe, fam.kwargs)
    for name in buffers:
        _replace(pipe.scheduler, name)
        moved = CS.graph_key_of(pipe, fam.kwargs)
        assert moved != key, f"{family} / {kind}: the key does not carry the address of {name}"
        key = moved


def test_wan_key_carries_the_dtype_of_the_latents():
    """WanPipeline._step branches on it: fp32 latents (UniPC) go through the cast kernel, bf16 ones (FlowMatch-Euler) do not."""
    pipe = CS.FAMILIES["wan"].build("cpu")
    pipe.scheduler.set_timesteps(3, device="cpu")
    lat = torch.zeros((1, 16, 3, 8, 8), dtype=torch.bfloat16)
    same, other = (pipe._make_graph_key(x, {"St": 16}, 5.0, True) for x in (lat, lat.float()))
    assert same == pipe._make_graph_key(lat.clone(), {"St": 16}, 5.0, True) and same != other


@pytest.mark.parametrize("family", ["sd15", "sdxl", "flux", "wan", "ddpm"])
def test_two_models_reporting_one_id_have_different_keys(family, monkeypatch):
    """``id()`` of a collected model can be handed to the next one: the key must tell the two apart by the weights token
    (loading.PretrainedMixin._weights_generation), which no two loads share."""
    fam = CS.FAMILIES[family]
    pipe = fam.build("cpu")
    first = CS.model_of(pipe)
    other = CS.model_of(fam.build("cpu"))                         # same seed: same config, same weights, another object
    monkeypatch.setattr(P, "id", lambda o: 4242 if o is first or o is other else builtins.id(o), raising=False)
    assert P.id(first) == P.id(other)
    key_a = CS.graph_key_of(pipe, fam.kwargs)
    setattr(pipe, CS.model_slot(pipe), other)
    assert CS.graph_key_of(pipe, fam.kwargs) != key_a
    assert P._weights_token(first) != P._weights_token(other)


def test_weights_generation_follows_loads_not_in_place_repacks():
    """The token is bumped by ``load_state_dict`` and left alone by ``_repack_in_place`` (fuse_lora / unfuse_lora), whose fresh CPU
    skeleton draws a number of its own without touching the model's."""
    pipe = CS.FAMILIES["sd15"].build("cpu")
    unet = pipe.unet
    t0 = P._weights_token(unet)
    assert t0 > 0
    mut = next(m for f, m in CS.CASES if f == "sd15" and m.name == "lora_fuse")
    before = {k: v.clone() for k, v in CS.hold_packed(pipe).items()}
    mut(pipe, {})
    assert any(not torch.equal(v, before[k]) for k, v in CS.hold_packed(pipe).items()), "the adapter changed no packed tensor"
    assert P._weights_token(unet) == t0
    mut.undo(pipe)
    assert all(torch.equal(v, before[k]) for k, v in CS.hold_packed(pipe).items()) and P._weights_token(unet) == t0
    unet.load_state_dict(CS._state_dict(unet, 0), device="cpu")
    t1 = P._weights_token(unet)
    assert t1 > t0
    unet.load_state_dict(CS._state_dict(unet, 0), device="cpu")
    assert P._weights_token(unet) > t1
