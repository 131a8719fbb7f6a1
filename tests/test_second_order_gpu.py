"""GPU: the fused two-phase step (da_dpmpp_2m_step with DA_PRED_SECOND_ORDER) and HeunDiscreteScheduler / KDPM2DiscreteScheduler in
the pipelines.

G1 the kernel against the torch fp32 restatement of the header (tests/second_order_emulation.py ``ref_entry``) to the bit, G2 its
footprint, G3 refusals and the unchanged DPM-Solver++ path, G4 predictor + corrector launches against one float64 step, G5 eager ==
captured graph == launch plan in the tiny pipelines and no stale replay, G6 the whole loop against a float64 oracle loop with the
shipped Euler path as the yardstick.

G1 can ask for bits because both sides do the same correctly rounded fp32 operations in the same order (the kernel through
``__f*_rn``, which hipcc may not contract; torch one op at a time) and round the model output's dtype at the same places.  The
guidance scale is 7.5, a bf16 number: torch casts a Python scalar to the tensor dtype before a bf16 op, the kernel keeps it fp32.

G4's bound: two entries of about ten fp32 roundings each against float64, ``EPS32`` = 2^-20 per entry (the rule of
test_dpmsolver_cpu.py), of the largest sample; the rows' own fp32 rounding (2^-24 of sigma and dt) is inside it."""
import math

import numpy as np
import pytest
import torch

import call_sequences as CS
import second_order_emulation as E
from footprint import bits_equal, guarded, poisoned
from second_order_emulation import EPS32

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
bf16 = torch.bfloat16
SD_BETAS = dict(beta_schedule="scaled_linear", beta_start=0.00085, beta_end=0.012)
G = 7.5


def _sched(kind, n, **kw):
    from diffusers_amd.schedulers import HeunDiscreteScheduler, KDPM2DiscreteScheduler
    s = {"heun": HeunDiscreteScheduler, "kdpm2": KDPM2DiscreteScheduler}[kind](**dict(SD_BETAS, **kw))
    s.set_timesteps(n, device=DEV)
    return s


def _inputs(n, row, x_dtype, e_dtype, cfg, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, generator=g) * float(row[3])).to(x_dtype)            # a sample at the row's noise level
    m1 = torch.randn(n, generator=g) * float(row[3])
    e = torch.randn((2 if cfg else 1) * n, generator=g).to(e_dtype)
    return e, x, m1


# ----------------------------------------------------------------------------------------------------------------------
# G1
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x_dtype", [bf16, torch.float32], ids=["x_bf16", "x_f32"])
@pytest.mark.parametrize("e_dtype", [bf16, torch.float32], ids=["e_bf16", "e_f32"])
def test_kernel_equals_the_restated_arithmetic_to_the_bit(x_dtype, e_dtype):
    """n = 1, 3: the tail alone; 4: the vector body alone; 5, 1023, 4099: both (4099: several workgroups); with CFG an n that is no
    multiple of 4 puts the cond half off the 4-wide grid and a base one element into its buffer is not 16-byte aligned: both run
    all-scalar.  Every operand sits in a sentinel-filled buffer: x, m1 and everything around them and around eps is compared."""
    from diffusers_amd import _lib as L, ops
    tables = {"heun": _sched("heun", 4).device_table, "kdpm2": _sched("kdpm2", 4).device_table}
    step = torch.zeros((), dtype=torch.int32, device=DEV)
    PAD = 256
    count = 0
    for n in (1, 3, 4, 5, 1023, 4099):
        for kind, j in (("heun", 6), ("heun", 2), ("heun", 3), ("kdpm2", 2), ("kdpm2", 3)):      # phases 0, 1, 2, 1, 2
            table = tables[kind]
            row = table[j].cpu()
            step.fill_(j)
            for shift, cfg, pred in ((sh, c, p) for sh in ("none", "x", "eps", "m1") for c in (False, True) for p in (0, 1, 2)):
                if kind == "kdpm2" and shift != "none":
                    continue
                e, x, m1 = _inputs(n, row, x_dtype, e_dtype, cfg, 17 * n + j)
                eb = guarded(e.numel(), dtype=e_dtype, lead=PAD + (shift == "eps"), trail=PAD).set(e)
                xb = guarded(n, dtype=x_dtype, lead=PAD + (shift == "x"), trail=PAD).set(x)
                mb = guarded(n, dtype=torch.float32, lead=PAD + (shift == "m1"), trail=PAD).set(m1)
                if shift != "none":
                    assert {"x": xb, "eps": eb, "m1": mb}[shift].ptr() % 16 != 0
                ops.second_order_step_(eb.view, xb.view, mb.view, table, step, step, cfg=cfg, guidance=G, pred_type=pred)
                torch.cuda.synchronize()
                want_x, want_m1 = E.ref_entry(e, x, m1, row, cfg=cfg, guidance=G, pred_type=pred)
                what = (n, kind, j, shift, cfg, pred)
                assert bits_equal(xb.view.cpu(), want_x), what
                assert bits_equal(mb.view.cpu(), want_m1), what
                assert bits_equal(eb.view.cpu(), e), what                                    # the model output is read only
                if int(row[6]) != 1:
                    assert bits_equal(want_m1, m1), what                                     # only a predictor writes the history
                for b, name in ((eb, "eps"), (xb, "x"), (mb, "m1")):
                    b.check(f"second_order {name} {what}")
                count += 1
    print(f"[parity] second-order step {x_dtype} / {e_dtype}: {count} launches bit-identical to the restatement")


# ----------------------------------------------------------------------------------------------------------------------
# G2
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("j", [2, 3], ids=["predictor", "corrector"])
@pytest.mark.parametrize("n,cfg", [(4099, False), (4 * 1023, True)])
def test_footprint_of_a_predictor_and_a_corrector_launch(j, n, cfg):
    """Mebibyte guard bands of NaN sentinels around eps, x and m1: nothing outside the operands is written, and nothing outside them is
    read into the result (the run on zero-surrounded copies gives the same bits)."""
    from diffusers_amd import ops
    table = _sched("heun", 4).device_table
    step = torch.full((), j, dtype=torch.int32, device=DEV)
    e, x, m1 = _inputs(n, table[j].cpu(), bf16, bf16, cfg, 5)
    outs = []
    for clean in (False, True):
        bufs = [poisoned(v) for v in (e, x, m1)]
        if clean:
            bufs = [b.clean() for b in bufs]
        eb, xb, mb = bufs
        ops.second_order_step_(eb.view, xb.view, mb.view, table, step, step, cfg=cfg, guidance=G)
        torch.cuda.synchronize()
        for b, name in ((eb, "eps"), (xb, "x"), (mb, "m1")):
            b.check(f"second_order footprint {name} entry {j} n{n}")
        assert torch.isfinite(xb.view.float()).all() and torch.isfinite(mb.view).all()
        outs.append((xb.view.cpu(), mb.view.cpu()))
    assert bits_equal(outs[0][0], outs[1][0]) and bits_equal(outs[0][1], outs[1][1])
    want_x, want_m1 = E.ref_entry(e, x, m1, table[j].cpu(), cfg=cfg, guidance=G)
    assert bits_equal(outs[0][0], want_x) and bits_equal(outs[0][1], want_m1)


# ----------------------------------------------------------------------------------------------------------------------
# G3
# ----------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_unchanged_dpmpp_path():
    from diffusers_amd import _lib as L, ops
    import test_dpmsolver_cpu as D
    lib = L.load()
    s = _sched("heun", 4)
    n = 64
    e, x, m1 = _inputs(n, s.device_table[2].cpu(), torch.float32, torch.float32, False, 9)
    ed, xd, md = e.to(DEV), x.to(DEV), m1.to(DEV)
    st = s.device_step
    p = dict(eps=ed.data_ptr(), x=xd.data_ptr(), m1=md.data_ptr(), table=s.device_table.data_ptr(), step=st.data_ptr(), begin=st.data_ptr())

    def call(pred_type, n_=n, **null):
        a = dict(p, **{k: None for k in null})
        return lib.da_dpmpp_2m_step(a["eps"], a["x"], a["m1"], a["table"], a["step"], a["begin"], 0, 0.0, n_, L.DTYPE_F32, L.DTYPE_F32,
                                    pred_type, None)

    INVALID = 1
    for name in p:                                                       # null pointers, n <= 0: refused before any launch
        assert call(L.PRED_SECOND_ORDER, **{name: True}) == INVALID, name
    assert call(L.PRED_SECOND_ORDER, n_=0) == INVALID and call(L.PRED_SECOND_ORDER + 2, n_=-4) == INVALID
    for bad in (11, 3, 4, 5, 6, 7, 12, 16, 24, -1, -8):                   # 11 is the flag with a prediction type that does not exist
        assert call(bad) == INVALID, bad
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), x) and torch.equal(md.cpu(), m1)        # nothing ran
    with pytest.raises(ValueError, match="pred_type"):
        ops.second_order_step_(ed, xd, md, s.device_table, st, st, pred_type=L.PRED_SECOND_ORDER)
    with pytest.raises(ValueError):                                      # the history is fp32, of the sample's size
        ops.second_order_step_(ed, xd, md.to(bf16), s.device_table, st, st)
    with pytest.raises(ValueError):
        ops.second_order_step_(ed, xd, md[:32], s.device_table, st, st)
    with pytest.raises(ValueError):                                      # [2 x sample] with cfg
        ops.second_order_step_(ed, xd, md, s.device_table, st, st, cfg=True, guidance=5.0)
    with pytest.raises((ValueError, RuntimeError)):                      # host tensors have no path
        ops.second_order_step_(e, x, m1, s.device_table, st, st)
    # 0..2 run the DPM-Solver++ kernel they ran: on fp32 tensors its stand-in does the same fp32 ops in the same order
    from diffusers_amd.schedulers import DPMSolverMultistepScheduler
    d = DPMSolverMultistepScheduler(**SD_BETAS, use_karras_sigmas=True)
    d.set_timesteps(8, device=DEV)
    step = torch.full((), 3, dtype=torch.int32, device=DEV)
    begin = torch.zeros((), dtype=torch.int32, device=DEV)
    assert float(d.device_table[3, 6]) == 1.0                            # a second-order row
    for pred in (0, 1, 2):
        xd, md = x.clone().to(DEV), m1.clone().to(DEV)
        ops.dpmpp_2m_step_(ed, xd, md, d.device_table, step, begin, pred_type=pred)
        xc, mc = x.clone(), m1.clone()
        D.dpmpp_2m_step_(e, xc, mc, d.device_table.cpu(), 3, 0, pred_type=pred)
        assert bits_equal(xd.cpu(), xc) and bits_equal(md.cpu(), mc), pred


# ----------------------------------------------------------------------------------------------------------------------
# G4
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["heun", "kdpm2"])
@pytest.mark.parametrize("pred", E.PREDS)
def test_a_corrector_reads_what_its_predictor_wrote(kind, pred):
    """Two launches, the device step counter advanced by da_advance_step between them, against ONE float64 step of the published
    algorithm; then the history is bit for bit what the predictor left."""
    from diffusers_amd import _lib as L, ops
    n_el = 4099
    s = _sched(kind, 5, use_karras_sigmas=True, prediction_type=pred)
    ts, sig = E.ref_ladder(5, ladder="karras", **SD_BETAS)
    g = torch.Generator().manual_seed(23)
    for i in (0, 2, 3):
        x = (torch.randn(n_el, generator=g) * math.sqrt(sig[i] ** 2 + 1)).float()
        es = [torch.randn(n_el, generator=g).float() for _ in range(2)]
        xd, md = x.clone().to(DEV), torch.full((n_el,), float("nan"), device=DEV)             # a corrector that read stale history shows
        step = torch.full((), 2 * i, dtype=torch.int32, device=DEV)
        ops.second_order_step_(es[0].to(DEV), xd, md, s.device_table, step, step, pred_type=L.PRED_TYPES[pred])
        hist = md.clone()
        ops.advance_step(step)
        ops.second_order_step_(es[1].to(DEV), xd, md, s.device_table, step, step, pred_type=L.PRED_TYPES[pred])
        torch.cuda.synchronize()
        assert int(step) == 2 * i + 1 and bits_equal(md, hist) and torch.isfinite(hist).all()
        model = lambda x_, s_, j: es[j % 2].double().numpy()          # noqa: E731
        want = E.STEPS[kind](x.double().numpy(), model, float(sig[i]), float(sig[i + 1]), pred, at=(0, 1))
        err = np.abs(xd.double().cpu().numpy() - want).max()
        bound = 2 * EPS32 * float(x.abs().max())
        print(f"[parity] {kind} {pred} step {i}: predictor + corrector vs float64, error / bound = {err / bound:.3f}")
        assert err <= bound, (i, err, bound)


# ----------------------------------------------------------------------------------------------------------------------
# pipelines
# ----------------------------------------------------------------------------------------------------------------------
def _pipe(kind, scheduler, **kw):
    from diffusers_amd import factory
    build = factory.build_sdxl_pipeline if kind == "sdxl" else factory.build_sd15_pipeline
    return build(device=DEV, tiny=True, seed=0, scheduler=scheduler, **kw)


def _kw(kind, seed=0, steps=4, gs=5.0, latents=True):
    g = torch.Generator().manual_seed(seed)
    kw = dict(prompt_embeds=torch.randn(1, 7, 64, generator=g).to(bf16), negative_prompt_embeds=torch.randn(1, 7, 64, generator=g).to(bf16),
              num_inference_steps=steps, guidance_scale=gs, output_type="latent")
    if latents:
        kw["latents"] = torch.randn(1, 4, 16, 16, generator=g).to(bf16)
    if kind == "sdxl":
        kw.update(pooled_prompt_embeds=torch.randn(1, 64, generator=g).to(bf16),
                  negative_pooled_prompt_embeds=torch.randn(1, 64, generator=g).to(bf16))
    return kw


def _image(seed=11, hw=32):
    return torch.rand(1, 3, hw, hw, generator=torch.Generator().manual_seed(seed))


def _three_identities(build, call, other_seed_call, changed_call):
    """eager == HIP graph == launch plan to the bit; a call that differs only in what the captured step reads from static buffers
    (``other_seed_call``) replays the captured step; ``changed_call`` (n = 3, another seed, another guidance scale) on the used
    pipelines equals a fresh pipeline's eager result.  Returns (the graph pipeline, the eager one)."""
    ep = build()
    eager = CS.run(ep, call, False)
    assert torch.isfinite(eager.float()).all()
    pipe = build()
    assert torch.equal(CS.run(pipe, call, True), eager)
    g0 = pipe._graph
    other = CS.run(pipe, other_seed_call, True)
    assert pipe._graph is g0 and not torch.equal(other, eager)
    assert torch.equal(other, CS.run(ep, other_seed_call, False))
    fresh = CS.run(build(), changed_call, False)
    assert torch.equal(CS.run(pipe, changed_call, True), fresh)
    assert torch.equal(CS.run(pipe, call, True), eager)                  # and back, on the history the other loops left
    plan = build()
    assert torch.equal(CS.run(plan, call, "plan"), eager)
    assert torch.equal(CS.run(plan, changed_call, "plan"), fresh)
    return pipe, ep


@pytest.mark.parametrize("scheduler", ["heun", "kdpm2"])
def test_text_to_image_eager_graph_and_plan_are_bit_identical(scheduler):
    kw = dict(_kw("sdxl"), height=32, width=32)
    pipe, ep = _three_identities(lambda: _pipe("sdxl", scheduler), kw, dict(kw, latents=_kw("sdxl", seed=5)["latents"]),
                                 dict(_kw("sdxl", seed=9, steps=3, gs=7.0), height=32, width=32))
    n = []
    pipe(use_graph=True, callback_on_step_end=lambda p, i, t, d: n.append(float(t)) or {}, **CS.materialise(kw, DEV))
    assert n == pipe.scheduler.timesteps.tolist() and len(n) == 7 and pipe.scheduler.step_index == 7     # once per entry
    for extra in (dict(guidance_rescale=0.7), dict(guidance_scale=1.0), dict(num_inference_steps=6, denoising_end=0.5)):
        call = dict(kw, **extra)
        assert torch.equal(CS.run(pipe, call, True), CS.run(ep, call, False)), sorted(extra)


@pytest.mark.parametrize("flavour", ["img2img", "inpaint", "controlnet", "pix2pix"])
def test_the_other_pipelines_with_heun(flavour):
    gen = lambda seed: (lambda: torch.Generator().manual_seed(seed))     # noqa: E731
    if flavour == "img2img":
        build = lambda: _pipe("sdxl", "heun", img2img=True)              # noqa: E731
        base = dict(_kw("sdxl", latents=False), image=_image(), strength=0.75)                # 3 of 4 steps: entries 2 .. 6
    elif flavour == "inpaint":
        build = lambda: _pipe("sdxl", "heun", inpaint=True, unet_in_channels=4)               # noqa: E731
        mask = torch.zeros(32, 32)
        mask[8:24, 4:20] = 1.0
        base = dict(_kw("sdxl", latents=False), image=_image(), mask_image=mask, strength=1.0)
    elif flavour == "controlnet":
        build = lambda: _pipe("sdxl", "heun", controlnet=True)           # noqa: E731
        base = dict(_kw("sdxl"), image=_image())
    else:
        build = lambda: _pipe("sdxl", "heun", pix2pix=True)              # noqa: E731
        base = dict(_kw("sdxl", gs=7.5, latents=False), image=_image(4, 64), image_guidance_scale=1.5)
    seeded = "latents" not in base
    call = dict(base, generator=gen(21)) if seeded else base
    other = dict(base, generator=gen(22)) if seeded else dict(base, latents=_kw("sdxl", seed=5)["latents"])
    changed = dict(call, num_inference_steps=3, guidance_scale=base["guidance_scale"] + 2.0)
    changed.update(dict(generator=gen(23)) if seeded else dict(latents=_kw("sdxl", seed=6)["latents"]))
    _three_identities(build, call, other, changed)


# ----------------------------------------------------------------------------------------------------------------------
# G6
# ----------------------------------------------------------------------------------------------------------------------
def _rel_rms(a, b):
    a, b = a.double().cpu().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


def test_pipeline_loop_against_a_float64_oracle_loop_with_euler_as_the_yardstick():
    """Final latents of the tiny SDXL pipeline (CFG, captured graph) against a loop written here that calls the same engine U-Net
    once per entry (bf16 only at its input and output) and does the sampler arithmetic in float64 from the float64 ladder: Heun and
    DPM2 with n = 4 (7 model calls), and -- the yardstick, code that shipped before these samplers -- EulerDiscreteScheduler with 7
    steps on the same pipeline, seed and prompt.  Bf16 latents through a U-Net have no derivable bound; required is at most 2x
    Euler's relative RMS error (2x: the U-Net amplifies bf16 storage differences differently along another trajectory)."""
    from diffusers_amd import factory
    from diffusers_amd.schedulers import EulerDiscreteScheduler
    gs = 5.0
    kw = dict(_kw("sdxl", gs=gs), height=32, width=32)
    lat = kw["latents"]
    ehs = torch.cat([kw["negative_prompt_embeds"], kw["prompt_embeds"]]).to(DEV)
    ids = torch.tensor([[32, 32, 0, 0, 32, 32]], dtype=torch.float32, device=DEV).repeat(2, 1)
    added = {"text_embeds": torch.cat([kw["negative_pooled_prompt_embeds"], kw["pooled_prompt_embeds"]]).to(DEV), "time_ids": ids}
    sig_all = E.ref_training_sigmas(**SD_BETAS)
    vals = {}
    for which, n in (("heun", 4), ("kdpm2", 4), ("euler", 7)):
        pipe = _pipe("sdxl", None if which == "euler" else which)
        if which == "euler":
            assert type(pipe.scheduler) is EulerDiscreteScheduler and dict(factory.SDXL_SCHEDULER) == dict(factory.SECOND_ORDER_SCHEDULER)
        got = CS.run(pipe, dict(kw, num_inference_steps=n), True)
        ts, sig = E.ref_ladder(n, spacing="leading", steps_offset=1, sig_all=sig_all)
        t_of = ts.repeat(2) if which == "euler" else E.entries(which, ts, sig, sig_all)[:, 7]       # entry tag -> model timestep

        def model(x, sigma, j):
            xin = torch.from_numpy(x / math.sqrt(sigma * sigma + 1)).to(bf16).reshape(1, 4, 16, 16)
            xin = torch.cat([xin, xin]).to(DEV).contiguous()
            out = pipe.unet(xin, float(np.float32(t_of[j])), encoder_hidden_states=ehs, added_cond_kwargs=added,
                            return_dict=False)[0].double().cpu().numpy()
            return (out[0] + gs * (out[1] - out[0])).reshape(-1)

        x0 = lat.double().numpy().reshape(-1) * math.sqrt(sig[0] ** 2 + 1)                     # leading spacing: init_noise_sigma
        want = E.ref_loop(which, x0, model, sig)
        vals[which] = _rel_rms(got, want)
        assert torch.isfinite(got.float()).all()
    line = (f"[parity] tiny sdxl, engine pipeline (bf16 latents, fused step) vs float64 oracle loop: rel_rms Heun n=4 {vals['heun']:.3e}, "
            f"DPM2 n=4 {vals['kdpm2']:.3e}, Euler 7 steps {vals['euler']:.3e}")
    print(line)
    assert vals["heun"] <= 2.0 * vals["euler"] and vals["kdpm2"] <= 2.0 * vals["euler"], line
