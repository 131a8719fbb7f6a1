"""GPU: da_euler_ancestral_step and EulerAncestralDiscreteScheduler in the SD / SDXL pipelines.

G1 one step, bit for bit against ``ref_step`` of tests/test_euler_ancestral_cpu.py (the reference's op chain with torch CPU ops: the
same IEEE operations in the same order, so the gate is ``torch.equal``), noise from a 20-row table and in the stride-0 form, ``out``
aliasing the sample; G2 the scalar tail and unaligned bases inside sentinel-filled over-allocations (tests/footprint.py); G3 eager ==
captured graph == launch plan in the tiny pipelines (text-to-image, img2img, inpainting, the base / refiner hand-off, guidance_rescale,
no CFG, one trailing step); G4 the pipeline's loop against a test-side fp32 loop with the Euler path as the yardstick."""
import numpy as np
import pytest
import torch

import footprint
from test_euler_ancestral_cpu import SD_BETAS, ref_step_row

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
bf16 = torch.bfloat16
PRED = {"epsilon": 0, "v_prediction": 1}


def _sched(n, **kw):
    from diffusers_amd.schedulers import EulerAncestralDiscreteScheduler
    cfg = dict(SD_BETAS)
    cfg.update(kw)
    s = EulerAncestralDiscreteScheduler(**cfg)
    s.set_timesteps(n, device=DEV)
    return s


# ----------------------------------------------------------------------------------------------------------------------
# G1
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 4, 9, 7), (2, 4, 32, 32)])
@pytest.mark.parametrize("dtype", [bf16, torch.float32], ids=["bf16", "f32"])
def test_one_step_is_bit_identical_to_the_restated_op_chain(shape, dtype):
    from diffusers_amd import ops
    g = torch.Generator().manual_seed(11)
    n = int(np.prod(shape))
    x = torch.randn(shape, generator=g)
    e2 = torch.randn((2,) + shape, generator=g).to(dtype)
    noise = torch.randn((20,) + shape, generator=g).to(dtype)           # every row differs
    noise_d, step = noise.to(DEV), torch.zeros((), dtype=torch.int32, device=DEV)
    checked = 0
    for pred in ("epsilon", "v_prediction"):
        s = _sched(20, prediction_type=pred)
        table = s.device_table
        rows = table.cpu()
        for r, (cfg, gs) in ((r, c) for r in (0, 9, 19) for c in ((False, 0.0), (True, 5.0), (True, 7.5))):
            xs = (x * float(rows[r, 0] + 1.0)).to(dtype)                # a sample at the row's noise level
            ee = (e2 if cfg else e2[1]).contiguous()
            want = ref_step_row(ee, xs, noise[r], rows[r], cfg=cfg, guidance=gs, pred_type=PRED[pred])
            step.fill_(r)
            xd, ed = xs.to(DEV), ee.to(DEV)
            what = (shape, str(dtype), pred, r, cfg, gs)
            got = ops.euler_ancestral_step(ed, xd, noise_d, table, step, cfg=cfg, guidance=gs, pred_type=PRED[pred],
                                           noise_step_stride=n)
            assert got.dtype == dtype and got.data_ptr() != xd.data_ptr() and torch.equal(xd.cpu(), xs), what
            assert torch.equal(got.cpu(), want), what
            if r != 19:     # ... fed row `step` and no other row (the last row adds no noise: sigma_up = 0)
                other = ref_step_row(ee, xs, noise[(r + 1) % 20], rows[r], cfg=cfg, guidance=gs, pred_type=PRED[pred])
                assert not torch.equal(got.cpu(), other), what
            else:
                assert float(rows[r, 6]) == 0.0
            # the stride-0 single-row form
            one = ops.euler_ancestral_step(ed, xd, noise_d[r].contiguous(), table, step, cfg=cfg, guidance=gs, pred_type=PRED[pred])
            assert torch.equal(one, got), what
            # `out` aliasing the sample gives the same bits
            alias = xd.clone()
            ret = ops.euler_ancestral_step(ed, alias, noise_d, table, step, cfg=cfg, guidance=gs, out=alias, pred_type=PRED[pred],
                                           noise_step_stride=n)
            assert ret.data_ptr() == alias.data_ptr() and torch.equal(alias, got), what
            assert torch.equal(ed.cpu(), ee) and torch.equal(noise_d.cpu(), noise), what         # inputs are read only
            checked += 1
    assert checked == 18


def test_scheduler_step_and_the_custom_op():
    """step() draws its noise as the reference does (on the generator's device, in the model output's dtype) and advances; the
    torch.library op is the functional form of the same launch."""
    from diffusers_amd import ops
    import diffusers_amd.torch_ops  # noqa: F401
    s = _sched(6)
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(1, 4, 8, 8, generator=g) * s.sigmas[0]).to(bf16)
    e = torch.randn(1, 4, 8, 8, generator=g).to(bf16)
    rows = s.device_table.cpu()
    gen = torch.Generator().manual_seed(9)
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(9), dtype=bf16)
    out = s.step(e.to(DEV), s.timesteps[0], x.to(DEV), generator=gen).prev_sample
    assert torch.equal(out.cpu(), ref_step_row(e, x, noise, rows[0])) and s.step_index == 1 and int(s.device_step) == 1
    s.reset(2)
    fn = torch.ops.mi355x.euler_ancestral_step(e.to(DEV), x.to(DEV), noise.to(DEV), s.device_table, s.device_step, False, 0.0, 0, 0)
    assert torch.equal(fn.cpu(), ref_step_row(e, x, noise, rows[2]))
    xd, ed, nd = x.to(DEV), e.to(DEV), noise.to(DEV)
    with pytest.raises(ValueError):                 # [2 x sample] with cfg
        ops.euler_ancestral_step(ed, xd, nd, s.device_table, s.device_step, cfg=True, guidance=5.0)
    with pytest.raises(ValueError):                 # the noise has the model output's dtype
        ops.euler_ancestral_step(ed, xd, nd.float(), s.device_table, s.device_step, cfg=False, guidance=0.0)
    with pytest.raises(ValueError):                 # a table of 6 rows, stride numel: 6 x numel elements
        ops.euler_ancestral_step(ed, xd, nd, s.device_table, s.device_step, cfg=False, guidance=0.0, noise_step_stride=x.numel())
    with pytest.raises(ValueError):                 # host tensors have no path
        ops.euler_ancestral_step(e, x, noise, s.device_table, s.device_step, cfg=False, guidance=0.0)
    with pytest.raises(ValueError, match="noise_table"):
        s.step_cfg(torch.cat([ed, ed]), xd, 5.0, out=xd)


# ----------------------------------------------------------------------------------------------------------------------
# G2
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [bf16, torch.float32], ids=["bf16", "f32"])
def test_scalar_tail_and_unaligned_bases(dtype):
    """Element counts with n % 4 in {1, 2, 3} run the 4-wide body plus a scalar tail without CFG and the all-scalar path with CFG
    (the cond half starts n elements in); an operand that starts one element into its allocation is not 16-byte aligned and makes
    the launch all-scalar.  Every operand lives in a sentinel-filled (NaN) buffer: the bands around it must be untouched, and a stray
    read would make the result non-finite."""
    from diffusers_amd import ops
    g = torch.Generator().manual_seed(13)
    band = footprint.MIN_BAND_BYTES // (2 if dtype == bf16 else 4)
    r = 10
    step = torch.full((), r, dtype=torch.int32, device=DEV)
    tables = {p: _sched(20, prediction_type=p).device_table for p in PRED}
    for n in (105, 106, 107, 12297):                                    # n % 4 = 1, 2, 3, 1 (the last: several workgroups + a tail)
        x = (torch.randn(n, generator=g) * 3.0).to(dtype)
        e2 = torch.randn(2, n, generator=g).to(dtype)
        nz = torch.randn(n, generator=g).to(dtype)
        for shift, (cfg, gs), pred in ((sh, c, p) for sh in ("none", "x", "eps", "noise", "out") for c in ((False, 0.0), (True, 7.5))
                                       for p in PRED):
            ee = (e2 if cfg else e2[1]).contiguous()
            box = {}
            for name, vals in (("x", x), ("eps", ee.reshape(-1)), ("noise", nz), ("out", torch.zeros(n, dtype=dtype))):
                box[name] = footprint.guarded(vals.numel(), dtype=dtype, lead=band + int(shift == name), device=DEV).set(vals)
                assert (box[name].ptr() % 16 != 0) == (shift == name)
            table = tables[pred]
            what = (n, str(dtype), shift, cfg, pred)
            got = ops.euler_ancestral_step(box["eps"].view.view(ee.shape), box["x"].view, box["noise"].view, table, step, cfg=cfg,
                                           guidance=gs, out=box["out"].view, pred_type=PRED[pred])
            torch.cuda.synchronize()
            want = ref_step_row(ee, x, nz, table[r].cpu(), cfg=cfg, guidance=gs, pred_type=PRED[pred])
            assert got.data_ptr() == box["out"].ptr() and torch.equal(got.cpu(), want), what
            for name in box:
                box[name].check(f"{name} {what}")
            assert torch.equal(box["eps"].view.cpu(), ee.reshape(-1)) and torch.equal(box["noise"].view.cpu(), nz), what
            assert torch.equal(box["x"].view.cpu(), x), what


# ----------------------------------------------------------------------------------------------------------------------
# pipelines
# ----------------------------------------------------------------------------------------------------------------------
def _embeds(seed, B, seq, dim, pooled):
    g = torch.Generator().manual_seed(seed)
    pe, npe = (torch.randn(B, seq, dim, generator=g).to(bf16) for _ in range(2))
    te, nte = (torch.randn(B, pooled, generator=g).to(bf16) for _ in range(2)) if pooled else (None, None)
    return pe, npe, te, nte


def _cross_dim(pipe):
    d = pipe.unet.config.cross_attention_dim
    return d if isinstance(d, int) else d[0]


def _pipe(kind, scheduler="euler_a", spacing=None, **build_kw):
    from diffusers_amd import factory
    from diffusers_amd.schedulers import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler
    build = factory.build_sdxl_pipeline if kind == "sdxl" else factory.build_sd15_pipeline
    pipe = build(device=DEV, tiny=True, seed=0, **build_kw)
    if scheduler == "euler_a":
        cfg = dict(factory.SDXL_EULER_A_SCHEDULER if kind == "sdxl" else factory.SD15_EULER_A_SCHEDULER)
        if spacing:
            cfg["timestep_spacing"] = spacing
        pipe.scheduler = EulerAncestralDiscreteScheduler(**cfg)
    else:
        pipe.scheduler = EulerDiscreteScheduler(**factory.SDXL_SCHEDULER)
    pe, npe, te, nte = _embeds(3, 1, 7, 64 if kind == "sdxl" else _cross_dim(pipe), 64 if kind == "sdxl" else 0)
    emb = dict(prompt_embeds=pe.to(DEV), negative_prompt_embeds=npe.to(DEV), output_type="latent")
    if kind == "sdxl":
        emb.update(pooled_prompt_embeds=te.to(DEV), negative_pooled_prompt_embeds=nte.to(DEV))
    return pipe, emb, (pe, npe, te, nte)


def _lat(seed):
    return torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(seed)).to(bf16).to(DEV)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------------------------------------------------------------------
# G3
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
def test_eager_graph_and_plan_replay_are_bit_identical(kind):
    pipe, emb, _ = _pipe(kind)

    def run(mode, seed, steps=8, **kw):
        out = pipe(latents=_lat(seed), generator=_gen(100 + seed), num_inference_steps=steps, guidance_scale=5.0, height=32, width=32,
                   use_graph=mode, **emb, **kw).images.clone()
        torch.cuda.synchronize()
        return out

    eager = run(False, 8)
    assert torch.isfinite(eager.float()).all()
    for mode in (True, "plan"):
        assert torch.equal(run(mode, 8), eager), mode
        graph = pipe._graph
        other = run(mode, 9)                                    # other latents, another seed, same step count: no re-capture
        assert pipe._graph is graph, mode
        assert torch.equal(other, run(False, 9)) and not torch.equal(other, eager), mode
        assert torch.equal(run(mode, 8, steps=11), run(False, 8, steps=11)), mode       # another step count
        assert torch.equal(run(mode, 8), eager), mode
    # the noise matters: the same latents with another generator seed give another image
    assert not torch.equal(pipe(latents=_lat(8), generator=_gen(1), num_inference_steps=8, guidance_scale=5.0, height=32, width=32,
                                use_graph=False, **emb).images, eager)


@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
def test_img2img_replay_is_bit_identical(kind):
    """strength 0.5 of 8 steps starts at row 4, strength 0.75 at row 2: both replay one captured step, which reads the table row and
    the noise row of the device step counter."""
    pipe, emb, _ = _pipe(kind, img2img=True)
    img = torch.rand(1, 3, 32, 32, generator=_gen(4))

    def run(mode, strength=0.5):
        n = []
        out = pipe(image=img, strength=strength, num_inference_steps=8, guidance_scale=5.0, use_graph=mode, generator=_gen(21),
                   callback_on_step_end=lambda p, i, t, d: n.append(float(t)) or {}, **emb).images.clone()
        torch.cuda.synchronize()
        return out, n

    eager, ts = run(False)
    assert len(ts) == 4 and ts == pipe.scheduler.timesteps[4:].tolist() and torch.isfinite(eager.float()).all()
    for mode in (True, "plan"):
        assert torch.equal(run(mode)[0], eager), mode
        graph = pipe._graph
        out75, ts75 = run(mode, strength=0.75)
        assert pipe._graph is graph and len(ts75) == 6
        assert torch.equal(out75, run(False, strength=0.75)[0]), mode
        assert torch.equal(run(mode)[0], eager), mode


@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
def test_inpainting_with_a_4_channel_unet_eager_equals_graph(kind):
    pipe, emb, _ = _pipe(kind, inpaint=True, unet_in_channels=4)
    img = torch.rand(1, 3, 32, 32, generator=_gen(4))
    mask = torch.zeros(32, 32)
    mask[8:24, 4:20] = 1.0
    outs = [pipe(image=img, mask_image=mask, strength=0.75, num_inference_steps=8, guidance_scale=5.0, use_graph=mode,
                 generator=_gen(21), **emb).images.clone() for mode in (False, True)]
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0].float()).all() and torch.equal(outs[0], outs[1])


def test_base_to_refiner_handoff_eager_graph_and_plan():
    from diffusers_amd.pipelines import StableDiffusionXLImg2ImgPipeline
    base, emb, _ = _pipe("sdxl")
    ref = StableDiffusionXLImg2ImgPipeline(vae=base.vae, unet=base.unet, scheduler=base.scheduler)
    outs = []
    for mode in (False, True, "plan"):
        mid = base(latents=_lat(8), generator=_gen(31), num_inference_steps=10, guidance_scale=5.0, height=32, width=32,
                   denoising_end=0.8, use_graph=mode, **emb).images.clone()
        outs.append(ref(image=mid, generator=_gen(32), num_inference_steps=10, denoising_start=0.8, guidance_scale=5.0,
                        use_graph=mode, **emb).images.clone())
        assert 0 < ref.scheduler.begin_index < 10
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and torch.isfinite(outs[0].float()).all()


@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
@pytest.mark.parametrize("kw", [dict(guidance_scale=5.0, guidance_rescale=0.7), dict(guidance_scale=1.0)], ids=["rescale", "no_cfg"])
def test_guidance_rescale_and_no_cfg(kind, kw):
    pipe, emb, _ = _pipe(kind)
    outs = [pipe(latents=_lat(8), generator=_gen(41), num_inference_steps=8, height=32, width=32, use_graph=mode, **kw, **emb).images.clone()
            for mode in (False, True)]
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0].float()).all() and torch.equal(outs[0], outs[1])


def test_one_trailing_step_without_guidance():
    """The few-step configuration: timestep_spacing="trailing", one step, guidance_scale = 0.  The only row is the last one
    (sigma_up = 0): the result is the model's x0 at t = 999."""
    pipe, emb, _ = _pipe("sdxl", spacing="trailing")
    outs = [pipe(latents=_lat(8), generator=_gen(51), num_inference_steps=1, guidance_scale=0.0, height=32, width=32, use_graph=mode,
                 **emb).images.clone() for mode in (False, True)]
    torch.cuda.synchronize()
    assert pipe.scheduler.timesteps.tolist() == [999.0]
    assert torch.isfinite(outs[0].float()).all() and torch.equal(outs[0], outs[1])


# ----------------------------------------------------------------------------------------------------------------------
# G4
# ----------------------------------------------------------------------------------------------------------------------
def _rel_rms(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
def test_pipeline_loop_against_a_test_side_fp32_loop_with_euler_as_the_yardstick(kind):
    """The engine pipeline (bf16 latents, the fused step, a seeded generator) against a loop written here: fp32 latents (bf16 only at
    the U-Net's input), the scheduler restated in float64, the same noise rows read back from the pipeline's table.  Eight bf16-latent
    steps through a random-weight U-Net have no derivable bound; both paths round the latents once per step, the ancestral trajectory
    differs from Euler's, and 2x the same quantity measured for EulerDiscreteScheduler (through oracle.samplers.EulerOracle, in this
    test) is the allowance the project gives a different trajectory."""
    from oracle.samplers import EulerOracle
    from diffusers_amd import factory
    steps, gs = 8, 5.0
    lat = _lat(8)
    vals = {}
    for which in ("euler_a", "euler"):
        pipe, emb, (pe, npe, te, nte) = _pipe(kind, scheduler=which)
        got = pipe(latents=lat.clone(), generator=_gen(61), num_inference_steps=steps, guidance_scale=gs, height=32, width=32,
                   use_graph=True, **emb).images.clone()
        ehs = torch.cat([npe, pe]).to(DEV)
        added = None
        if kind == "sdxl":
            ids = torch.tensor([[32, 32, 0, 0, 32, 32]], dtype=torch.float32, device=DEV).repeat(2, 1)
            added = {"text_embeds": torch.cat([nte, te]).to(DEV), "time_ids": ids}

        def eps_of(x_in, t):
            xin = torch.cat([x_in, x_in]).to(bf16).to(DEV).contiguous()
            out = pipe.unet(xin, float(t), encoder_hidden_states=ehs, added_cond_kwargs=added, return_dict=False)[0].float().cpu()
            return out[:1] + gs * (out[1:] - out[:1])

        if which == "euler_a":
            sch = pipe.scheduler
            sig, ts = sch.sigmas.double().numpy(), sch.timesteps.tolist()
            noise = pipe._noise_table.double().cpu().numpy()
            assert noise.shape[0] == steps
            x = lat.float().cpu().double().numpy() * float(sch.init_noise_sigma)
            for i in range(steps):
                s, to = sig[i], sig[i + 1]
                e = eps_of(torch.from_numpy(x / np.sqrt(s * s + 1.0)).float(), ts[i]).double().numpy()
                up = np.sqrt(to ** 2 * (s ** 2 - to ** 2) / s ** 2)
                down = np.sqrt(to ** 2 - up ** 2)
                x = x + e * (down - s) + noise[i] * up          # (x - x0) / sigma = e for an epsilon model
            want = torch.from_numpy(x)
        else:
            o = EulerOracle(**factory.SDXL_SCHEDULER)
            o.set_timesteps(steps)
            x = lat.float().cpu() * o.init_noise_sigma
            for t in o.timesteps:
                x = o.step(eps_of(o.scale_model_input(x), t), x)
            want = x
        vals[which] = _rel_rms(got, want)
        assert torch.isfinite(got.float()).all()
    line = (f"[parity] tiny {kind} {steps} steps, engine pipeline (bf16 latents) vs fp32 loop: rel_rms Euler ancestral "
            f"{vals['euler_a']:.3e}, Euler {vals['euler']:.3e}, ratio {vals['euler_a'] / vals['euler']:.2f}")
    print(line)             # (the lines of one run on an MI355X are kept in profiles/euler_ancestral_gpu_suite_parity_lines.txt)
    assert vals["euler_a"] <= 2.0 * vals["euler"], line
