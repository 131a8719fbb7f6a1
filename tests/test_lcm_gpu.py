"""GPU: the consistency update behind da_x0_linear_step, LCMScheduler in the SD / SDXL pipelines, the U-Net's ``timestep_cond``.

G1 one step, bit for bit against ``ref_step_row`` of tests/lcm_emulation.py (the reference's op chain with every rounding explicit:
the same IEEE operations in the same order, so the gate is ``torch.equal``); G2 the scalar tail and unaligned bases inside
sentinel-filled over-allocations (tests/footprint.py); G3 ``pred_type`` 0-2 unchanged; G4 eager == captured graph == launch plan in the
tiny pipelines; G5 the U-Net with ``time_cond_proj_dim`` against the fp32 oracle; G6 the pipeline's loop against a test-side fp32 loop
with the Euler path as the yardstick."""
import numpy as np
import pytest
import torch

import footprint
import lcm_emulation as E
import ops_emulation

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
bf16 = torch.bfloat16
PREDS = {"epsilon": 4, "v_prediction": 5, "sample": 6}


def _rows(clip):
    """A middle row and a final row, hand-made so that both terms of ``denoised`` matter: c_out = 0.9, c_skip = 0.3."""
    mid = [0.6, 0.8, 0.9, 0.3, 0.95, 0.3125, clip, 499.0]
    fin = [0.6, 0.8, 0.9, 0.3, 1.0, 0.0, clip, 259.0]
    return torch.tensor([mid, fin, mid, fin], dtype=torch.float32)


# ----------------------------------------------------------------------------------------------------------------------
# G1
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 4, 9, 7), (2, 4, 32, 32)])
@pytest.mark.parametrize("dtype", [bf16, torch.float32], ids=["bf16", "f32"])
def test_one_step_is_bit_identical_to_the_restated_op_chain(shape, dtype):
    from diffusers_amd import ops
    g = torch.Generator().manual_seed(11)
    n = int(np.prod(shape))
    x = (torch.randn(shape, generator=g) * 2.0).to(dtype)
    e2 = torch.randn((2,) + shape, generator=g).to(dtype)
    noise = torch.randn((4,) + shape, generator=g).to(dtype)               # every row differs
    noise[1] = float("nan")                                                # the final rows' noise blocks: never read
    noise[3] = float("nan")
    noise_d, step = noise.to(DEV), torch.zeros((), dtype=torch.int32, device=DEV)
    xd = x.to(DEV)
    checked = 0
    for clip in (0.0, 1.5):
        rows = _rows(clip)
        table = rows.to(DEV)
        for pred, pt in PREDS.items():
            for r, (cfg, gs) in ((r, c) for r in (1, 2) for c in ((False, 0.0), (True, 1.5), (True, 7.5))):
                ee = (e2 if cfg else e2[1]).contiguous()
                final = float(rows[r, 5]) == 0.0
                want = E.ref_step_row(ee, x, None if final else noise[r], rows[r], cfg=cfg, guidance=gs, pred_type=pt)
                step.fill_(r)                                              # a counter of 2 in a 4-row table picks row 2 and noise row 2
                ed = ee.to(DEV)
                what = (shape, str(dtype), pred, r, cfg, gs, clip)
                got = ops.x0_linear_step(ed, xd, noise_d, table, step, cfg=cfg, guidance=gs, pred_type=pt, noise_step_stride=n)
                assert got.dtype == dtype and got.data_ptr() != xd.data_ptr() and torch.equal(xd.cpu(), x), what
                assert torch.isfinite(got.float()).all() and torch.equal(got.cpu(), want), what
                if final:
                    den_row = rows[r - 1].clone()                          # = `denoised` of the same scalars
                    den_row[4], den_row[5] = 1.0, 0.0
                    assert torch.equal(want, E.ref_step_row(ee, x, None, den_row, cfg=cfg, guidance=gs, pred_type=pt)), what
                else:                                                      # ... fed noise row `step` and no other
                    other = E.ref_step_row(ee, x, noise[0], rows[r], cfg=cfg, guidance=gs, pred_type=pt)
                    assert not torch.equal(got.cpu(), other), what
                    one = ops.x0_linear_step(ed, xd, noise_d[r].contiguous(), table, step, cfg=cfg, guidance=gs, pred_type=pt)
                    assert torch.equal(one, got), what                     # the stride-0 single-block form
                if clip:
                    assert not torch.equal(want, E.ref_step_row(ee, x, None if final else noise[r], _rows(0.0)[r], cfg=cfg, guidance=gs,
                                                                pred_type=pt)), what
                alias = xd.clone()                                         # `out` aliasing the sample gives the same bits
                ret = ops.x0_linear_step(ed, alias, noise_d, table, step, cfg=cfg, guidance=gs, out=alias, pred_type=pt,
                                         noise_step_stride=n)
                assert ret.data_ptr() == alias.data_ptr() and torch.equal(alias, got), what
                assert torch.equal(ed.cpu(), ee), what                     # inputs are read only
                checked += 1
    assert checked == 36 and footprint.bits_equal(noise_d.cpu(), noise)


def test_scheduler_step_on_the_device():
    """step() draws like the reference, returns ``denoised`` next to the sample, and the last step returns ``denoised``."""
    from diffusers_amd import ops
    from diffusers_amd.schedulers import LCMScheduler
    s = LCMScheduler(timestep_scaling=1e-3)
    s.set_timesteps(3, device=DEV)
    rows = E.ref_rows(s.alphas_cumprod, s.timesteps.tolist(), 1e-3)
    assert torch.equal(s.device_table[:3].cpu(), rows)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 4, 8, 8, generator=g).to(bf16)
    gen, twin = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    for i, t in enumerate(s.timesteps):
        e = torch.randn(1, 4, 8, 8, generator=g).to(bf16)
        out = s.step(e.to(DEV), t, x.to(DEV), generator=gen)
        den_row = rows[i].clone()
        den_row[4], den_row[5] = 1.0, 0.0
        assert torch.equal(out.denoised.cpu(), E.ref_step_row(e, x, None, den_row))
        noise = torch.randn(x.shape, generator=twin, dtype=bf16) if i < 2 else None
        assert torch.equal(out.prev_sample.cpu(), E.ref_step_row(e, x, noise, rows[i])) and int(s.device_step) == i + 1
        x = out.prev_sample.cpu()
    assert torch.equal(gen.get_state(), twin.get_state())
    xd = x.to(DEV)
    with pytest.raises(ValueError, match="noise"):
        ops.x0_linear_step(xd, xd, None, s.device_table, s.device_step, cfg=False, guidance=0.0, pred_type=4)
    for bad in (3, 7, 8, -1):
        with pytest.raises(ValueError, match="pred_type"):
            ops.x0_linear_step(xd, xd, xd, s.device_table, s.device_step, cfg=False, guidance=0.0, pred_type=bad)


# ----------------------------------------------------------------------------------------------------------------------
# G2
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [bf16, torch.float32], ids=["bf16", "f32"])
def test_scalar_tail_and_unaligned_bases(dtype):
    """Odd element counts (a tail, several workgroups) and operands that start one element into their allocation.  Every operand
    lives in a sentinel-filled (NaN) buffer: the bands around it must be untouched, and a stray read would make the result
    non-finite."""
    from diffusers_amd import ops
    g = torch.Generator().manual_seed(13)
    band = footprint.MIN_BAND_BYTES // (2 if dtype == bf16 else 4)
    table = _rows(0.0).to(DEV)
    for n in (105, 106, 107, 12297):
        x = (torch.randn(n, generator=g) * 3.0).to(dtype)
        e2 = torch.randn(2, n, generator=g).to(dtype)
        nz = torch.randn(n, generator=g).to(dtype)
        for shift, (cfg, gs), pt, r in ((sh, c, p, r) for sh in ("none", "x", "eps", "noise", "out") for c in ((False, 0.0), (True, 7.5))
                                        for p, r in ((4, 0), (5, 1))):
            step = torch.full((), r, dtype=torch.int32, device=DEV)
            ee = (e2 if cfg else e2[1]).contiguous()
            box = {}
            for name, vals in (("x", x), ("eps", ee.reshape(-1)), ("noise", nz), ("out", torch.zeros(n, dtype=dtype))):
                box[name] = footprint.guarded(vals.numel(), dtype=dtype, lead=band + int(shift == name), device=DEV).set(vals)
                assert (box[name].ptr() % 16 != 0) == (shift == name)
            what = (n, str(dtype), shift, cfg, pt, r)
            got = ops.x0_linear_step(box["eps"].view.view(ee.shape), box["x"].view, box["noise"].view, table, step, cfg=cfg,
                                     guidance=gs, out=box["out"].view, pred_type=pt)
            torch.cuda.synchronize()
            want = E.ref_step_row(ee, x, nz, table[r].cpu(), cfg=cfg, guidance=gs, pred_type=pt)
            assert got.data_ptr() == box["out"].ptr() and torch.equal(got.cpu(), want), what
            for name in box:
                box[name].check(f"{name} {what}")
            assert torch.equal(box["eps"].view.cpu(), ee.reshape(-1)) and torch.equal(box["noise"].view.cpu(), nz), what
            assert torch.equal(box["x"].view.cpu(), x), what


# ----------------------------------------------------------------------------------------------------------------------
# G3
# ----------------------------------------------------------------------------------------------------------------------
def test_the_ddim_and_ddpm_prediction_types_are_unchanged():
    """pred_type 0-2 run the kernels they ran: on fp32 tensors (no intermediate rounding, so the stand-in of tests/ops_emulation.py is
    the same operations in the same order) the output equals the stand-in to the bit."""
    from diffusers_amd import ops
    from diffusers_amd.schedulers import DDIMScheduler, DDPMScheduler
    g = torch.Generator().manual_seed(17)
    x = torch.randn(2, 4, 9, 7, generator=g)
    e = torch.randn(2, 4, 9, 7, generator=g)
    noise = torch.randn(2, 4, 9, 7, generator=g)
    step = torch.full((), 2, dtype=torch.int32, device=DEV)
    for pred, pt in (("epsilon", 0), ("v_prediction", 1), ("sample", 2)):
        for cls in (DDIMScheduler, DDPMScheduler):
            s = cls(**E.SD_BETAS, prediction_type=pred, clip_sample=False)
            s.set_timesteps(5, device=DEV)
            table = s.device_table
            got = ops.x0_linear_step(e.to(DEV), x.to(DEV), noise.to(DEV), table, step, cfg=False, guidance=0.0, pred_type=pt).cpu()
            want = ops_emulation.x0_linear_step(e, x, noise, table.cpu(), 2, cfg=False, guidance=0.0, pred_type=pt)
            assert torch.isfinite(got).all() and torch.equal(got, want), (pred, cls.__name__)


# ----------------------------------------------------------------------------------------------------------------------
# pipelines
# ----------------------------------------------------------------------------------------------------------------------
def _embeds(kind, negative=True):
    g = torch.Generator().manual_seed(3)
    pe, npe = (torch.randn(1, 7, 64, generator=g).to(bf16) for _ in range(2))
    te, nte = (torch.randn(1, 64, generator=g).to(bf16) for _ in range(2))
    emb = dict(prompt_embeds=pe.to(DEV), output_type="latent")
    if negative:
        emb["negative_prompt_embeds"] = npe.to(DEV)
    if kind == "sdxl":
        emb["pooled_prompt_embeds"] = te.to(DEV)
        if negative:
            emb["negative_pooled_prompt_embeds"] = nte.to(DEV)
    return emb, (pe, npe, te, nte)


def _pipe(kind, scheduler="lcm", **build_kw):
    from diffusers_amd import factory
    build = factory.build_sdxl_pipeline if kind == "sdxl" else factory.build_sd15_pipeline
    pipe = build(device=DEV, tiny=True, seed=0, scheduler=scheduler, **build_kw)
    if scheduler is None:
        from diffusers_amd.schedulers import EulerDiscreteScheduler
        pipe.scheduler = EulerDiscreteScheduler(**factory.SDXL_SCHEDULER)
    return pipe


def _lat(seed):
    return torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(seed)).to(bf16).to(DEV)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
def test_text_to_image_eager_graph_and_plan_are_bit_identical(kind):
    pipe = _pipe(kind)
    emb, _ = _embeds(kind)

    def run(mode, seed, steps=4, gs=1.5):
        out = pipe(latents=_lat(seed), generator=_gen(100 + seed), num_inference_steps=steps, guidance_scale=gs, height=32, width=32,
                   use_graph=mode, **emb).images.clone()
        torch.cuda.synchronize()
        return out

    eager = {gs: run(False, 8, gs=gs) for gs in (1.0, 1.5)}
    one = run(False, 8, steps=1)
    assert all(torch.isfinite(v.float()).all() for v in eager.values()) and not torch.equal(eager[1.0], eager[1.5])
    assert pipe.scheduler.timesteps.tolist() == [999]
    for mode in (True, "plan"):
        for gs in (1.0, 1.5):                                              # no CFG, and CFG: the LCM-LoRA usage
            assert torch.equal(run(mode, 8, gs=gs), eager[gs]), (mode, gs)
        graph = pipe._graph
        other = run(mode, 9)                                               # other latents, a new seed: the capture is reused
        assert pipe._graph is graph, mode
        assert torch.equal(other, run(False, 9)) and not torch.equal(other, eager[1.5]), mode
        assert torch.equal(run(mode, 8, steps=1), one), mode               # a 1-step call: nothing drawn, the table still there
        assert torch.equal(run(mode, 8), eager[1.5]), mode
    assert not torch.equal(pipe(latents=_lat(8), generator=_gen(1), num_inference_steps=4, guidance_scale=1.5, height=32, width=32,
                                use_graph=False, **emb).images, eager[1.5])  # the noise matters


@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
def test_img2img_and_inpainting_replays_are_bit_identical(kind):
    emb, _ = _embeds(kind)
    img = torch.rand(1, 3, 32, 32, generator=_gen(4))
    mask = torch.zeros(32, 32)
    mask[8:24, 4:20] = 1.0
    for build_kw, call_kw in ((dict(img2img=True), {}), (dict(inpaint=True, unet_in_channels=4), dict(mask_image=mask))):
        pipe = _pipe(kind, **build_kw)
        outs = {}
        for mode in (False, True, "plan"):
            ts = []
            outs[mode] = pipe(image=img, strength=0.5, num_inference_steps=4, guidance_scale=1.5, use_graph=mode, generator=_gen(21),
                              callback_on_step_end=lambda p, i, t, d: ts.append(int(t)) or {}, **call_kw, **emb).images.clone()
            torch.cuda.synchronize()
            assert ts == [499, 259], (build_kw, mode)
        assert torch.isfinite(outs[False].float()).all(), build_kw
        assert torch.equal(outs[True], outs[False]) and torch.equal(outs["plan"], outs[False]), build_kw


@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
def test_controlnet_replays_are_bit_identical(kind):
    pipe = _pipe(kind, controlnet=True)
    emb, _ = _embeds(kind)
    img = torch.rand(1, 3, 32, 32, generator=_gen(4))
    outs = [pipe(image=img, num_inference_steps=4, guidance_scale=1.5, use_graph=mode, generator=_gen(21), latents=_lat(8),
                 **emb).images.clone() for mode in (False, True, "plan")]
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0].float()).all() and torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
def test_cond_unet_runs_without_a_cfg_batch_and_follows_a_new_guidance_scale_through_one_capture(kind):
    pipe = _pipe(kind, time_cond_proj_dim=E.COND_DIM)
    emb, _ = _embeds(kind, negative=False)
    batches = []
    fwd = pipe.unet.forward
    pipe.unet.forward = lambda sample, *a, **k: batches.append(sample.shape[0]) or fwd(sample, *a, **k)

    def run(mode, gs):
        out = pipe(latents=_lat(8), generator=_gen(31), num_inference_steps=4, guidance_scale=gs, height=32, width=32, use_graph=mode,
                   **emb).images.clone()
        torch.cuda.synchronize()
        return out

    eager = {gs: run(False, gs) for gs in (8.0, 4.0)}
    assert set(batches) == {1} and not torch.equal(eager[8.0], eager[4.0])
    for mode in (True, "plan"):
        assert torch.equal(run(mode, 8.0), eager[8.0]), mode
        graph = pipe._graph
        assert torch.equal(run(mode, 4.0), eager[4.0]) and pipe._graph is graph, mode
        assert torch.equal(run(mode, 8.0), eager[8.0]) and pipe._graph is graph, mode


# ----------------------------------------------------------------------------------------------------------------------
# G5
# ----------------------------------------------------------------------------------------------------------------------
def _rel_rms(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


MODEL_REL_RMS = 2.5e-2          # the gate tests/test_models_gpu.py applies to the same tiny U-Nets


@pytest.mark.parametrize("fold", [0, 3], ids=["fold0", "fold3"])
@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
def test_cond_unet_forward_against_the_oracle(kind, fold, monkeypatch):
    from oracle import reference_math as R
    from diffusers_amd import ops
    from diffusers_amd.unet_2d_condition import UNet2DConditionModel
    monkeypatch.setattr(ops, "LN_FOLD", fold)
    cfg, sd, tc = E.cond_unet_case(kind)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 4, 16, 16, generator=g).to(bf16)
    ehs = torch.randn(2, 7, 64, generator=g).to(bf16)
    added = None
    if kind == "sdxl":
        added = {"text_embeds": torch.randn(2, 64, generator=g).to(bf16), "time_ids": torch.tensor([[32., 32, 0, 0, 32, 32]]).repeat(2, 1)}
    full = dict(UNet2DConditionModel(**cfg).config)
    ref = R.unet_forward(E.oracle_state_dict(sd, tc), full, x.float(), 499.0, ehs.float(),
                         None if added is None else {k: v.float() for k, v in added.items()})
    unet = UNet2DConditionModel(**cfg).load_state_dict(sd, device=DEV)
    dadded = None if added is None else {k: v.to(DEV) for k, v in added.items()}
    y = unet(x.to(DEV), torch.tensor(499.0), ehs.to(DEV), timestep_cond=tc.to(DEV), added_cond_kwargs=dadded, return_dict=False)[0]
    rr = _rel_rms(y, ref)
    print(f"[parity] tiny {kind} U-Net with time_cond_proj_dim (LN_FOLD={fold}): rel_rms vs oracle fp32 = {rr:.3e}")
    assert torch.isfinite(y.float()).all() and rr < MODEL_REL_RMS
    cond = unet.precompute_conditioning(ehs.to(DEV), dadded, timestep_cond=tc.to(DEV))
    assert torch.equal(unet(x.to(DEV), torch.tensor(499.0), None, conditioning=cond, return_dict=False)[0], y)
    with pytest.raises(ValueError, match="timestep_cond"):
        unet(x.to(DEV), torch.tensor(499.0), ehs.to(DEV), added_cond_kwargs=dadded)


# ----------------------------------------------------------------------------------------------------------------------
# G6
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
def test_pipeline_loop_against_a_test_side_fp32_loop_with_euler_as_the_yardstick(kind):
    """The engine pipeline (bf16 latents, the fused step, the captured graph, a seeded generator) against a loop written here: fp32
    latents (bf16 only at the U-Net's input), the schedule restated in float64, the same noise rows read back from the pipeline's
    table.  bf16-latent steps through a random-weight U-Net have no derivable bound; both paths round the latents once per step, and
    2x the same quantity measured for EulerDiscreteScheduler (through oracle.samplers.EulerOracle, in this test, at the same step
    count) is the allowance the project gives a different trajectory."""
    from oracle.samplers import EulerOracle
    from diffusers_amd import factory
    steps, gs = 4, 1.5
    lat = _lat(8)
    vals = {}
    for which in ("lcm", "euler"):
        pipe = _pipe(kind, scheduler="lcm" if which == "lcm" else None)
        emb, (pe, npe, te, nte) = _embeds(kind)
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

        if which == "lcm":
            sch = pipe.scheduler
            ts = sch.timesteps.tolist()
            assert ts == [999, 759, 499, 259]
            betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
            abar = np.cumprod(1.0 - betas)
            noise = pipe._noise_table.double().cpu().numpy()
            assert noise.shape[0] == steps
            x = lat.float().cpu().double().numpy()
            for i, t in enumerate(ts):
                e = eps_of(torch.from_numpy(x).float(), t).double().numpy()
                x0 = (x - np.sqrt(1 - abar[t]) * e) / np.sqrt(abar[t])
                scaled = t * 10.0
                den = scaled / np.sqrt(scaled ** 2 + 0.25) * x0 + 0.25 / (scaled ** 2 + 0.25) * x
                x = den if i == steps - 1 else np.sqrt(abar[ts[i + 1]]) * den + np.sqrt(1 - abar[ts[i + 1]]) * noise[i]
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
    line = (f"[parity] tiny {kind} {steps} steps, engine pipeline (bf16 latents) vs fp32 loop: rel_rms LCM "
            f"{vals['lcm']:.3e}, Euler {vals['euler']:.3e}, ratio {vals['lcm'] / vals['euler']:.2f}")
    print(line)             # (the lines of one run on an MI355X are kept in profiles/lcm_gpu_suite_parity_lines.txt)
    assert vals["lcm"] <= 2.0 * vals["euler"], line
