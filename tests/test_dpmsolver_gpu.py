"""GPU: da_dpmpp_2m_step and DPMSolverMultistepScheduler in the pipelines.

G1 one step against float64, G2 sequences and a loop started on stale history, G3 eager == captured graph == launch plan in the
tiny SDXL / SD 1.5 pipelines (text-to-image, img2img, denoising_end), G4 the pipeline's loop against a test-side fp32 loop with the
Euler path as the yardstick, G5 guidance_rescale and no-CFG.  The float64 restatement is the one of tests/test_dpmsolver_cpu.py.

Bound of one step (G1, G2).  The kernel does about ten fp32 operations per element, each correctly rounded (2^-24 relative to its
result, which is at most the sum of the absolute values of its operands).  With T = the sum of the absolute values of the terms of
the update, every product expanded down to the inputs (``row_step``), the fp32 result is within 2^-20 T of the float64 value (16x
headroom); a bf16 sample is that value rounded once more, 2^-8 |ref| (one bf16 ulp: the correct rounding, or its neighbour when the
fp32 error crosses a rounding boundary).

Bound of the history.  The history is the fp32 x0.  Its rounding errors are relative to the terms of x0 itself, t0 = (|x| +
sigma_s0 |e|) / alpha_s0 for epsilon, alpha_s0 |x| + sigma_s0 |e| for v_prediction, |e| for sample (``row_step``), so the bound here is
2^-20 t0 and NOT 2^-20 T of the update: T holds x0 only through c0 t0, and c0 is close to 0 on the first rows of a ladder (0.03 on row
0 of 20 Karras steps), where an exactly rounded x0 is already off by more than 2^-20 T in elements with small |x|; on late rows t0
exceeds T instead.  x0 takes at most three roundings (product, difference, quotient), each 2^-24 of a value no larger than t0, so
2^-20 t0 keeps about 5x headroom; no element is exempt.

The reference is fed the fp32 table row the kernel reads and the same inputs; with CFG the combine u + g (c - u) is evaluated with
torch ops in the model output's dtype, which is what the kernel's combine reproduces operation by operation."""
import numpy as np
import pytest
import torch

from test_dpmsolver_cpu import EPS32, SD_BETAS, ref_alpha_sigma, ref_first_order, ref_step, row_step

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
bf16 = torch.bfloat16


def _sched(n, **kw):
    from diffusers_amd.schedulers import DPMSolverMultistepScheduler
    cfg = dict(SD_BETAS)
    cfg.update(kw)
    s = DPMSolverMultistepScheduler(**cfg)
    s.set_timesteps(n, device=DEV)
    return s


def _combine(e, cfg, g, shape):
    """The CFG combine with torch CPU ops in the model output's dtype (every op rounded in that dtype, as the kernel does)."""
    if not cfg:
        return e.reshape(shape).double().numpy()
    u, c = e[0], e[1]
    return (u + g * (c - u)).reshape(shape).double().numpy()


def _check_step(got_x, got_m1, x, e, m1, row, second, pred, x_dtype, what):
    want, want_x0, T, t0 = row_step(x.double().numpy(), e, m1.double().numpy(), row, second, pred)
    err = np.abs(got_x.double().cpu().numpy() - want)
    bound = EPS32 * T + (2.0 ** -8 * np.abs(want) if x_dtype == bf16 else 0.0)
    herr = np.abs(got_m1.double().cpu().numpy() - want_x0)
    assert np.isfinite(got_x.float().cpu().numpy()).all(), what
    assert (err <= bound).all(), (what, float((err / np.maximum(bound, 1e-300)).max()))
    assert (herr <= EPS32 * t0).all(), (what, "history", float((herr / np.maximum(EPS32 * t0, 1e-300)).max()))
    return float((err / np.maximum(bound, 1e-300)).max())


# ----------------------------------------------------------------------------------------------------------------------
# G1
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 4, 128, 128), (2, 4, 9, 7)])
@pytest.mark.parametrize("x_dtype", [bf16, torch.float32], ids=["bf16", "f32"])
def test_one_step_against_float64(shape, x_dtype):
    from diffusers_amd import _lib as L, ops
    g = torch.Generator().manual_seed(11)
    x = torch.randn(shape, generator=g)
    m1 = torch.randn(shape, generator=g)
    e2 = torch.randn((2,) + shape, generator=g)
    worst = 0.0
    tables = {(st, final): _sched(20, use_karras_sigmas=(final == "zero"), solver_type=st, final_sigmas_type=final,
                                  lower_order_final=False).device_table
              for st in ("midpoint", "heun") for final in ("zero", "sigma_min")}
    step, begin = (torch.zeros((), dtype=torch.int32, device=DEV) for _ in range(2))
    for (st, final), table in tables.items():
        rows = table.cpu().numpy()
        assert rows[19, 6] == (0.0 if final == "zero" else 1.0)         # the last row runs second order only past a non-zero sigma
        for r, order, pred, (cfg, gs), e_dtype in (
                (r, o, p, c, d) for r in (0, 1, 10, 19) for o in (1, 2) for p in ("epsilon", "v_prediction", "sample")
                for c in ((False, 0.0), (True, 5.0), (True, 7.5)) for d in (bf16, torch.float32)):
            if st == "heun" and order == 1:
                continue                                                # first-order rows do not depend on the solver type
            xs = (x * float(rows[r, 1] / rows[r, 0] + 1.0)).to(x_dtype)  # samples at the row's noise level
            ee = (e2 if cfg else e2[1]).to(e_dtype)
            xd, md, ed = xs.to(DEV), m1.clone().to(DEV), ee.contiguous().to(DEV)
            step.fill_(r)
            begin.fill_(r if order == 1 else (r + 1) % 20)               # first step of its loop <=> first order
            second = order == 2 and rows[r, 6] != 0
            ops.dpmpp_2m_step_(ed, xd, md, table, step, begin, cfg=cfg, guidance=gs, pred_type=L.PRED_TYPES[pred])
            torch.cuda.synchronize()
            what = (shape, str(x_dtype), st, final, r, order, pred, cfg, gs, str(e_dtype))
            worst = max(worst, _check_step(xd, md, xs, _combine(ee, cfg, gs, shape), m1, rows[r], second, L.PRED_TYPES[pred],
                                           x_dtype, what))
            if final == "zero" and r == 19:                              # sigma_last = 0: the row is x' = x0
                assert torch.equal(xd.float(), md.to(x_dtype).float()), what
    print(f"[parity] dpmpp one step {shape} {x_dtype}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("x_dtype", [bf16, torch.float32], ids=["bf16", "f32"])
def test_scalar_tail_and_unaligned_bases(x_dtype):
    """G1's bound on the kernel's other two paths.  Element counts with n % 4 in {1, 2, 3} run a 4-wide body plus a scalar tail
    without CFG and the all-scalar path with CFG (the cond half starts n elements in, off the 4-wide grid); a sample, model output or
    history that starts one element into a larger buffer is not 16-byte aligned and runs all-scalar too.  Every operand lives inside
    an over-allocated buffer of a known value: what lies before and past its n elements must be untouched."""
    from diffusers_amd import _lib as L, ops
    PAD, CANARY = 8, 1024.0
    g = torch.Generator().manual_seed(13)
    table = _sched(20, use_karras_sigmas=True).device_table
    rows = table.cpu().numpy()
    r = 10
    step = torch.full((), r, dtype=torch.int32, device=DEV)
    begin = torch.zeros((), dtype=torch.int32, device=DEV)
    worst = 0.0

    def boxed(values, dtype, off):
        """``values`` copied ``PAD + off`` elements into a canary-filled device buffer -> (buffer, the view the kernel gets)."""
        buf = torch.full((values.numel() + 2 * PAD + 1,), CANARY, dtype=dtype, device=DEV)
        view = buf[PAD + off:PAD + off + values.numel()]
        view.copy_(values.reshape(-1).to(dtype))
        return buf, view

    def untouched(buf, view_len, off):
        lo, hi = buf[:PAD + off], buf[PAD + off + view_len:]
        return bool((lo == CANARY).all()) and bool((hi == CANARY).all()) and hi.numel() >= PAD

    for n in (105, 106, 107, 12297):                                    # n % 4 = 1, 2, 3, 1 (the last: several workgroups + a tail)
        x = torch.randn(n, generator=g) * float(rows[r, 1] / rows[r, 0] + 1.0)
        m1 = torch.randn(n, generator=g)
        e2 = torch.randn(2, n, generator=g)
        for shift, (cfg, gs), order, pred, e_dtype in (
                (sh, c, o, p, d) for sh in ("none", "x", "eps", "m1") for c in ((False, 0.0), (True, 7.5)) for o in (1, 2)
                for p in ("epsilon", "v_prediction", "sample") for d in (bf16, torch.float32)):
            ee = (e2 if cfg else e2[1]).to(e_dtype)
            offs = {k: int(shift == k) for k in ("x", "eps", "m1")}
            xb, xv = boxed(x, x_dtype, offs["x"])
            eb, ev = boxed(ee, e_dtype, offs["eps"])
            mb, mv = boxed(m1, torch.float32, offs["m1"])
            if shift != "none":
                assert {"x": xv, "eps": ev, "m1": mv}[shift].data_ptr() % 16 != 0
            xs = xv.clone().cpu()                                        # the sample as stored (rounded to bf16 where it is bf16)
            begin.fill_(r if order == 1 else 0)
            ops.dpmpp_2m_step_(ev, xv, mv, table, step, begin, cfg=cfg, guidance=gs, pred_type=L.PRED_TYPES[pred])
            torch.cuda.synchronize()
            what = (n, str(x_dtype), shift, cfg, order, pred, str(e_dtype))
            worst = max(worst, _check_step(xv, mv, xs, _combine(ee, cfg, gs, (n,)), m1, rows[r], order == 2, L.PRED_TYPES[pred],
                                           x_dtype, what))
            assert untouched(xb, n, offs["x"]) and untouched(mb, n, offs["m1"]) and untouched(eb, ee.numel(), offs["eps"]), what
            assert torch.equal(ev.cpu(), ee.reshape(-1)), what           # the model output is read only
    print(f"[parity] dpmpp scalar tail / unaligned bases {x_dtype}: worst error / bound = {worst:.3f}")


def test_argument_checks():
    from diffusers_amd import ops
    s = _sched(8)
    x = torch.randn(1, 4, 8, 8, device=DEV).to(bf16)
    m1 = torch.zeros(1, 4, 8, 8, device=DEV)
    st, bg = s.device_step, s.device_begin
    with pytest.raises(ValueError):                 # the history is fp32
        ops.dpmpp_2m_step_(x, x.clone(), m1.to(bf16), s.device_table, st, bg)
    with pytest.raises(ValueError):                 # [2 x sample] with cfg
        ops.dpmpp_2m_step_(x, x.clone(), m1, s.device_table, st, bg, cfg=True, guidance=5.0)
    with pytest.raises(ValueError):
        ops.dpmpp_2m_step_(x, x.clone(), m1[:, :2], s.device_table, st, bg)
    with pytest.raises((ValueError, RuntimeError)):     # host tensors have no path
        ops.dpmpp_2m_step_(x.cpu(), x.cpu(), m1.cpu(), s.device_table, st, bg)
    import diffusers_amd.torch_ops  # noqa: F401
    xn, mn = torch.ops.mi355x.dpmpp_2m_step(x, x, m1, s.device_table, st, bg, False, 0.0, 0)
    x2, m2 = x.clone(), m1.clone()
    ops.dpmpp_2m_step_(x, x2, m2, s.device_table, st, bg)
    assert torch.equal(xn, x2) and torch.equal(mn, m2) and xn.data_ptr() != x.data_ptr()
    xt = x.transpose(-1, -2)                        # the functional op takes a non-contiguous sample (the in-place one cannot)
    xn_t, _ = torch.ops.mi355x.dpmpp_2m_step(x, xt, m1, s.device_table, st, bg, False, 0.0, 0)
    x3, m3 = xt.contiguous(), m1.clone()
    ops.dpmpp_2m_step_(x, x3, m3, s.device_table, st, bg)
    assert torch.equal(xn_t, x3)
    with pytest.raises(ValueError):
        ops.dpmpp_2m_step_(x, xt, m1.clone(), s.device_table, st, bg)


# ----------------------------------------------------------------------------------------------------------------------
# G2
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x_dtype", [bf16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("solver_type", ["midpoint", "heun"])
def test_sequences_and_a_loop_started_on_stale_history(x_dtype, solver_type):
    """12 steps with a fresh model output per step from row 0, then -- after reset(5), the history holding the last x0 of that run --
    from row 5.  Every step is within the one-step bound of the restated step applied to the sample and history the kernel had (the
    steps are not contractions for an arbitrary model output, so errors are not summed along the trajectory); which steps are first
    order follows the restated rule for a loop that begins there; row 5 equals a first-order step on zeroed history bit for bit."""
    n, shape = 12, (2, 4, 33, 31)
    g = torch.Generator().manual_seed(5)
    es = [torch.randn(shape, generator=g).to(x_dtype) for _ in range(n)]
    start = torch.randn(shape, generator=g)
    s = _sched(n, use_karras_sigmas=True, solver_type=solver_type)
    rows, sig = s.device_table.cpu().numpy(), s.sigmas.double().numpy()
    row5 = None
    for begin in (0, 5):
        s.reset(begin)
        a, b = ref_alpha_sigma(sig[begin])
        x = (start * float(b / a + 1.0)).to(x_dtype).to(DEV)
        for i in range(begin, n):
            x_in, m_in = x.clone().cpu(), s.history(x).clone().cpu()
            s.step_inplace(es[i].to(DEV), x)
            torch.cuda.synchronize()
            second = not ref_first_order(i, n, i == begin)
            assert second == (bool(rows[i, 6]) and i != begin)
            _check_step(x, s.history(x), x_in, es[i].double().numpy(), m_in, rows[i], second, 0, x_dtype, (begin, i))
            if x_dtype == torch.float32:        # and the row is the restated step: fp32 storage of its coefficients, a few 2^-24 T
                want, _ = ref_step(x_in.double().numpy(), es[i].double().numpy(), m_in.double().numpy(), sig, i, not second, solver_type)
                T = row_step(x_in.double().numpy(), es[i].double().numpy(), m_in.double().numpy(), rows[i], second, 0)[2]
                assert (np.abs(x.double().cpu().numpy() - want) <= 2 * EPS32 * T).all(), (begin, i)
            if begin == 5 and i == 5:
                row5 = x.clone()
        assert s.step_index == n
    fresh = _sched(n, use_karras_sigmas=True, solver_type=solver_type)
    fresh.reset(5)
    a, b = ref_alpha_sigma(sig[5])
    x = (start * float(b / a + 1.0)).to(x_dtype).to(DEV)
    assert float(fresh.history(x).abs().max()) == 0.0
    fresh.step_inplace(es[5].to(DEV), x)
    assert torch.equal(x, row5)


# ----------------------------------------------------------------------------------------------------------------------
# pipelines
# ----------------------------------------------------------------------------------------------------------------------
def _embeds(seed, B, seq, dim, pooled):
    g = torch.Generator().manual_seed(seed)
    pe, npe = (torch.randn(B, seq, dim, generator=g).to(bf16) for _ in range(2))
    te, nte = (torch.randn(B, pooled, generator=g).to(bf16) for _ in range(2)) if pooled else (None, None)
    return pe, npe, te, nte


def _pipe(kind, img2img=False, scheduler="dpm"):
    from diffusers_amd import factory
    from diffusers_amd.schedulers import DPMSolverMultistepScheduler, EulerDiscreteScheduler
    build = factory.build_sdxl_pipeline if kind == "sdxl" else factory.build_sd15_pipeline
    pipe = build(device=DEV, tiny=True, seed=0, img2img=img2img)
    if scheduler == "dpm":
        pipe.scheduler = DPMSolverMultistepScheduler(**(factory.SDXL_DPM_SCHEDULER if kind == "sdxl" else factory.SD15_DPM_SCHEDULER))
    else:
        pipe.scheduler = EulerDiscreteScheduler(**factory.SDXL_SCHEDULER)
    pe, npe, te, nte = _embeds(3, 1, 7, 64 if kind == "sdxl" else _cross_dim(pipe), 64 if kind == "sdxl" else 0)
    emb = dict(prompt_embeds=pe.to(DEV), negative_prompt_embeds=npe.to(DEV), output_type="latent")
    if kind == "sdxl":
        emb.update(pooled_prompt_embeds=te.to(DEV), negative_pooled_prompt_embeds=nte.to(DEV))
    return pipe, emb, (pe, npe, te, nte)


def _cross_dim(pipe):
    d = pipe.unet.config.cross_attention_dim
    return d if isinstance(d, int) else d[0]


def _lat(seed):
    return torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(seed)).to(bf16).to(DEV)


# ----------------------------------------------------------------------------------------------------------------------
# G3
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
def test_eager_graph_and_plan_replay_are_bit_identical(kind):
    pipe, emb, _ = _pipe(kind)

    def run(mode, seed, steps=8, **kw):
        out = pipe(latents=_lat(seed), num_inference_steps=steps, guidance_scale=5.0, height=32, width=32, use_graph=mode,
                   **emb, **kw).images.clone()
        torch.cuda.synchronize()
        return out

    eager = run(False, 8)
    assert torch.isfinite(eager.float()).all()
    for mode in (True, "plan"):
        assert torch.equal(run(mode, 8), eager), mode
        graph = pipe._graph
        other = run(mode, 9)                                    # other latents, same step count: no re-capture
        assert pipe._graph is graph, mode
        assert torch.equal(other, run(False, 9)) and not torch.equal(other, eager), mode
        assert torch.equal(run(mode, 8, steps=11), run(False, 8, steps=11)), mode       # another step count
        assert torch.equal(run(mode, 8), eager), mode
    if kind == "sdxl":
        want = run(False, 8, steps=10, denoising_end=0.8)
        for mode in (True, "plan"):
            n = []
            part = run(mode, 8, steps=10, denoising_end=0.8, callback_on_step_end=lambda p, i, t, d: n.append(i) or {})
            assert 0 < len(n) < 10 and torch.equal(part, want), mode
        for kw in (dict(timesteps=[900, 500, 100]), dict(sigmas=[10.0, 1.0, 0.0])):
            with pytest.raises(ValueError, match="does not support custom timestep or sigma schedules"):
                run(False, 8, **kw)


@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
def test_img2img_replay_is_bit_identical(kind):
    """strength 0.5 of 8 steps: the loop starts at row 4 and replays the same captured step; its first step is first order."""
    pipe, emb, _ = _pipe(kind, img2img=True)
    img = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(4))

    def run(mode, strength=0.5, image=img):
        n = []
        out = pipe(image=image, strength=strength, num_inference_steps=8, guidance_scale=5.0, use_graph=mode,
                   generator=torch.Generator().manual_seed(21), callback_on_step_end=lambda p, i, t, d: n.append(int(t)) or {},
                   **emb).images.clone()
        torch.cuda.synchronize()
        return out, n

    eager, ts = run(False)
    assert len(ts) == 4 and ts == pipe.scheduler.timesteps[4:].tolist() and torch.isfinite(eager.float()).all()
    assert int(pipe.scheduler.device_begin) == 4
    for mode in (True, "plan"):
        assert torch.equal(run(mode)[0], eager), mode
        graph = pipe._graph
        out75, ts75 = run(mode, strength=0.75)                  # another start row replays the same graph
        assert pipe._graph is graph and len(ts75) == 6
        assert torch.equal(out75, run(False, strength=0.75)[0]), mode
        assert torch.equal(run(mode)[0], eager), mode           # and back, on the history the longer loop left


def test_base_to_refiner_handoff_runs_the_second_half_from_its_own_first_step():
    """denoising_end = 0.8 then denoising_start = 0.8 on the same scheduler: eager == graph == plan on both sides.  (Unlike a one-step
    method, the hand-off is not bit-identical to the uninterrupted run: the refiner's first step is first order, as in the reference.)"""
    from diffusers_amd.pipelines import StableDiffusionXLImg2ImgPipeline
    base, emb, _ = _pipe("sdxl")
    ref = StableDiffusionXLImg2ImgPipeline(vae=base.vae, unet=base.unet, scheduler=base.scheduler)
    outs = []
    for mode in (False, True, "plan"):
        mid = base(latents=_lat(8), num_inference_steps=12, guidance_scale=5.0, height=32, width=32, denoising_end=0.8,
                   use_graph=mode, **emb).images.clone()
        outs.append(ref(image=mid, num_inference_steps=12, denoising_start=0.8, guidance_scale=5.0, use_graph=mode, **emb).images.clone())
        assert int(base.scheduler.device_begin) > 0
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and torch.isfinite(outs[0].float()).all()


# ----------------------------------------------------------------------------------------------------------------------
# G4
# ----------------------------------------------------------------------------------------------------------------------
def _rel_rms(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
def test_pipeline_loop_against_a_test_side_fp32_loop_with_euler_as_the_yardstick(kind):
    """The engine U-Net called eagerly from a loop written here (fp32 latents, bf16 only at the U-Net's input, the restated scheduler
    in float64) against the engine pipeline (bf16 latents, the fused step), 8 steps, Karras.  Eight steps of bf16 latents through a
    U-Net have no derivable bound, so the yardstick is the path that ships: the same quantity for EulerDiscreteScheduler through
    oracle.samplers in the same test.  Gate: at most 2x Euler's (both round the latents to bf16 once per step; 2x covers the
    second-order term amplifying a rounding of the previous step by 1 / (2 r0))."""
    from oracle.samplers import EulerOracle
    from diffusers_amd import factory
    steps, gs = 8, 5.0
    lat = _lat(8)
    vals = {}
    for which in ("dpm", "euler"):
        pipe, emb, (pe, npe, te, nte) = _pipe(kind, scheduler=which)
        got = pipe(latents=lat.clone(), num_inference_steps=steps, guidance_scale=gs, height=32, width=32, use_graph=True,
                   **emb).images.clone()
        ehs = torch.cat([npe, pe]).to(DEV)
        added = None
        if kind == "sdxl":
            ids = torch.tensor([[32, 32, 0, 0, 32, 32]], dtype=torch.float32, device=DEV).repeat(2, 1)
            added = {"text_embeds": torch.cat([nte, te]).to(DEV), "time_ids": ids}

        def eps_of(x_in, t):
            xin = torch.cat([x_in, x_in]).to(bf16).to(DEV).contiguous()
            out = pipe.unet(xin, float(t), encoder_hidden_states=ehs, added_cond_kwargs=added, return_dict=False)[0].float().cpu()
            return out[:1] + gs * (out[1:] - out[:1])

        if which == "dpm":
            sch = pipe.scheduler
            sig, ts = sch.sigmas.double().numpy(), sch.timesteps.tolist()
            x, m1 = lat.float().cpu().double().numpy(), None
            for i in range(steps):
                e = eps_of(torch.from_numpy(x).float(), ts[i]).double().numpy()
                x, m1 = ref_step(x, e, m1, sig, i, ref_first_order(i, steps, i == 0), "midpoint")
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
    line = (f"[parity] tiny {kind} {steps} steps, engine pipeline (bf16 latents) vs fp32 loop: rel_rms DPM++ 2M Karras "
            f"{vals['dpm']:.3e}, Euler {vals['euler']:.3e}, ratio {vals['dpm'] / vals['euler']:.2f}")
    print(line)             # (the lines of one run on an MI355X are kept in profiles/dpmpp_gpu_suite_parity_lines.txt)
    assert vals["dpm"] <= 2.0 * vals["euler"], line


# ----------------------------------------------------------------------------------------------------------------------
# G5
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
@pytest.mark.parametrize("kw", [dict(guidance_scale=5.0, guidance_rescale=0.7), dict(guidance_scale=1.0)], ids=["rescale", "no_cfg"])
def test_guidance_rescale_and_no_cfg(kind, kw):
    pipe, emb, _ = _pipe(kind)
    outs = [pipe(latents=_lat(8), num_inference_steps=8, height=32, width=32, use_graph=mode, **kw, **emb).images.clone()
            for mode in (False, True)]
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0].float()).all() and torch.equal(outs[0], outs[1])
