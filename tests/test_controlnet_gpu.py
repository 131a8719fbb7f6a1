"""GPU: the rounded fp32 gate of the first-family GEMM epilogue (da_gemm_params.gate_f32 == 2), the memory footprint of the
ControlNet launches, ControlNetModel on the device and the two ControlNet pipelines (tiny configs: 16 x 16 latents, 32 x 32 control
image, block_out_channels (64, 128)).  The restatement and the oracle loops are those of tests/controlnet_emulation.py."""
import functools

import pytest
import torch
import torch.nn.functional as F

import call_sequences as CS
import controlnet_emulation as CE
from footprint import bits_equal, guarded, poisoned
from oracle import ref_runtime as RR

pytestmark = pytest.mark.gpu

bf16, f32 = torch.bfloat16, torch.float32
DEV = "cuda"


def _ops():
    from diffusers_amd import _lib as L
    from diffusers_amd import ops
    return ops, L


def rnd(shape, seed, scale=1.0, dtype=bf16):
    return (torch.randn(shape, generator=torch.Generator("cpu").manual_seed(seed)) * scale).to(dtype).to(DEV)


# ---- 4. gate mode 2, to the bit ------------------------------------------------------------------------------------------
GATES = {"0.7": (0.7, 0.7), "1.0": (1.0, 1.0), "0.0": (0.0, 0.0), "pair": (0.7, -0.3), "exact pair": (0.5, -1.25)}


@pytest.mark.parametrize("conv", [0, 1])
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("hw", [(8, 8), (6, 10)])
def test_rounded_f32_gate_to_the_bit(conv, C, hw):
    """M = 2 * 8 * 8 (whole 64-row tiles) and 2 * 6 * 10 (a partial one), N = K = C, as nn.Linear and as a 1x1 conv, on a 64- and
    a 128-row first-family tile: ``y`` from a launch without gate and residual; then gate mode 2 with ``residual == C`` gives
    ``bf16(r + bf16(y.float() * g))`` from y's own bits; a gate that is exact in bf16 also equals the bf16-gate launch."""
    ops, L = _ops()
    H, W_ = hw
    B, M = 2, 2 * H * W_
    x, w, bias, r = rnd((B, H, W_, C), 1), rnd((C, C), 2, C ** -0.5), rnd((C,), 3), rnd((B, H, W_, C), 4)

    def launch(tile, out=None, **kw):
        if conv:
            return ops.conv2d_nhwc(x, w, bias, ksize=1, tile=tile, staging=L.STAGE_LDS_DIRECT, out=out, **kw)
        if "residual" in kw:
            kw["residual"] = kw["residual"].view(M, C)
        if "gate" in kw:
            kw["rows_per_batch"] = H * W_
        return ops.linear(x.view(M, C), w, bias, tile=tile, staging=L.STAGE_LDS_DIRECT, out=None if out is None else out.view(M, C),
                          **kw).view(B, H, W_, C)

    for tile in (L.TILE_64x64, L.TILE_128x128):
        y = launch(tile)
        for name, (g0, g1) in GATES.items():
            gate = torch.tensor([[g0] * C, [g1] * C], dtype=f32, device=DEV)
            c = r.clone()
            launch(tile, out=c, gate=gate, gate_round=True, residual=c)
            gg = gate[:, None, None, :]
            want = (r.float() + (y.float() * gg).to(bf16).float()).to(bf16)
            assert bits_equal(c, want), f"conv={conv} C={C} {hw} tile {L.TILE_NAMES[tile]} gate {name}"
            if gate.to(bf16).float().equal(gate):
                c2 = r.clone()
                launch(tile, out=c2, gate=gate.to(bf16), residual=c2)
                assert bits_equal(c2, c), f"bf16-gate launch differs for the exact gate {name}"
            if name == "0.7":      # and it is NOT the Wan mode (product kept in fp32) on some element of this size
                c1 = r.clone()
                launch(tile, out=c1, gate=gate, residual=c1)
                assert not bits_equal(c1, c)
    # the library's own tile choice is a first-family tile: same bits as the pinned one (every tile of a family sums K alike)
    gate = torch.full((B, C), 0.7, dtype=f32, device=DEV)
    c, ca = r.clone(), r.clone()
    launch(L.TILE_64x64, out=c, gate=gate, gate_round=True, residual=c)
    launch(None, out=ca, gate=gate, gate_round=True, residual=ca)
    assert bits_equal(c, ca)


def test_rounded_f32_gate_refusals_and_plan_replay():
    ops, L = _ops()
    from diffusers_amd import plan as P
    B, H, W_, C = 2, 6, 10, 128
    x, w, bias, r = rnd((B, H, W_, C), 1), rnd((C, C), 2, C ** -0.5), rnd((C,), 3), rnd((B, H, W_, C), 4)
    gate = torch.tensor([[0.7] * C, [-0.3] * C], dtype=f32, device=DEV)
    for tile in (L.TILE_K2_128x128, L.TILE_K1_256x128, L.TILE_K3_256x256):
        c = r.clone()
        with pytest.raises(RuntimeError, match="DA_ERR_UNSUPPORTED"):
            if tile == L.TILE_K3_256x256:    # nn.Linear only
                ops.linear(x.view(-1, C), w, bias, gate=gate, gate_round=True, rows_per_batch=H * W_, residual=c.view(-1, C),
                           out=c.view(-1, C), tile=tile, staging=L.STAGE_LDS_DIRECT)
            else:
                ops.conv2d_nhwc(x, w, bias, ksize=1, gate=gate, gate_round=True, residual=c, out=c, tile=tile, staging=L.STAGE_LDS_DIRECT)
        torch.cuda.synchronize()
        assert bits_equal(c, r)
    p = L.GemmParams()
    out = torch.empty((B * H * W_, C), device=DEV, dtype=bf16)
    p.A, p.W, p.C, p.gate = x.data_ptr(), w.data_ptr(), out.data_ptr(), gate.data_ptr()
    p.M, p.N, p.K, p.lda, p.ldw, p.ldc, p.ld_gate, p.rows_per_batch = B * H * W_, C, C, C, C, C, C, H * W_
    p.tile, p.staging = L.TILE_64x64, L.STAGE_LDS_DIRECT
    import ctypes
    st = torch.cuda.current_stream().cuda_stream
    for bad in (3, -1):
        p.gate_f32 = bad
        assert L.load().da_gemm_bf16(ctypes.byref(p), st) == 1          # DA_ERR_INVALID
    with pytest.raises(TypeError, match="gate_round"):
        ops.conv2d_nhwc(x, w, bias, ksize=1, gate=gate.to(bf16), gate_round=True)
    w3 = rnd((C, 9 * C), 5, (9 * C) ** -0.5)
    with pytest.raises(ValueError, match="1x1"):
        ops.conv2d_nhwc(x, w3, bias, ksize=3, gate=gate, gate_round=True)
    # a recorded plan replays the same launch, bit for bit
    c = r.clone()
    ops.conv2d_nhwc(x, w, bias, ksize=1, gate=gate, gate_round=True, residual=c, out=c)
    c2 = r.clone()
    pl, _ = P.record(lambda: ops.conv2d_nhwc(x, w, bias, ksize=1, gate=gate, gate_round=True, residual=c2, out=c2))
    assert len(pl) == 1 and pl.foreign_ops == [] and bits_equal(c2, c)
    c2.copy_(r)
    pl.launch()
    torch.cuda.synchronize()
    assert bits_equal(c2, c)


# ---- 5. memory footprint -------------------------------------------------------------------------------------------------
def test_handoff_launch_footprint():
    """The hand-off launch (conv == 1, gate mode 2, residual == C) inside guard bands, its operands inside poison: nothing outside
    the logical tensors is written, nothing outside them changes a bit of the result."""
    ops, L = _ops()
    B, H, W_, C = 2, 6, 10, 128
    x, w, bias, r = rnd((B, H, W_, C), 1), rnd((C, C), 2, C ** -0.5), rnd((C,), 3), rnd((B, H, W_, C), 4)
    gate = torch.tensor([[0.7] * C, [-0.3] * C], dtype=f32, device=DEV)
    results = []
    for kind in ("poisoned", "clean"):
        ins = {"x": poisoned(x), "w": poisoned(w), "bias": poisoned(bias), "gate": poisoned(gate, ld=C + 4)}
        if kind == "clean":
            ins = {k: g.clean() for k, g in ins.items()}
        tgt = poisoned(r)
        if kind == "clean":
            tgt = tgt.clean()
        before = {k: g.snapshot() for k, g in ins.items()}
        ops.conv2d_nhwc(ins["x"].view, ins["w"].view, ins["bias"].view, ksize=1, gate=ins["gate"].view, gate_round=True,
                        residual=tgt.view, out=tgt.view)
        torch.cuda.synchronize()
        tgt.check(f"hand-off target ({kind})")
        for k, g in ins.items():
            assert torch.equal(g.bits, before[k]), f"read-only operand {k} was written ({kind} run)"
        results.append(tgt.view.clone())
    assert bits_equal(results[0], results[1])
    y = (F.conv2d(x.float().permute(0, 3, 1, 2), w.float()[:, :, None, None], bias.float()).permute(0, 2, 3, 1)).to(bf16)
    want = (r.float() + (y.float() * gate[:, None, None, :]).to(bf16).float()).to(bf16)
    assert (results[0].float() - want.float()).abs().max() <= 2 * 2.0 ** -8 * want.float().abs().max()


@pytest.mark.parametrize("stride", [1, 2])
def test_zero_padded_channel_conv_footprint(stride):
    """A conv of the conditioning embedding: 16 real input channels and 32 real output channels inside the 64-wide granule
    (``k_valid`` = 16, zero weight rows and bias past 32), SiLU, both strides; the padding channels of the output are zero."""
    ops, L = _ops()
    from diffusers_amd.controlnet import _pad_conv
    B, H, W_, ci, co = 2, 6, 10, 16, 32
    w4, b = rnd((co, ci, 3, 3), 1, (9 * ci) ** -0.5), rnd((co,), 2)
    wp, bp = _pad_conv(w4, b)
    assert tuple(wp.shape) == (64, 9 * 64) and not wp.view(64, 9, 64)[:, :, ci:].any() and not wp[co:].any() and not bp[co:].any()
    x = torch.zeros((B, H, W_, 64), device=DEV, dtype=bf16)
    x[..., :ci] = rnd((B, H, W_, ci), 3)
    Ho, Wo = (H + 2 - 3) // stride + 1, (W_ + 2 - 3) // stride + 1
    results = []
    for kind in ("poisoned", "clean"):
        ins = {"x": poisoned(x), "w": poisoned(wp), "bias": poisoned(bp)}
        if kind == "clean":
            ins = {k: g.clean() for k, g in ins.items()}
        out = guarded((B, Ho, Wo, 64))
        before = {k: g.snapshot() for k, g in ins.items()}
        ops.conv2d_nhwc(ins["x"].view, ins["w"].view, ins["bias"].view, ksize=3, stride=stride, act=L.ACT_SILU, k_valid=ci, out=out.view)
        torch.cuda.synchronize()
        out.check(f"embedding conv output ({kind})")
        for k, g in ins.items():
            assert torch.equal(g.bits, before[k]), f"read-only operand {k} was written ({kind} run)"
        results.append(out.view.clone())
    assert bits_equal(results[0], results[1])
    got = results[0]
    assert not got[..., co:].any() and got[..., :co].abs().sum() > 0
    ref = F.silu(F.conv2d(x[..., :ci].float().permute(0, 3, 1, 2), w4.float(), b.float(), stride=stride, padding=1).to(bf16).float())
    assert CE.rel_rms(got[..., :co].permute(0, 3, 1, 2), ref) < 2.0 ** -8


# ---- 6. the model on the device ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model_case(flavour):
    """Inputs, the fp32 restatement and the bf16-on-CPU floor of one flavour, computed once and shared (read only)."""
    from diffusers_amd import factory, init as dinit
    ucfg = dinit.TINY_SDXL_UNET if flavour == "sdxl" else dinit.TINY_SD15_UNET
    cn, sd = factory.build_controlnet(ucfg, seed=3, device=DEV, conditioning_embedding_out_channels=(16, 32))
    g = torch.Generator().manual_seed(0)
    sample, ehs = torch.randn(2, 4, 16, 16, generator=g).to(bf16), torch.randn(2, 7, 64, generator=g).to(bf16)
    image = torch.rand(2, 3, 32, 32, generator=g).to(bf16).float()
    added = None
    if flavour == "sdxl":
        added = {"text_embeds": torch.randn(2, 64, generator=g).to(bf16), "time_ids": torch.tensor([[32., 32., 0., 0., 32., 32.]]).repeat(2, 1)}
    cfg, scale = dict(cn.config), 0.7

    def restated(dt):
        ad = None if added is None else {"text_embeds": added["text_embeds"].to(dt), "time_ids": added["time_ids"]}
        down, mid = CE.controlnet_forward(CE.cast(sd, dt), cfg, sample.to(dt), 801.0, ehs.to(dt), image.to(dt), scale, ad)
        return down + [mid]
    return cn, sample, ehs, image, added, scale, restated(f32), restated(bf16)


@pytest.mark.parametrize("flavour", ["sd15", "sdxl"])
def test_controlnet_forward_on_the_device(flavour):
    cn, sample, ehs, image, added, scale, ref, low = _model_case(flavour)
    ad = None if added is None else {k: v.to(DEV) for k, v in added.items()}
    out = cn(sample.to(DEV), 801.0, ehs.to(DEV), image.to(DEV), conditioning_scale=scale, added_cond_kwargs=ad)
    got = list(out.down_block_res_samples) + [out.mid_block_res_sample]
    for k, (gk, lo, r) in enumerate(zip(got, low, ref)):
        floor, err = CE.rel_rms(lo, r), CE.rel_rms(gk, r)
        print(f"[controlnet gpu {flavour}] residual {k}: engine {err:.3e}, bf16 restatement on the CPU (floor) {floor:.3e}")
        assert gk.dtype == bf16 and tuple(gk.shape) == tuple(r.shape) and err <= 1.5 * floor, (k, err, floor)
    # features + handoff_ on zero skips ARE forward's residuals
    cond = cn.precompute_conditioning(ehs.to(DEV), ad, image.to(DEV), conditioning_scale=scale)
    feats = cn.features(sample.to(DEV), cond, timestep=801.0)
    zeros = [torch.zeros_like(f) for f in feats]
    cn.handoff_(zeros[:-1], zeros[-1], feats, cond["gate"])
    for z, gk in zip(zeros, got):
        assert bits_equal(z.permute(0, 3, 1, 2).contiguous(), gk)
    # uint8 pixels through da_vae_conv_in_image, and the embedding's padding channels
    u8 = (image.permute(0, 2, 3, 1) * 255).round().to(torch.uint8).contiguous().to(DEV)
    emb = cn.precompute_conditioning(ehs.to(DEV), ad, u8)["embed"]
    assert tuple(emb.shape) == (2, 16, 16, 64) and not emb[..., 32:].any() and emb[..., :32].abs().sum() > 0
    same = cn.precompute_conditioning(ehs.to(DEV), ad, (u8.float() / 255.0).permute(0, 3, 1, 2).contiguous())["embed"]
    assert bits_equal(emb, same)


# ---- 7. / 8. the pipelines ---------------------------------------------------------------------------------------------------
def _pipe(flavour, controlnet=True, **kw):
    from diffusers_amd import factory
    build = factory.build_sdxl_pipeline if flavour == "sdxl" else factory.build_sd15_pipeline
    return build(device=DEV, tiny=True, controlnet=controlnet, **kw)


def _kw(flavour, seed=0, steps=4):
    g = torch.Generator().manual_seed(seed)
    kw = dict(prompt_embeds=torch.randn(1, 7, 64, generator=g).to(bf16), negative_prompt_embeds=torch.randn(1, 7, 64, generator=g).to(bf16),
              latents=torch.randn(1, 4, 16, 16, generator=g).to(bf16), num_inference_steps=steps, guidance_scale=5.0, output_type="latent")
    if flavour == "sdxl":
        kw.update(pooled_prompt_embeds=torch.randn(1, 64, generator=g).to(bf16),
                  negative_pooled_prompt_embeds=torch.randn(1, 64, generator=g).to(bf16))
    return kw


def _image(seed=11):
    return torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("flavour", ["sd15", "sdxl"])
def test_pipeline_identities(flavour):
    from diffusers_amd import factory, init as dinit, plan as P
    kw, img = _kw(flavour), _image()
    base = CS.run(_pipe(flavour, controlnet=False), dict(kw, height=32, width=32), True)
    pipe = _pipe(flavour)
    # scale 0, and a ControlNet whose zero convs are zero: the base pipeline's latents
    assert torch.equal(CS.run(pipe, dict(kw, image=img, controlnet_conditioning_scale=0.0), True), base)
    ucfg = dinit.TINY_SDXL_UNET if flavour == "sdxl" else dinit.TINY_SD15_UNET
    zero = factory.build_controlnet(ucfg, seed=3, device=DEV, zero_convs=True, conditioning_embedding_out_channels=(16, 32))[0]
    assert torch.equal(CS.run(_pipe(flavour, controlnet=zero), dict(kw, image=img), True), base)
    # graph = plan = eager
    eager = CS.run(_pipe(flavour), dict(kw, image=img), False)
    assert not torch.equal(eager, base)
    graph = CS.run(pipe, dict(kw, image=img), True)
    assert torch.equal(graph, eager)
    pp = _pipe(flavour)
    assert torch.equal(CS.run(pp, dict(kw, image=img), "plan"), eager)
    assert isinstance(pp._graph, P.Plan) and pp._graph.foreign_ops == [] and len(pp._graph) > 0       # recorded strict: no torch op
    # second calls: another image and another prompt replay the captured step, another scale captures again; each equals a
    # fresh pipeline's eager result
    g0 = pipe._graph
    kw2 = _kw(flavour, seed=5)
    for change, recapture in ((dict(image=_image(12)), False), (dict(kw2, latents=kw["latents"]), False),
                              (dict(controlnet_conditioning_scale=0.5), True)):
        call = dict(dict(kw, image=img), **change)
        got = CS.run(pipe, call, True)
        assert (pipe._graph is not g0) == recapture, sorted(change)
        g0 = pipe._graph
        assert torch.equal(got, CS.run(_pipe(flavour), call, False)), sorted(change)


@pytest.mark.parametrize("flavour", ["sd15", "sdxl"])
def test_pipeline_accuracy_against_the_fp32_oracle_loop(flavour):
    """PSNR of the 4-step latents against an fp32 loop around the restatement; the gate is relative: within 1 dB of what the BASE
    pipeline reaches against its own fp32 loop."""
    from diffusers_amd import factory, init as dinit
    kw, img = _kw(flavour), _image()
    ucfg = dinit.TINY_SDXL_UNET if flavour == "sdxl" else dinit.TINY_SD15_UNET
    from diffusers_amd.unet_2d_condition import UNet2DConditionModel
    from diffusers_amd.controlnet import ControlNetModel
    ufull = dict(UNet2DConditionModel(**ucfg).config)
    usd = CE.cast(dinit.random_state_dict(dinit.unet_param_shapes(ufull), seed=0), f32)
    ccfg = dict(ControlNetModel(**dinit.controlnet_config(ucfg, conditioning_embedding_out_channels=(16, 32))).config)
    csd = CE.cast(dinit.random_state_dict(dinit.controlnet_param_shapes(ccfg), seed=3), f32)
    ctx = torch.cat([kw["negative_prompt_embeds"], kw["prompt_embeds"]]).float()
    added = None
    if flavour == "sdxl":
        added = {"text_embeds": torch.cat([kw["negative_pooled_prompt_embeds"], kw["pooled_prompt_embeds"]]).float(),
                 "time_ids": torch.tensor([[32., 32., 0., 0., 32., 32.]]).repeat(2, 1)}
    image2 = torch.cat([img, img]).to(bf16).float()

    def plain(x, t):
        return CE.unet_forward(usd, ufull, x, t, ctx, added)

    def controlled(x, t):
        down, mid = CE.controlnet_forward(csd, ccfg, x, t, ctx, image2, 1.0, added)
        return CE.unet_forward(usd, ufull, x, t, ctx, added, down, mid)
    kind, scfg = ("euler", factory.SDXL_SCHEDULER) if flavour == "sdxl" else ("ddim", factory.SD15_SCHEDULER)
    want_base = CE.oracle_loop(kind, scfg, 4, 5.0, kw["latents"].float(), plain)
    want_cn = CE.oracle_loop(kind, scfg, 4, 5.0, kw["latents"].float(), controlled)
    got_base = CS.run(_pipe(flavour, controlnet=False), dict(kw, height=32, width=32), True)
    got_cn = CS.run(_pipe(flavour), dict(kw, image=img), True)
    p_base, p_cn = CE.psnr(got_base, want_base), CE.psnr(got_cn, want_cn)
    print(f"[controlnet gpu {flavour}] 4-step latents vs the fp32 oracle loop: ControlNet pipeline {p_cn:.2f} dB, base pipeline "
          f"{p_base:.2f} dB; the two oracles differ by {CE.psnr(want_cn, want_base):.2f} dB")
    assert p_base > 25.0, "the oracle loop does not describe the base pipeline"
    assert p_cn >= p_base - 1.0


# ---- 9. with the reference archive -------------------------------------------------------------------------------------------
@pytest.mark.skipif(not RR.available(), reason="reference archive oracle/_ref/diffusers_ref.zip did not ship")
@pytest.mark.parametrize("flavour", ["sd15", "sdxl"])
def test_against_the_reference_classes(flavour):
    """The reference ``ControlNetModel`` (fp32, same weights) against the engine's under the floor rule of test 6, and -- SDXL --
    the reference ``StableDiffusionXLControlNetPipeline.__call__`` against the engine pipeline under the rule of test 8."""
    from diffusers_amd import factory, init as dinit
    ref = RR.load_reference()
    cn, sample, ehs, image, added, scale, want, low = _model_case(flavour)
    ucfg = dinit.TINY_SDXL_UNET if flavour == "sdxl" else dinit.TINY_SD15_UNET
    csd = dinit.random_state_dict(dinit.controlnet_param_shapes(cn.config), seed=3)
    ccfg = dict(dinit.controlnet_config(ucfg, conditioning_embedding_out_channels=(16, 32)))
    rcn = RR.build_model(ref, "ControlNetModel", ccfg, csd, DEV, f32)
    ad = None if added is None else {k: v.to(DEV).float() for k, v in added.items()}
    with torch.no_grad():
        down, mid = rcn(sample.to(DEV).float(), torch.tensor(801.0, device=DEV), ehs.to(DEV).float(), image.to(DEV),
                        conditioning_scale=scale, added_cond_kwargs=ad, return_dict=False)
    out = cn(sample.to(DEV), 801.0, ehs.to(DEV), image.to(DEV), conditioning_scale=scale,
             added_cond_kwargs=None if added is None else {k: v.to(DEV) for k, v in added.items()})
    got = list(out.down_block_res_samples) + [out.mid_block_res_sample]
    for k, (gk, lo, r, rr) in enumerate(zip(got, low, want, list(down) + [mid])):
        assert CE.rel_rms(r, rr) < 1e-4, "the restatement is not the reference module"
        assert CE.rel_rms(gk, rr) <= 1.5 * CE.rel_rms(lo, rr)
    if flavour != "sdxl":
        return
    kw, img = _kw("sdxl"), _image()
    _, usd = factory.build_unet(ucfg, seed=0, device="cpu")
    _, vsd = factory.build_vae(dinit.TINY_VAE, seed=1, device="cpu")
    runet, rvae = RR.build_unet(ref, ucfg, usd, DEV, f32), RR.build_vae(ref, dinit.TINY_VAE, vsd, DEV, f32)
    common = dict(vae=rvae, text_encoder=None, text_encoder_2=None, tokenizer=None, tokenizer_2=None, unet=runet)
    rbase = ref.StableDiffusionXLPipeline(scheduler=ref.EulerDiscreteScheduler(**factory.SDXL_SCHEDULER), **common)
    rpipe = ref.StableDiffusionXLControlNetPipeline(controlnet=rcn, scheduler=ref.EulerDiscreteScheduler(**factory.SDXL_SCHEDULER), **common)
    rk = {k: (v.to(DEV).float() if torch.is_tensor(v) else v) for k, v in kw.items()}
    for p in (rbase, rpipe):
        p.set_progress_bar_config(disable=True)
    with torch.no_grad():
        want_base = rbase(height=32, width=32, **rk).images
        want_cn = rpipe(image=img.to(DEV), height=32, width=32, **rk).images
    p_base = CE.psnr(CS.run(_pipe("sdxl", controlnet=False), dict(kw, height=32, width=32), True), want_base)
    p_cn = CE.psnr(CS.run(_pipe("sdxl"), dict(kw, image=img), True), want_cn)
    print(f"[controlnet gpu sdxl] vs the reference pipelines: ControlNet {p_cn:.2f} dB, base {p_base:.2f} dB")
    assert p_cn >= p_base - 1.0
