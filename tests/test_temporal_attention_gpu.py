"""AnimateDiff on the engine.  The temporal attention kernel (csrc/attention_temporal.hip: attention over the frame axis of a frame-major token matrix, F <= 32,
D = 40 / 80 / 160) against fp64 under the suite's element-wise attention bound (attention_domain.TOL_DEFAULT, the gate of
test_kernels_gpu.py::test_flash_attention), its footprint and its refusals; one MotionModule (diffusers_amd/motion_adapter.py) against
a float64 restatement of the reference's AnimateDiffTransformer3D under the 1.5 x bf16-floor rule of the ControlNet / tiny-VAE tests;
the identities of AnimateDiffPipeline on the tiny factory configuration."""
import ctypes as C

import pytest
import torch

import attention_domain as ad
import footprint as FP

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
DEV = "cuda"


def _frame_major(t, B, HW):
    """[B*HW sequences][F][C] -> the engine's token matrix [(b F + f) HW + p][C]"""
    n, F, Cc = t.shape
    return t.view(B, HW, F, Cc).permute(0, 2, 1, 3).reshape(B * F * HW, Cc)


def _sequence_major(t, B, F, HW):
    return t.view(B, F, HW, -1).permute(0, 2, 1, 3).reshape(B * HW, F, -1)


def _run(q, k, v, B, HW, H, scale):
    """q / k / v [B*HW][F][C] (CPU) -> kernel output in the same arrangement; the operands are column views of ONE [rows][3C + 8]
    buffer (row stride != width), as the fused Q|K|V projection leaves them."""
    from diffusers_amd import ops
    n, F, Cc = q.shape
    qkv = torch.randn((B * F * HW, 3 * Cc + 8), generator=torch.Generator("cpu").manual_seed(1)).to(bf16)
    for i, t in enumerate((q, k, v)):
        qkv[:, i * Cc:(i + 1) * Cc] = _frame_major(t, B, HW)
    qkv = qkv.to(DEV)
    out = ops.temporal_attention(qkv[:, :Cc], qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:3 * Cc], B=B, F=F, HW=HW, H=H, D=Cc // H, scale=scale)
    return _sequence_major(out.cpu(), B, F, HW)


# HW: the issue's {1, 3, P, P + 1} with P = 1 pixel per workgroup, duplicates dropped
@pytest.mark.parametrize("B,H", [(1, 1), (1, 8), (2, 1), (2, 8)])
@pytest.mark.parametrize("HW", [1, 2, 3])
@pytest.mark.parametrize("F", [1, 2, 15, 16, 17, 32])
@pytest.mark.parametrize("D", [40, 80, 160])
def test_temporal_attention_against_fp64(D, F, HW, B, H):
    scale = ad.default_scale(D)
    q, k, v = ad.family("vscale", 0.0, B * HW, H, F, F, D, scale, seed=D + F + HW + B + H)              # (V * 2^0: plain N(0, 1))
    fails = ad.check(_run(q, k, v, B, HW, H, scale), ad.attention_ref64(q, k, v, H, scale), None,
                     f"temporal D{D} F{F} HW{HW} B{B} H{H}", ad.TOL_DEFAULT)
    assert not fails, "\n".join(fails)


HOSTILE = [("offset", 3000.0), ("offset", -3000.0), ("rowmix", 3000.0), ("onehot", 0.0), ("vscale", 100.0)]


@pytest.mark.parametrize("kind,level", HOSTILE, ids=[ad.family_id(f) for f in HOSTILE])
def test_temporal_attention_on_hostile_scores(kind, level):
    D, F, B, H, HW = 40, 32, 1, 2, 2
    scale = ad.default_scale(D)
    q, k, v = ad.family(kind, level, B * HW, H, F, F, D, scale, seed=7)
    out = _run(q, k, v, B, HW, H, scale)
    fails = ad.check(out, ad.attention_ref64(q, k, v, H, scale), None, f"temporal {ad.family_id((kind, level))}", ad.TOL_DEFAULT)
    if kind == "onehot":
        fails += ad.check_onehot(out, v, F, "temporal onehot")
    assert not fails, "\n".join(fails)


def test_torch_op_takes_the_3d_form_without_a_copy_and_refuses_the_rest():
    from diffusers_amd import ops, torch_ops  # noqa: F401
    B, F, HW, H, D = 2, 16, 5, 8, 40
    Cc = H * D
    qkv = torch.randn((B * F, HW, 3 * Cc), generator=torch.Generator("cpu").manual_seed(3)).to(bf16)
    q, k, v = qkv.to(DEV).chunk(3, -1)
    got = torch.ops.mi355x.temporal_attn(q, k, v, F, H, None)
    seq = [_sequence_major(t.reshape(B * F * HW, Cc), B, F, HW) for t in qkv.chunk(3, -1)]
    fails = ad.check(_sequence_major(got.cpu().view(B * F * HW, Cc), B, F, HW), ad.attention_ref64(*seq, H, ad.default_scale(D)), None,
                     "torch op B2", ad.TOL_DEFAULT)
    assert got.shape == q.shape and not fails, "\n".join(fails)
    with pytest.raises(ValueError, match="does not carry HW"):
        torch.ops.mi355x.temporal_attn(*(t.reshape(B * F * HW, Cc) for t in (q, k, v)), F, H, None)
    with pytest.raises(ValueError, match="it is not copied"):
        torch.ops.mi355x.temporal_attn(q, k, v.transpose(0, 1).contiguous().transpose(0, 1), F, H, None)


@pytest.mark.parametrize("D", [40, 80, 160])
def test_temporal_attention_footprint(D):
    """Q | K | V inside one poisoned [rows][3C] (+ 8 sentinel columns) buffer, `out` a column block of a wider guarded buffer: nothing
    outside the B F HW x H D block is written, and the surroundings of the inputs do not reach the output."""
    from diffusers_amd import ops
    B, F, HW, H = 2, 17, 2, 8
    Cc, rows, pad = H * D, B * F * HW, 32
    vals = torch.randn((rows, 3 * Cc), generator=torch.Generator("cpu").manual_seed(D)).to(bf16)
    qkv = FP.poisoned(vals, ld=3 * Cc + 8)
    outs = []
    for src in (qkv, qkv.clean()):
        o = FP.guarded((rows, Cc + 2 * pad), ld=Cc + 2 * pad + 8)
        o.view.fill_(-7.0)
        ops.temporal_attention(*(src.view[:, i * Cc:(i + 1) * Cc] for i in range(3)), B=B, F=F, HW=HW, H=H, D=D,
                               out=o.view[:, pad:pad + Cc])
        torch.cuda.synchronize()
        o.check(f"temporal attention D{D}: out"), src.check(f"temporal attention D{D}: qkv")
        assert bool((o.view[:, :pad] == -7.0).all()) and bool((o.view[:, pad + Cc:] == -7.0).all()), "columns beside the block written"
        outs.append(o.view[:, pad:pad + Cc].clone())
    assert bool(torch.isfinite(outs[0].float()).all()) and FP.bits_equal(outs[0], outs[1])
    q, k, v = (_sequence_major(vals[:, i * Cc:(i + 1) * Cc], B, F, HW) for i in range(3))
    fails = ad.check(_sequence_major(outs[0].cpu(), B, F, HW), ad.attention_ref64(q, k, v, H, ad.default_scale(D)), None,
                     f"footprint D{D}", ad.TOL_DEFAULT)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("bad", [dict(F=0), dict(F=33), dict(D=64), dict(q_row_stride=324), dict(out=8)], ids=lambda b: str(b))
def test_temporal_attention_refusals_never_launch(bad):
    """The library refuses by return value before any launch; ops names a misaligned stride or base."""
    from diffusers_amd import _lib as L, ops
    B, F, HW, H, D = 1, 16, 3, 8, 40
    buf = torch.zeros((B * 33 * HW, 3 * H * D + 8), dtype=bf16, device=DEV)
    p = L.AttentionTemporalParams()
    p.q, p.k, p.v, p.out = (buf.data_ptr() + 2 * i * H * D for i in (0, 1, 2, 0))
    p.B, p.F, p.HW, p.H, p.D, p.scale = B, F, HW, H, D, D ** -0.5
    p.q_row_stride = p.k_row_stride = p.v_row_stride = p.o_row_stride = buf.shape[1]
    for key, val in bad.items():
        setattr(p, key, p.out + val if key == "out" else val)
    assert L.load().da_attention_temporal_bf16(C.byref(p), None) == ops.DA_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert not bool(buf.any())
    if "q_row_stride" in bad or "out" in bad:
        t = torch.zeros((B * F * HW, 3 * H * D + 4), dtype=bf16, device=DEV)
        views = [t[:, i * H * D:(i + 1) * H * D] for i in range(3)]
        out = torch.zeros((B * F * HW * H * D + 4,), dtype=bf16, device=DEV)[4:].view(B * F * HW, H * D) if "out" in bad else None
        if out is not None:
            views = [v.contiguous() for v in views]
        with pytest.raises(ValueError, match="multiple of 8 elements and a 16-byte aligned"):
            ops.temporal_attention(*views, B=B, F=F, HW=HW, H=H, D=D, out=out)


# ---- MotionModule against the reference's AnimateDiffTransformer3D, restated -----------------------------------------------------------
def _restated(x, sd, dtype, F, heads=8, per_frame_groupnorm=False):
    """x [B*F][HW][C]; the reference's module with torch ops in `dtype`, INCLUDING the permute to (B HW, F, C) the engine avoids."""
    from diffusers_amd.motion_adapter import sinusoidal_pe
    nn = torch.nn.functional
    w = {k[len("m."):]: t.to(dtype) for k, t in sd.items()}
    BF, HW, Cc = x.shape
    B, tb = BF // F, "transformer_blocks.0."
    x = x.to(dtype)
    slabs = x.view(BF, HW, Cc) if per_frame_groupnorm else x.view(B, F * HW, Cc)
    h = nn.group_norm(slabs.transpose(1, 2), 32, w["norm.weight"], w["norm.bias"], 1e-6).transpose(1, 2).reshape(B, F, HW, Cc)
    h = h.permute(0, 2, 1, 3).reshape(B * HW, F, Cc)
    h = h @ w["proj_in.weight"].t() + w["proj_in.bias"]
    pe = sinusoidal_pe(Cc)[:F].to(dtype)
    for i in (1, 2):
        n = nn.layer_norm(h, (Cc,), w[f"{tb}norm{i}.weight"], w[f"{tb}norm{i}.bias"], 1e-5) + pe
        q, k, v = ((n @ w[f"{tb}attn{i}.to_{c}.weight"].t()).view(B * HW, F, heads, Cc // heads).transpose(1, 2) for c in "qkv")
        o = torch.softmax(q @ k.transpose(2, 3) * (Cc // heads) ** -0.5, -1) @ v
        h = h + o.transpose(1, 2).reshape(B * HW, F, Cc) @ w[f"{tb}attn{i}.to_out.0.weight"].t() + w[f"{tb}attn{i}.to_out.0.bias"]
    n = nn.layer_norm(h, (Cc,), w[f"{tb}norm3.weight"], w[f"{tb}norm3.bias"], 1e-5)
    val, gate = (n @ w[f"{tb}ff.net.0.proj.weight"].t() + w[f"{tb}ff.net.0.proj.bias"]).chunk(2, -1)
    h = h + (val * nn.gelu(gate)) @ w[f"{tb}ff.net.2.weight"].t() + w[f"{tb}ff.net.2.bias"]
    h = h.view(B, HW, F, Cc).permute(0, 2, 1, 3).reshape(BF, HW, Cc)
    return h @ w["proj_out.weight"].t() + w["proj_out.bias"] + x


def test_motion_module_against_the_restated_reference():
    """C = 320, F = 16, HW = 8 x 8, B = 2.  Gate: rel-rms to fp64 <= 1.5 x that of the same restatement run in bf16.  A restatement
    whose GroupNorm normalises per frame is further from the engine than the gate allows: the statistics span all F frames."""
    from diffusers_amd import init as dinit
    from diffusers_amd.layers import Weights
    from diffusers_amd.motion_adapter import MotionModule, motion_adapter_param_shapes
    cfg = dict(block_out_channels=(320,), motion_layers_per_block=1, motion_mid_block_layers_per_block=1, use_motion_mid_block=False)
    shapes = {k.replace("down_blocks.0.motion_modules.0.", "m."): s for k, s in motion_adapter_param_shapes(cfg).items()
              if k.startswith("down_blocks.0.motion_modules.0.")}
    sd = dinit.random_state_dict(shapes, seed=11)
    B, F, HW, Cc = 2, 16, 64, 320
    x = torch.randn((B * F, HW, Cc), generator=torch.Generator("cpu").manual_seed(5))
    x = (x * (0.5 + torch.arange(B * F) % F / F)[:, None, None]).to(bf16)       # frames differ in scale: per-frame statistics would hide it
    got = MotionModule(Weights(sd, DEV), "m")(x.to(DEV), F).cpu()
    ref = _restated(x, sd, torch.float64, F)
    err, floor = ad.rel_rms64(got, ref), ad.rel_rms64(_restated(x, sd, bf16, F), ref)
    wrong = ad.rel_rms64(got, _restated(x, sd, torch.float64, F, per_frame_groupnorm=True))
    print(f"[motion module] engine {err:.3e}, bf16 restatement (floor) {floor:.3e}, against a per-frame GroupNorm {wrong:.3e}")
    assert got.shape == x.shape and err <= 1.5 * floor, (err, floor)
    assert wrong > 1.5 * floor, "a per-frame GroupNorm reference must fail this test"


def test_motion_adapter_builds_by_block_and_refuses_what_is_not_built():
    from diffusers_amd import MotionAdapter, factory
    ad_, sd = factory.build_motion_adapter(dict(block_out_channels=(320, 640)), motion_layers_per_block=1)
    assert [len(b) for b in ad_.down] == [1, 1] and [len(b) for b in ad_.up] == [2, 2] and len(ad_.mid) == 1
    assert [m.channels for b in ad_.up for m in b] == [640, 640, 320, 320] and ad_.mid[0].channels == 640
    x = torch.randn((2 * 3, 2, 2, 640), generator=torch.Generator("cpu").manual_seed(9)).to(bf16).to(DEV)
    y = ad_.mid[0](x, 3)
    assert y.shape == x.shape and bool(torch.isfinite(y.float()).all()) and not torch.equal(y, x)
    with pytest.raises(NotImplementedError, match="context windows"):
        ad_.mid[0](x.repeat(11, 1, 1, 1), 33)
    with pytest.raises(NotImplementedError, match="motion LoRA"):
        ad_.load_lora_weights("some/dir")
    with pytest.raises(NotImplementedError, match="motion_max_seq_length"):
        MotionAdapter(motion_max_seq_length=64)
    with pytest.raises(ValueError, match="unexpected keys"):
        MotionAdapter.from_state_dict(dict(sd, bogus=torch.zeros(1)), block_out_channels=(320, 640), motion_layers_per_block=1)


# ---- AnimateDiffPipeline on the tiny configuration (two levels, 320 / 640 channels, 8 x 8 latents) -------------------------------------
@pytest.fixture(scope="module")
def pipe():
    from diffusers_amd import factory
    return factory.build_animatediff_pipeline(tiny=True)


def _embeds(seed):
    g = torch.Generator("cpu").manual_seed(seed)
    return g, dict(prompt_embeds=torch.randn((1, 8, 64), generator=g).to(bf16), negative_prompt_embeds=torch.randn((1, 8, 64), generator=g).to(bf16),
                   height=16, width=16, num_inference_steps=3, guidance_scale=5.0)


def _video(pipe, seed, F, use_graph, **kw):
    g, args = _embeds(seed)
    return pipe(num_frames=F, generator=g, use_graph=use_graph, **{**args, "output_type": "latent", **kw}).images


def test_pipeline_eager_equals_graph_and_the_graph_key_carries_num_frames(pipe):
    """Five frames under CFG: ten rows of time embedding, past the eight one skinny-linear launch takes."""
    eager = {(s, F): _video(pipe, s, F, False).clone() for s, F in ((1, 5), (2, 5), (1, 2))}
    assert eager[1, 5].shape == (1, 4, 5, 8, 8) and bool(torch.isfinite(eager[1, 5].float()).all())
    assert not torch.equal(eager[1, 5][:, :, 0], eager[1, 5][:, :, 1])
    assert torch.equal(_video(pipe, 1, 5, True), eager[1, 5])
    captured = pipe._graph
    assert torch.equal(_video(pipe, 2, 5, True), eager[2, 5]) and pipe._graph is captured, "another seed replays"
    assert torch.equal(_video(pipe, 1, 2, True), eager[1, 2]) and pipe._graph is not captured, "another num_frames recaptures"
    # decoded two frames at a time: frames 0-1, 2-3 and 4 of the same latents through the VAE, in order
    from diffusers_amd.pipelines import decode_postprocessed
    chunked = _video(pipe, 1, 5, True, output_type="pt", decode_chunk_size=2)
    frames = eager[1, 5][0].transpose(0, 1).contiguous()
    parts = [decode_postprocessed(pipe.vae, frames[i:i + 2], "pt", latents_div=float(pipe.vae.config.scaling_factor)) for i in (0, 2, 4)]
    assert chunked.shape == (1, 5, 3, 16, 16) and torch.equal(chunked[0], torch.cat(parts))


def test_one_frame_with_zeroed_proj_out_is_the_stable_diffusion_pipeline(pipe):
    """The reference zero-initialises proj_out: a module then adds nothing, and one frame is one image, to the bit."""
    from diffusers_amd import DDIMScheduler, StableDiffusionPipeline, factory, init as dinit
    ad_ = pipe.motion_adapter
    for m in [m for b in ad_.down + ad_.up for m in b] + ad_.mid:
        m.proj_out.weight.zero_(), m.proj_out.bias.zero_()
    sd = StableDiffusionPipeline(vae=pipe.vae, unet=factory.build_unet(dinit.TINY_ANIMATEDIFF_UNET, seed=0)[0],
                                 scheduler=DDIMScheduler(**factory.SD15_SCHEDULER))
    lat = torch.randn((1, 4, 8, 8), generator=torch.Generator("cpu").manual_seed(4)).to(bf16)
    for use_graph in (False, True):
        video = pipe(num_frames=1, latents=lat[:, :, None], use_graph=use_graph, **_embeds(5)[1]).images
        image = sd(latents=lat, use_graph=use_graph, **_embeds(5)[1]).images
        assert video.shape == (1, 1, 3, 16, 16) and torch.equal(video[:, 0], image)


def test_pipeline_refuses_by_name_what_is_not_built(pipe):
    from diffusers_amd import UNetMotionModel, factory, init as dinit
    args = _embeds(1)[1]
    for kw, what in ((dict(use_graph="plan"), "launch-plan"), (dict(num_frames=33), "context windows"), (dict(video=[0]), "video-to-video"),
                     (dict(conditioning_frames=[0]), "SparseCtrl")):
        with pytest.raises(NotImplementedError, match=what):
            pipe(**dict(args, **kw))
    for call, what in ((lambda: pipe.enable_freeu(0.9, 0.2, 1.2, 1.4), "FreeU"), (pipe.enable_free_noise, "FreeNoise"),
                       (lambda: pipe.load_lora_weights("dir"), "motion LoRA"),
                       (lambda: UNetMotionModel.from_unet2d(factory.build_unet(dinit.TINY_SDXL_UNET)[0], pipe.motion_adapter), "SDXL")):
        with pytest.raises(NotImplementedError, match=what):
            call()
