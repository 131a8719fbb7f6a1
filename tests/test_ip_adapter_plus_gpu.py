"""IP-Adapter Plus: ip_adapter.Resampler against IPAdapterPlusImageProjection restated in float64, and the tiny SD 1.5 / SDXL
pipelines with a seeded plus adapter (factory ``ip_adapter=["plus"]``: 8 latents, width 128, 2 layers over 17 x 128 hidden states).
The attention kernel itself is tests/test_resampler_attention_gpu.py."""
import pytest
import torch

import attention_domain as ad

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
F = torch.nn.functional
KINDS = ["sd15", "sdxl"]


def _restated(sd, x, dt):
    """IPAdapterPlusImageProjection in `dt`: [B][n_img][S0][embed] -> [B][n_img * Nq][cross]."""
    w = {k: v.to(dt) for k, v in sd.items()}
    ln = lambda t, p: F.layer_norm(t, (t.shape[-1],), w[p + ".weight"], w[p + ".bias"], 1e-5)  # noqa: E731
    split = lambda t: t.view(t.shape[0], t.shape[1], -1, 64).transpose(1, 2)  # noqa: E731
    B, n_img, S0, E = x.shape
    x = x.to(dt).reshape(B * n_img, S0, E) @ w["proj_in.weight"].t() + w["proj_in.bias"]
    lat = w["latents"].repeat(B * n_img, 1, 1)
    i = 0
    while f"layers.{i}.0.to_q.weight" in w:
        p = f"layers.{i}."
        e, l = ln(x, p + "0.norm1"), ln(lat, p + "0.norm2")
        k, v = (torch.cat([e, l], 1) @ w[p + "0.to_kv.weight"].t()).chunk(2, -1)
        a = torch.softmax(split(l @ w[p + "0.to_q.weight"].t()) @ split(k).transpose(2, 3) * 0.125, -1) @ split(v)
        lat = a.transpose(1, 2).reshape(lat.shape[0], lat.shape[1], -1) @ w[p + "0.to_out.weight"].t() + lat
        lat = F.gelu(ln(lat, p + "1.0") @ w[p + "1.1.weight"].t()) @ w[p + "1.3.weight"].t() + lat
        i += 1
    return ln(lat @ w["proj_out.weight"].t() + w["proj_out.bias"], "norm_out").reshape(B, -1, w["proj_out.weight"].shape[0])


@pytest.mark.parametrize("size", ["tiny", "sd15"])
def test_resampler_against_fp64(size):
    """Gate: rel-rms to fp64 <= FLOOR_FACTOR x that of the same restatement run in bf16 on the same inputs."""
    from diffusers_amd import factory, init as dinit, ip_adapter as I
    cfg, kw, (n_img, S0) = (dinit.TINY_SD15_UNET, dict(num_tokens=8, image_embed_dim=64, dim=128, depth=2), (2, 17)) if size == "tiny" else \
        (dinit.SD15_UNET, dict(num_tokens=16, image_embed_dim=1280, dim=768, depth=4), (1, 257))
    sd = factory.build_ip_adapter_state_dict(cfg, plus=True, seed=9, **kw)["image_proj"]
    x = torch.randn((2, n_img, S0, kw["image_embed_dim"]), generator=torch.Generator("cpu").manual_seed(1)).to(bf16)
    proj = I.Resampler(sd, cfg["cross_attention_dim"], "cuda")
    got, ref = proj(x.cuda()).cpu(), _restated(sd, x, torch.float64)
    err, floor = ad.rel_rms64(got, ref), ad.rel_rms64(_restated(sd, x, bf16), ref)
    print(f"[resampler {size}] engine {err:.3e}, bf16 restatement (floor) {floor:.3e}")
    assert proj.heads == kw["dim"] // 64 and got.shape == ref.shape == (2, n_img * kw["num_tokens"], cfg["cross_attention_dim"])
    assert err <= ad.FLOOR_FACTOR * floor, (err, floor)


def _build(kind, **kw):
    from diffusers_amd import factory
    return (factory.build_sdxl_pipeline if kind == "sdxl" else factory.build_sd15_pipeline)(tiny=True, **kw)


@pytest.fixture(scope="module", params=KINDS)
def pipes(request):
    return request.param, _build(request.param, ip_adapter=["plus"]), _build(request.param)


def _args(kind, seed):
    g = torch.Generator("cpu").manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=g).to(bf16)  # noqa: E731
    kw = dict(prompt_embeds=r(1, 8, 64), negative_prompt_embeds=r(1, 8, 64), height=16, width=16, num_inference_steps=3, guidance_scale=5.0,
              output_type="latent", generator=g)
    if kind == "sdxl":
        kw.update(pooled_prompt_embeds=r(1, 64), negative_pooled_prompt_embeds=r(1, 64))
    return kw, r


def _run(pipe, kind, seed, use_graph, ip=True):
    kw, r = _args(kind, seed)
    embeds = [r(2, 2, 17, 128)]                     # (drawn either way: the latents come from the same generator)
    return pipe(use_graph=use_graph, **kw, **({"ip_adapter_image_embeds": embeds} if ip else {})).images.clone()


def test_eager_equals_graph_embeds_replay_and_scale_zero(pipes):
    kind, pipe, plain = pipes
    pipe.set_ip_adapter_scale(0.7)
    eager = {s: _run(pipe, kind, s, False) for s in (1, 2)}
    assert bool(torch.isfinite(eager[1].float()).all()) and not torch.equal(eager[1], _run(plain, kind, 1, False, ip=False))
    assert torch.equal(_run(pipe, kind, 1, True), eager[1])
    captured = pipe._graph
    assert torch.equal(_run(pipe, kind, 2, True), eager[2]) and pipe._graph is captured, "new embeds of the same shape replay"
    pipe.set_ip_adapter_scale(0.0)
    for g in (False, True):
        assert torch.equal(_run(pipe, kind, 3, g), _run(plain, kind, 3, g, ip=False)), "scale 0"


def test_base_and_plus_together_and_refusals_by_name(pipes):
    from diffusers_amd import factory, init as dinit
    kind, pipe, plain = pipes
    kw, r = _args(kind, 1)
    both = _build(kind, ip_adapter=[4, "plus"])
    got = both(**kw, ip_adapter_image_embeds=[r(2, 1, 64), r(2, 1, 17, 128)]).images
    assert bool(torch.isfinite(got.float()).all()) and not torch.equal(got, _run(plain, kind, 1, True, ip=False))
    with pytest.raises(NotImplementedError, match="more than 32 image tokens"):
        pipe(**kw, ip_adapter_image_embeds=[r(2, 5, 17, 128)])
    sd = factory.build_ip_adapter_state_dict(dinit.TINY_SDXL_UNET if kind == "sdxl" else dinit.TINY_SD15_UNET, plus=True, num_tokens=8,
                                             image_embed_dim=128, dim=128, depth=2)
    proj = sd["image_proj"]
    with pytest.raises(NotImplementedError, match="FaceID"):
        plain.load_ip_adapter(dict(sd, image_proj={"proj.0.weight": torch.zeros(8, 8), "norm.weight": torch.zeros(8)}))
    with pytest.raises(NotImplementedError, match=r"Resampler.*'layers\.1\.0\.to_out\.weight' is missing"):
        plain.load_ip_adapter(dict(sd, image_proj={k: v for k, v in proj.items() if k != "layers.1.0.to_out.weight"}))
    with pytest.raises(NotImplementedError, match=r"Resampler.*'extra' is unexpected"):
        plain.load_ip_adapter(dict(sd, image_proj=dict(proj, extra=torch.zeros(1))))


def test_image_through_the_engine_encoder_equals_hidden_states_by_hand():
    from diffusers_amd import factory
    pipe = factory.build_sd15_pipeline(tiny=True, ip_adapter=["plus"])
    enc = factory.build_clip_vision(dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, hidden_act="quick_gelu", image_size=56,
                                         patch_size=14, projection_dim=64, intermediate_size=256), seed=3)[0]
    pipe.image_encoder = enc
    kw, _ = _args("sd15", 2)
    img = torch.randint(0, 256, (90, 120, 3), generator=torch.Generator("cpu").manual_seed(1), dtype=torch.uint8)
    run = lambda **k: pipe(**dict(kw, generator=torch.Generator("cpu").manual_seed(4)), **k).images.clone()  # noqa: E731
    pos = enc.encode_image(img, output_hidden_states=True, return_embeds=False).hidden_states[-2]
    neg = enc(pixel_values=torch.zeros(1, 3, 56, 56), output_hidden_states=True).hidden_states[-2]
    assert pos.shape == (1, 17, 128)
    assert torch.equal(run(ip_adapter_image=img), run(ip_adapter_image_embeds=[torch.stack([neg, pos])]))
