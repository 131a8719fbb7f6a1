"""IP-Adapter on the tiny SD 1.5 and SDXL pipelines (factory ``ip_adapter=``: two adapters of 4 and 8 image tokens): the identities of
the captured step, scales, unloading and the refusals.  The kernel and the layer are tests/test_ip_attention_gpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
KINDS = ["sd15", "sdxl"]


def _build(kind, **kw):
    from diffusers_amd import factory
    return (factory.build_sdxl_pipeline if kind == "sdxl" else factory.build_sd15_pipeline)(tiny=True, **kw)


@pytest.fixture(scope="module", params=KINDS)
def pipes(request):
    return request.param, _build(request.param, ip_adapter=[4, 8]), _build(request.param)


def _args(kind, seed):
    g = torch.Generator("cpu").manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=g).to(bf16)  # noqa: E731
    kw = dict(prompt_embeds=r(1, 8, 64), negative_prompt_embeds=r(1, 8, 64), height=16, width=16, num_inference_steps=3, guidance_scale=5.0,
              output_type="latent", generator=g)
    if kind == "sdxl":
        kw.update(pooled_prompt_embeds=r(1, 64), negative_pooled_prompt_embeds=r(1, 64))
    return kw, [r(2, 1, 64), r(2, 2, 64)]           # one image for the first adapter, two for the second: 4 and 16 tokens


def _run(pipe, kind, seed, use_graph, ip=True):
    kw, embeds = _args(kind, seed)
    return pipe(use_graph=use_graph, **kw, **({"ip_adapter_image_embeds": embeds} if ip else {})).images.clone()


def test_eager_equals_graph_embeds_replay_and_a_scale_recaptures(pipes):
    kind, pipe, plain = pipes
    pipe.set_ip_adapter_scale([0.7, -0.4])
    eager = {s: _run(pipe, kind, s, False) for s in (1, 2)}
    assert bool(torch.isfinite(eager[1].float()).all()) and not torch.equal(eager[1], _run(plain, kind, 1, False, ip=False))
    assert torch.equal(_run(pipe, kind, 1, True), eager[1])
    captured = pipe._graph
    assert torch.equal(_run(pipe, kind, 2, True), eager[2]) and pipe._graph is captured, "new embeds of the same shape replay"
    pipe.set_ip_adapter_scale(0.5)
    assert torch.equal(_run(pipe, kind, 1, True), _run(pipe, kind, 1, False)) and pipe._graph is not captured, "a new scale recaptures"


def test_scale_zero_and_unload_equal_the_pipeline_without_an_adapter(pipes):
    kind, pipe, plain = pipes
    want = {g: _run(plain, kind, 3, g, ip=False) for g in (False, True)}
    pipe.set_ip_adapter_scale(0.0)
    for g in (False, True):
        assert torch.equal(_run(pipe, kind, 3, g), want[g]), "scale 0"
    fresh = _build(kind, ip_adapter=[4, 8])
    fresh.unload_ip_adapter()
    assert fresh.unet.encoder_hid_proj is None
    for g in (False, True):
        assert torch.equal(_run(fresh, kind, 3, g, ip=False), want[g]), "unloaded"


def test_refusals_by_name(pipes):
    from diffusers_amd import factory, init as dinit
    kind, pipe, plain = pipes
    kw, embeds = _args(kind, 1)
    cfg = dinit.TINY_SDXL_UNET if kind == "sdxl" else dinit.TINY_SD15_UNET
    for extra, err, what in ((dict(use_graph="plan", ip_adapter_image_embeds=embeds), NotImplementedError, "launch-plan number"),
                             (dict(ip_adapter_image=torch.zeros(1, 3, 8, 8)), NotImplementedError, "ip_adapter_image_embeds"),
                             (dict(), ValueError, "an IP-Adapter is loaded"),
                             (dict(ip_adapter_image_embeds=embeds, ip_adapter_masks=[0]), NotImplementedError, "ip_adapter_masks"),
                             (dict(ip_adapter_image_embeds=[embeds[0], embeds[1].repeat(1, 3, 1)]), NotImplementedError, "more than 32 image tokens")):
        with pytest.raises(err, match=what):
            pipe(**kw, **extra)
    with pytest.raises(ValueError, match="need an IP-Adapter"):
        plain(**kw, ip_adapter_image_embeds=embeds)
    with pytest.raises(NotImplementedError, match="per-block"):
        pipe.set_ip_adapter_scale({"down": 1.0})
    sd = factory.build_ip_adapter_state_dict(cfg, image_embed_dim=64)
    with pytest.raises(NotImplementedError, match="1 .. 4 at once"):
        plain.load_ip_adapter([sd] * 5)
    with pytest.raises(NotImplementedError, match="Resampler"):
        plain.load_ip_adapter(dict(sd, image_proj={"latents": torch.zeros(1, 16, 64)}))
    from diffusers_amd.pipelines import FluxPipeline
    for other, what in ((factory.build_sd15_pipeline(tiny=True, pix2pix=True), "InstructPix2Pix"),
                        (factory.build_animatediff_pipeline(tiny=True), "AnimateDiff"), (FluxPipeline.__new__(FluxPipeline), "FLUX")):
        with pytest.raises(NotImplementedError, match=what):
            other.load_ip_adapter(sd)


def test_image_projection_against_fp64():
    """ImageProjection (Linear, reshape, LayerNorm) against torch in float64 under 1.5 x the same restatement in bf16."""
    import attention_domain as ad
    from diffusers_amd import factory, init as dinit, ip_adapter as I
    nn = torch.nn.functional
    sd = factory.build_ip_adapter_state_dict(dinit.TINY_SD15_UNET, num_tokens=4, image_embed_dim=64)
    x = torch.randn((2, 3, 64), generator=torch.Generator("cpu").manual_seed(1)).to(bf16)
    got = I.ImageProjection(sd["image_proj"], 64, "cuda")(x.cuda()).cpu()

    def restated(dt):
        w = {k: v.to(dt) for k, v in sd["image_proj"].items()}
        y = (x.to(dt).reshape(6, 64) @ w["proj.weight"].t() + w["proj.bias"]).reshape(2, 12, 64)
        return nn.layer_norm(y, (64,), w["norm.weight"], w["norm.bias"], 1e-5)
    ref = restated(torch.float64)
    err, floor = ad.rel_rms64(got, ref), ad.rel_rms64(restated(bf16), ref)
    print(f"[image projection] engine {err:.3e}, bf16 restatement (floor) {floor:.3e}")
    assert got.shape == (2, 12, 64) and err <= 1.5 * floor, (err, floor)
