"""GPU: da_clip_patch_embed (csrc/clip_patch_embed.hip) against float64, its footprint and refusals; the CLIP vision encoder against
``transformers`` in float64; ``encode_image`` against CLIPImageProcessor; ``ip_adapter_image=`` in the tiny SD 1.5 pipeline.

Kernel bound.  The reference restates the header's arithmetic in float64 from the same bf16 weights and the pixel the kernel forms (fp32
``(u8 / 255 - mean) * inv_std`` rounded to bf16).  With T = sum_k |v_k| |w_k| + |pos| the fp32 row is within EPS32 T of it (EPS32 = 2^-20:
the suite's fp32 rule, tests/test_dpmsolver_cpu.py), so ``emb_out`` is within 2^-8 |e| + EPS32 T (one bf16 rounding).  The LayerNorm maps
an input error d (row maximum dm) to at most |gamma| rstd (d + dm) (the element, the mean) + |y - beta| rstd dm (the variance: d rstd /
rstd <= rstd dm), its own few fp32 roundings stay under 4 EPS32 (|y - beta| + |beta|); ``x_out`` adds one bf16 rounding, 2^-8 |y|."""
import pytest
import torch
import torch.nn.functional as F

import attention_domain as ad
import footprint as FP
from test_dpmsolver_cpu import EPS32

pytestmark = pytest.mark.gpu

bf16, f64 = torch.bfloat16, torch.float64
DEV = "cuda"
MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
EPS = 1e-5
SHAPES = [(128, 14, 28), (256, 14, 42), (1280, 14, 98), (1664, 14, 28), (128, 16, 32), (128, 32, 64)]


def _inputs(hidden, P, S, B, mode, seed, constant=False):
    """(image, crop, pixels fp32 [B][3][S][S] as the kernel forms them, weights): full-range bytes in a non-square source."""
    g = torch.Generator("cpu").manual_seed(seed)
    n = 1 + (S // P) ** 2
    r = lambda *s: torch.randn(s, generator=g)  # noqa: E731
    w = dict(weight=((torch.rand((hidden, 3, P, P), generator=g) * 2 - 1) * (3 * P * P) ** -0.5).to(bf16), cls=(0.5 * r(hidden)).to(bf16),
             pos=(0.1 * r(n, hidden)).to(bf16), gamma=(1 + 0.1 * r(hidden)).to(bf16), beta=(0.05 * r(hidden)).to(bf16))
    if mode == "f32":
        img = torch.full((B, 3, S, S), 0.7) if constant else 1.5 * r(B, 3, S, S)
        return img, (0, 0), img, w
    img = torch.randint(0, 256, (B, S + 5, S + 9, 3), generator=g, dtype=torch.uint8)
    if constant:
        img[:] = 200
    top, left = 3, 6
    crop = img[:, top:top + S, left:left + S].permute(0, 3, 1, 2).float()
    inv = torch.tensor([1.0 / s for s in STD], dtype=torch.float32).view(1, 3, 1, 1)
    return img, (top, left), (crop / 255.0 - torch.tensor(MEAN).view(1, 3, 1, 1)) * inv, w


def _reference(pix, w, P):
    """(e, y, slack_e, slack_y) in float64, [B][1 + G G][hidden]."""
    hidden = w["weight"].shape[0]
    v = F.unfold(pix.to(bf16).to(f64), P, stride=P).transpose(1, 2)                  # [B][G G][(c, i, j)]
    wk, pos = w["weight"].to(f64).reshape(hidden, -1), w["pos"].to(f64)
    cls = (w["cls"].to(f64) + pos[0]).expand(v.shape[0], 1, hidden)
    e = torch.cat([cls, v @ wk.t() + pos[1:]], 1)
    d = EPS32 * torch.cat([cls.abs(), v.abs() @ wk.abs().t() + pos[1:].abs()], 1)
    mu = e.mean(-1, keepdim=True)
    rstd = (((e - mu) ** 2).mean(-1, keepdim=True) + EPS).rsqrt()
    gamma, beta = w["gamma"].to(f64), w["beta"].to(f64)
    y = (e - mu) * rstd * gamma + beta
    dm = d.amax(-1, keepdim=True)
    slack_y = gamma.abs() * rstd * (d + dm) + (y - beta).abs() * rstd * dm + 4 * EPS32 * ((y - beta).abs() + beta.abs())
    return e, y, d, slack_y


def _launch(img, crop, w, P, S, want_emb, clean=False):
    """One launch on guarded buffers: poisoned inputs (uint8 rows 7 bytes apart from packed), strided outputs; bands checked."""
    from diffusers_amd import ops
    pick = lambda gd: gd.clean() if clean else gd  # noqa: E731
    B, hidden = img.shape[0], w["weight"].shape[0]
    rows = B * ((1 + (S // P) ** 2 + 15) // 16 * 16)
    if img.dtype == torch.uint8:
        _, Hs, Ws, _ = img.shape
        gi = pick(FP.poisoned(img.reshape(B * Hs, Ws * 3), ld=Ws * 3 + 7))
        image = gi.view.as_strided((B, Hs, Ws, 3), (Hs * gi.ld, gi.ld, 3, 1), gi.view.storage_offset())
    else:
        gi = pick(FP.poisoned(img.reshape(-1, S)))
        image = gi.view.view(img.shape)
    gw = {k: pick(FP.poisoned(ops.pack_clip_patch_weight(t) if k == "weight" else t)) for k, t in w.items()}
    gx, ge = FP.guarded((rows, hidden), ld=hidden + 8), FP.guarded((rows, hidden), ld=hidden + 16) if want_emb else None
    gx.view.fill_(float("nan"))
    if ge is not None:
        ge.view.fill_(float("nan"))
    x, emb = ops.clip_patch_embed(image, gw["weight"].view, gw["cls"].view, gw["pos"].view, gw["gamma"].view, gw["beta"].view, EPS,
                                  patch=P, size=S, crop=crop, mean=MEAN, std=STD, out=gx.view, emb_out=False if ge is None else ge.view)
    torch.cuda.synchronize()
    for gd in [gi, gx, *gw.values()] + ([ge] if ge is not None else []):
        gd.check("clip patch embed")
    return x.cpu().contiguous(), None if emb is None else emb.cpu().contiguous()


def _check(got, ref, slack, n, what):
    """Rows [0, n) of every image within 2^-8 |ref| + slack; the padding rows zeros."""
    B = ref.shape[0]
    got = got.view(B, -1, ref.shape[-1])
    err = (got[:, :n].to(f64) - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + slack
    worst = float((err / bound).nan_to_num(float("inf")).max())
    print(f"[clip patch] {what}: max_abs={float(err.nan_to_num(float('inf')).max()):.3e} worst err/bound={worst:.3f}")
    assert worst <= 1.0, what
    assert bool((got[:, n:].contiguous().view(torch.int16) == 0).all()), f"{what}: padding rows"


@pytest.mark.parametrize("mode", ["u8", "f32"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hidden,P,S", SHAPES, ids=lambda v: str(v))
def test_kernel_against_fp64(hidden, P, S, B, mode):
    img, crop, pix, w = _inputs(hidden, P, S, B, mode, seed=hidden + P + S + B)
    x, emb = _launch(img, crop, w, P, S, want_emb=B == 3)
    e, y, slack_e, slack_y = _reference(pix, w, P)
    _check(x, y, slack_y, e.shape[1], f"x_out {hidden} P{P} S{S} B{B} {mode}")
    if emb is not None:
        _check(emb, e, slack_e, e.shape[1], f"emb_out {hidden} P{P} S{S} B{B} {mode}")


@pytest.mark.parametrize("mode", ["u8", "f32"])
def test_constant_image_and_surroundings_do_not_matter(mode):
    """A constant image (every patch alike: the rows differ by the position embedding alone), and the same launch with zeros in place
    of the poison around every input: bit-identical."""
    hidden, P, S, B = 256, 14, 42, 2
    img, crop, pix, w = _inputs(hidden, P, S, B, mode, seed=5, constant=True)
    x, emb = _launch(img, crop, w, P, S, want_emb=True)
    e, y, slack_e, slack_y = _reference(pix, w, P)
    _check(x, y, slack_y, e.shape[1], f"constant {mode} x_out")
    _check(emb, e, slack_e, e.shape[1], f"constant {mode} emb_out")
    x2, emb2 = _launch(img, crop, w, P, S, want_emb=True, clean=True)
    assert FP.bits_equal(x, x2) and FP.bits_equal(emb, emb2)


REFUSALS = [(dict(hidden=192), 3), (dict(hidden=1792), 3), (dict(S=30), 3), (dict(P=33, S=66), 3), (dict(x_ld=132), 3), (dict(emb_ld=140), 3),
            (dict(x_off=2), 3), (dict(w_off=2), 3), (dict(pos_off=2), 3), (dict(top=6), 3), (dict(left=10), 3), (dict(row=3 * 37 - 1), 3),
            (dict(image=None), 1), (dict(weight=None), 1), (dict(gamma=None), 1), (dict(x_out=None), 1), (dict(mode=2), 1)]


@pytest.mark.parametrize("over,status", REFUSALS, ids=lambda v: str(v).replace(" ", ""))
def test_refusals_write_nothing(over, status):
    from diffusers_amd import _lib as L
    big = torch.zeros(1 << 20, dtype=bf16, device=DEV)                               # every operand: in bounds whatever is refused
    img = torch.zeros((1, 33, 37, 3), dtype=torch.uint8, device=DEV)
    gx, ge = FP.guarded((16, 128), ld=136), FP.guarded((16, 128), ld=136)
    a = dict(image=img.data_ptr(), mode=0, row=3 * 37, top=5, left=9, weight=big.data_ptr(), gamma=big.data_ptr(), x_out=gx.ptr(), x_ld=136,
             emb_ld=136, hidden=128, S=28, P=14, x_off=0, w_off=0, pos_off=0)
    a.update(over)
    ptr = lambda v, off=0: None if v is None else v + off  # noqa: E731
    rc = L.load().da_clip_patch_embed(a["image"], a["mode"], 33, 37, a["row"], a["top"], a["left"], *MEAN, *(1 / s for s in STD),
                                      ptr(a["weight"], a["w_off"]), big.data_ptr(), big.data_ptr() + a["pos_off"], a["gamma"],
                                      big.data_ptr(), EPS, ptr(a["x_out"], a["x_off"]), a["x_ld"], ge.ptr(), a["emb_ld"], 1, a["S"],
                                      a["P"], a["hidden"], None)
    torch.cuda.synchronize()
    assert rc == status
    for gd in (gx, ge):
        gd.check("refused launch")
        assert not bool(gd.view.any()), "a refused launch wrote into its output"


# ---- the encoder ------------------------------------------------------------------------------------------------------------------------
CONFIGS = [dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, hidden_act="quick_gelu"),
           dict(hidden_size=640, num_attention_heads=8, num_hidden_layers=2, hidden_act="gelu"),
           dict(hidden_size=1664, num_attention_heads=16, num_hidden_layers=1, hidden_act="quick_gelu")]


def _config(**kw):
    return dict(dict(image_size=56, patch_size=14, projection_dim=64, intermediate_size=2 * kw["hidden_size"]), **kw)


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"h{c['hidden_size']}-{c['hidden_act']}")
def test_encoder_against_transformers_fp64(cfg):
    import transformers
    from diffusers_amd import factory
    cfg = _config(**cfg)
    enc, sd = factory.build_clip_vision(cfg, seed=3)
    pv = torch.randn((2, 3, 56, 56), generator=torch.Generator("cpu").manual_seed(1))

    def theirs(dt):
        m = transformers.CLIPVisionModelWithProjection(transformers.CLIPVisionConfig(**cfg)).eval()
        m.load_state_dict({k: v.float() for k, v in sd.items()})
        with torch.no_grad():
            return m.to(dt)(pixel_values=pv.to(dt), output_hidden_states=True)
    ref, low, got = theirs(f64), theirs(bf16), enc(pixel_values=pv.to(DEV), output_hidden_states=True)
    assert len(got.hidden_states) == len(ref.hidden_states) and got.image_embeds.shape == (2, 64)
    for name, pick in (("image_embeds", lambda o: o.image_embeds), ("last_hidden_state", lambda o: o.last_hidden_state),
                       ("hidden_states[0]", lambda o: o.hidden_states[0]), ("hidden_states[-2]", lambda o: o.hidden_states[-2]),
                       ("hidden_states[-1]", lambda o: o.hidden_states[-1])):
        err, floor = ad.rel_rms64(pick(got).cpu(), pick(ref)), ad.rel_rms64(pick(low), pick(ref))
        print(f"[clip vision h{cfg['hidden_size']}] {name}: engine {err:.3e}, transformers bf16 (floor) {floor:.3e}")
        assert err <= ad.FLOOR_FACTOR * floor, (name, err, floor)


@pytest.fixture(scope="module")
def tiny():
    from diffusers_amd import factory
    return factory.build_clip_vision(_config(**CONFIGS[0], ), seed=3)[0]


def _pil(h, w, seed):
    from PIL import Image
    g = torch.Generator("cpu").manual_seed(seed)
    return Image.fromarray(torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).numpy())


@pytest.mark.parametrize("h,w", [(300, 200), (200, 300)])
def test_encode_image_equals_the_image_processor_route_to_the_bit(tiny, h, w):
    """Pillow-exact resize, and both modes round the same pixel to bf16 (tests/test_clip_vision_cpu.py checks that rounding for these
    two images): hidden_states[0] has the same bits."""
    from transformers.models.clip.image_processing_pil_clip import CLIPImageProcessorPil
    img = _pil(h, w, seed=h)
    pv = CLIPImageProcessorPil(size={"shortest_edge": 56}, crop_size={"height": 56, "width": 56})(images=img, return_tensors="pt").pixel_values
    a = tiny.encode_image(img, output_hidden_states=True, return_embeds=False)
    b = tiny(pixel_values=pv.to(DEV), output_hidden_states=True)
    assert FP.bits_equal(a.hidden_states[0].contiguous(), b.hidden_states[0].contiguous())
    assert FP.bits_equal(a.image_embeds, b.image_embeds)


def test_pipeline_takes_the_image_and_a_new_size_replays_the_graph(tiny):
    from diffusers_amd import factory
    pipe = factory.build_sd15_pipeline(tiny=True, ip_adapter=[4])
    g = torch.Generator("cpu").manual_seed(2)
    kw = dict(prompt_embeds=torch.randn((1, 8, 64), generator=g).to(bf16), negative_prompt_embeds=torch.randn((1, 8, 64), generator=g).to(bf16),
              height=16, width=16, num_inference_steps=3, guidance_scale=5.0, output_type="latent")
    run = lambda **k: pipe(**kw, generator=torch.Generator("cpu").manual_seed(4), **k).images.clone()  # noqa: E731
    first, second = _pil(90, 120, 1), _pil(200, 64, 2)
    with pytest.raises(NotImplementedError, match="ip_adapter_image_embeds"):
        run(ip_adapter_image=first)
    pipe.image_encoder = tiny

    def by_hand(img):
        e = tiny.encode_image(img)[None]
        return [torch.cat([torch.zeros_like(e), e])]
    got = run(ip_adapter_image=first, use_graph=True)
    captured = pipe._graph
    assert captured is not None and torch.equal(got, run(ip_adapter_image_embeds=by_hand(first), use_graph=False))
    assert torch.equal(run(ip_adapter_image=[second], use_graph=True), run(ip_adapter_image_embeds=by_hand(second), use_graph=False))
    assert pipe._graph is captured and not torch.equal(got, run(ip_adapter_image=second, use_graph=True))
