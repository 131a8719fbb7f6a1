"""CPU leg of the attention value-domain tests: the conditions tests/test_attention_domain_gpu.py asserts on the flash kernels are
conditions a plain fp32 restatement of their arithmetic (attention_domain.flash_model_f32) and the torch stand-in of
tests/ops_emulation.py meet against fp64 on every family, the generators produce what they claim, and a deliberately wrong model
is caught by the families that are there to catch it."""
import pytest
import torch

import attention_domain as ad
import ops_emulation as E

bf16 = torch.bfloat16
IDS = [ad.family_id(f) for f in ad.FAMILIES]


def _cases(kind, level, Ds=(64, 128)):
    for D in Ds:
        for Skv in ad.SKVS:
            yield D, Skv, ad.case(kind, level, D, Skv)


@pytest.mark.parametrize("kind,level", ad.FAMILIES, ids=IDS)
def test_fp32_model_meets_every_condition(kind, level):
    """Online softmax (first generation), the deferred maximum (algo 0 / 2) and the row sum of the rounded P (algo 4): the
    element-wise bound of the suite against fp64 with no element exempted; the AUG forms (algo 3 / 5) meet their 3e-2 bound once the
    first tile leaves the zero accumulators alone."""
    fails = []
    for D, Skv, c in _cases(kind, level):
        for variant in ("v1", 2, 4, 3, 5):
            what = f"fp32 model {variant} {ad.family_id((kind, level))} D{D} Skv{Skv}"
            out = c.model(variant)
            fails += ad.check(out, c.ref, None, what, ad.tol_of(variant))
            if kind == "onehot":
                fails += ad.check_onehot(out, c.v, ad.SQ, what)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("kind,level", ad.FAMILIES, ids=IDS)
def test_attention_stand_in_meets_every_condition(kind, level):
    """tests/ops_emulation.py attention (fp32 softmax, bf16 output) against fp64, and inside 1.5 x the plain model's rel-rms."""
    fails = []
    for D, Skv, c in _cases(kind, level, Ds=(64, 96, 128, 160)):
        q, kp, vt, kw = ad.operands(c.q, c.k, c.v)
        out = E.attention(q, kp, vt, H=c.H, D=D, scale=c.scale, **kw)
        what = f"stand-in attention {ad.family_id((kind, level))} D{D} Skv{Skv}"
        fails += ad.check(out, c.ref, c.model_rr("v1"), what, ad.TOL_DEFAULT)
        if kind == "onehot":
            fails += ad.check_onehot(out, c.v, ad.SQ, what)
    assert not fails, "\n".join(fails)


def test_aug_first_tile_rescale_is_what_breaks_low_offsets():
    """The AUG form as attention2.hip had it -- alpha = exp2(-shift) applied to the still-zero accumulators of the first tile -- is
    0 * inf once every score of a wave's first tile lies more than 128 log2-units below zero: offsets of -300 and below, the negative
    rows of `rowmix`, the low first tile of `late_low_to_high`.  Above that the two forms agree bit for bit."""
    for kind, level in ad.FAMILIES:
        c = ad.case(kind, level, 64, 333)
        old, new = c.model(3, first_tile_rescale=True), c.model(3)
        breaks = (kind == "offset" and level <= -300) or kind in ("rowmix", "late_low_to_high")
        nan_rows = torch.isnan(old.float()).any(-1)
        assert bool(nan_rows.any()) == breaks, (kind, level)
        assert bool(torch.isfinite(new.float()).all())
        assert torch.equal(old[~nan_rows], new[~nan_rows]), (kind, level)


@pytest.mark.parametrize("name", ad.MASKED_FAMILIES)
def test_masked_model_and_stand_in_meet_every_condition(name):
    fails = []
    for dtype, shared in ad.masked_variants(name):
        c = ad.masked_case(name, dtype, shared)
        what = f"{name} bias={dtype} shared_row={shared}"
        fails += ad.check(c.model(), c.ref, None, f"fp32 model, masked {what}", ad.TOL_DEFAULT, ad.REL_RMS_MASKED)
        q, kp, vt, kw = ad.operands(c.q, c.k, c.v)
        out = E.attention(q, kp, vt, H=c.H, D=ad.MASKED_D, scale=c.scale, causal=c.causal, bias=c.bias, **kw)
        fails += ad.check(out, c.ref, c.model_rr(), f"stand-in, masked {what}", ad.TOL_DEFAULT, ad.REL_RMS_MASKED)
        if name == "dead_row":       # the contract: a query without a visible key gives a row of zeros, in all three
            for o in (c.ref, c.model(), out.view(1, ad.MASKED_S, -1)):
                assert not o[0, ad.DEAD_ROW].any() and bool(o[0, ad.DEAD_ROW + 1].any())
    assert not fails, "\n".join(fails)


def test_masked_families_mask_what_they_claim():
    S = ad.MASKED_S
    dead = lambda n, sh=False: (ad.masked_case(n, bf16, sh).bias[..., :S].float() <= -1e29)    # noqa: E731
    for sh in (False, True):
        assert bool(dead("left_padding", sh)[..., :70].all()) and not dead("left_padding", sh)[..., 70:].any()     # the whole first tile
        assert bool(dead("middle_tile", sh)[..., 64:128].all()) and int(dead("middle_tile", sh)[0, 0, 0].sum()) == 64
        assert torch.equal(dead("interleaved", sh)[0, 0, 0], torch.arange(S) % 2 == 1)
        for sign in (1, -1):
            b = ad.masked_case("bias_offset+1e4" if sign > 0 else "bias_offset-1e4", torch.float32, sh).bias[..., :S]
            assert float((b - sign * 1e4).abs().max()) < 5.0
    d = dead("dead_row")
    assert bool(d[0, :, ad.DEAD_ROW].all()) and int(d.all(-1).sum()) == ad.H_
    assert ad.masked_case("left_padding", bf16, True).bias.shape == (1, 1, 1, 192)
    assert ad.masked_case("causal", None, False).causal and ad.masked_case("causal_bias", bf16, False).causal


def test_generators_produce_what_they_claim():
    D, Skv = 64, 333
    for lv in ad.OFFSET_LEVELS:
        c = ad.case("offset", lv, D, Skv)
        sc = ad.scores64(c.q, c.k, c.H, c.scale)
        assert abs(float(sc.mean()) - lv) < abs(lv) * 2.0 ** -8 + 0.2 and float((sc - sc.mean()).abs().max()) < 8.0
    for lv in ad.ROWMIX_LEVELS:
        c = ad.case("rowmix", lv, D, Skv)
        row = ad.scores64(c.q, c.k, c.H, c.scale).mean(-1)[0, 0]
        assert bool((row[0::2] > 0.99 * lv).all()) and bool((row[1::2] < -0.99 * lv).all())      # both signs inside every wave
    for st in ad.RAMP_STEPS:
        for skv in ad.SKVS:
            mx = ad.log2_tile_maxima(ad.case("ramp", st, D, skv))
            d = mx[..., 1:] - mx[..., :-1]
            # (k's column 0 is rounded to bf16: up to 2^-9 of the level reached, six steps at the most; + the score noise)
            assert float((d - st).abs().max()) < 0.25 + 6 * abs(st) * 2.0 ** -8, (st, float((d - st).abs().max()))
            # 7.5: a tile never outgrows the previous one by the threshold (two do); 8.5 and 40: every tile does
            assert bool((d.abs() < ad.DEFER_LOG2).all()) == (abs(st) == 7.5) and bool((d.abs() > ad.DEFER_LOG2).all()) == (abs(st) != 7.5)
            if skv == 333:
                assert bool(((mx[..., 2] - mx[..., 0]).abs() > ad.DEFER_LOG2).all())
    for kind, sign in (("late_low_to_high", 1.0), ("late_high_to_low", -1.0)):
        mx = ad.log2_tile_maxima(ad.case(kind, 300.0, D, Skv)) * sign / ad.LOG2E
        assert bool((mx[..., 0] < -290).all()) and bool((mx[..., -1] > 290).all()) and bool((mx[..., 1:-1].abs() < 10).all())
    for Dh in (64, 128):
        for skv in ad.SKVS:
            c = ad.case("onehot", 0.0, Dh, skv)
            pi = ad.onehot_pi(ad.SQ, skv)
            assert set((pi % 64).tolist()) == set(range(64)) and set(range(skv // 64 * 64, skv)) <= set(pi.tolist()) and int(pi.max()) < skv
            sc = ad.scores64(c.q, c.k, c.H, c.scale) * ad.LOG2E
            top = sc.topk(2, dim=-1)
            assert torch.equal(top.indices[..., 0], pi.expand(1, c.H, ad.SQ)) and float((top.values[..., 0] - top.values[..., 1]).min()) >= 200.0
            assert torch.equal(c.ref.to(bf16), c.v[:, pi])                      # the expected output: the selected rows of V
    for kind in ("uniform_keys", "uniform_q0"):
        c = ad.case(kind, 0.0, D, Skv)
        mean = ad.heads(c.v, c.H).double().mean(2, keepdim=True).expand(-1, -1, ad.SQ, -1).permute(0, 2, 1, 3).reshape(c.ref.shape)
        assert float((c.ref - mean).abs().max()) < 1e-12
    assert float(ad.case("vscale", 100.0, D, Skv).v.float().abs().max()) > 2.0 ** 100
    c = ad.case("voutlier", 1e4, D, Skv)
    w = torch.softmax(ad.scores64(c.q, c.k, c.H, c.scale), -1)[..., Skv // 2]
    assert float(c.v[:, Skv // 2].float().abs().max()) > 1e4 and 1e-4 < float(w.mean()) < 3e-2     # a key of ordinary weight


@pytest.mark.parametrize("kind,level", [f for f in ad.FAMILIES if (f[0] == "ramp" and f[1] > 0) or f[0] == "late_low_to_high"],
                         ids=lambda x: str(x))
def test_negative_control_a_rescale_that_forgets_l_is_caught(kind, level):
    """A deferred-maximum kernel whose rescale reaches O but not l fails the element-wise bound on the rising `ramp`s and on
    `late_low_to_high` (and meets it on N(0, 1) data, where the shift settles in the first tile)."""
    c = ad.case(kind, level, 64, 333)
    bad = c.model(2, forget_alpha_on_l=True)
    assert ad.check(bad, c.ref, c.model_rr(2), f"negative control {kind} {level:+g}", ad.TOL_DEFAULT)
    assert not ad.check(c.model(2), c.ref, c.model_rr(2), f"the right model {kind} {level:+g}", ad.TOL_DEFAULT)


def test_split_shape_model_meets_the_conditions():
    """The key-split case of the GPU file (16 key tiles, 40 heads) on the plain and deferred models."""
    B, H, D, Sq, Skv = ad.SPLIT_SHAPE
    kind, level = ad.SPLIT_FAMILIES[2]
    c = ad.case(kind, level, D, Skv, B, H, Sq)
    fails = []
    for variant in (2, 3):
        fails += ad.check(c.model(variant), c.ref, None, f"fp32 model {variant} {kind} split shape", ad.tol_of(variant))
    assert not fails, "\n".join(fails)
