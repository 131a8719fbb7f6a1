"""GPU: the two ends of the VAE encoder (csrc/misc.hip image loader of the four-pixel conv_in, csrc/vae_encode.hip posterior ->
latents) against torch restatements in their documented operation order, and AutoencoderKL.encode against an fp32 restatement of
Encoder.forward built from oracle.reference_math pieces, gated relative to the torch-bf16 noise floor."""
import shutil
import subprocess
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from test_isa_guards import _serialised_runs

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
DEV = torch.device("cuda", 0)
bf16 = torch.bfloat16


def rel_rms(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


def _rb(x):
    return x.to(bf16).float()


# ---- K1: image -> conv_in ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [16, 13, 33])
@pytest.mark.parametrize("form", ["f32_nchw", "f32_nhwc", "u8_nhwc"])
@pytest.mark.parametrize("normalize", [True, False])
def test_conv_in_image_equals_thin_conv_on_the_converted_image(form, W, normalize):
    from diffusers_amd import ops
    g = torch.Generator().manual_seed(3)
    B, H, Cout = 2, 24, 128
    w = (torch.randn(Cout, 3, 3, 3, generator=g) * 0.2).to(bf16)
    b = (torch.randn(Cout, generator=g) * 0.1).to(bf16)
    wp = ops.pack_conv_weight(w).to(DEV)
    if form == "u8_nhwc":
        img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
        x = img.float() / 255.0                                  # correctly rounded, as numpy's / 255.0
    else:
        x = torch.rand(B, H, W, 3, generator=g)
        img = x if form == "f32_nhwc" else x.permute(0, 3, 1, 2).contiguous()
    if normalize:
        x = 2.0 * x - 1.0
    pre = x.to(bf16).permute(0, 3, 1, 2).contiguous()            # NCHW bf16: what the reference's encoder receives
    y = ops.vae_conv_in_image(img.to(DEV), wp, b.to(DEV), nchw=form == "f32_nchw", normalize=normalize)
    want = ops.conv_thin_in(pre.to(DEV), wp, b.to(DEV), ksize=3, in_nchw=True)
    torch.cuda.synchronize()
    assert torch.equal(y, want)
    ref = F.conv2d(pre.float(), w.float(), b.float(), padding=1).permute(0, 2, 3, 1)
    assert (y.float().cpu() - ref).abs().max() <= 1e-2 * ref.abs().max()


# ---- K2: conv_out result -> latents ----------------------------------------------------------------------------------------
def _k2_ref(raw, wq, bq, eps1, eps2, mode, scale, shift, a, b):
    """Restatement of csrc/vae_encode.hip's documented order: raw [B][2L][HW] bf16 -> [B][L or 2L][HW]."""
    x = raw.float()
    if wq is not None:
        acc = bq.float()[None, :, None].expand(x.shape[0], -1, x.shape[2]).clone()
        for k in range(x.shape[1]):
            acc = acc + wq[:, k].float()[None, :, None] * x[:, k:k + 1]   # the product of two bf16 values is exact in fp32
        p = _rb(acc)
    else:
        p = x
    if mode == "moments":
        return p.to(bf16)
    Lc = p.shape[1] // 2
    z = p[:, :Lc]
    if mode == "sample":
        lv = p[:, Lc:].clamp(-30.0, 20.0)
        std = torch.exp(_rb(0.5 * lv).to(bf16)).float()              # torch.exp of a bf16 tensor
        z = _rb(z + _rb(std * eps1.float()))
    if shift is not None:
        z = _rb(z - shift)
    if scale is not None:
        z = _rb(z * scale)
    if eps2 is not None:
        z = _rb(_rb(a * z) + _rb(b * eps2.float()))
    return z.to(bf16)


def _ulps(a, b):
    a, b = a.float(), b.float()
    m = torch.maximum(a.abs(), b.abs()).clamp_min(1e-30)
    return float(((a - b).abs() / (m * 2.0 ** -7)).max())


# MOMENTS writes the posterior parameters: latent scaling, the shift and add_noise apply to latents only
_K2_CASES = [("moments", False, None)] + [(m, n, sh) for m in ("mean", "sample") for n in (False, True) for sh in (None, 0.1159)]


@pytest.mark.parametrize("layout", ["nchw", "nhwc16"])
@pytest.mark.parametrize("quant", [True, False])
@pytest.mark.parametrize("mode,noise,shift", _K2_CASES)
def test_posterior_latents_matches_restatement(layout, mode, quant, noise, shift):
    from diffusers_amd import _lib as L, ops
    g = torch.Generator().manual_seed(7)
    B, H, W, Lc = 2, 9, 13, 4
    HW = H * W
    raw = torch.randn(B, 2 * Lc, HW, generator=g) * 3
    raw[:, Lc:] = torch.linspace(-45, 35, B * Lc * HW).reshape(B, Lc, HW)[:, torch.randperm(Lc, generator=g)]   # both clamp sides
    raw = raw.to(bf16)
    wq = (torch.randn(2 * Lc, 2 * Lc, generator=g) * 0.5).to(bf16) if quant else None
    bq = (torch.randn(2 * Lc, generator=g) * 0.1).to(bf16) if quant else None
    eps1 = torch.randn(B, Lc, HW, generator=g).to(bf16) if mode == "sample" else None
    eps2 = torch.randn(B, Lc, HW, generator=g).to(bf16) if noise else None
    scale, a, b = (0.13025, 0.6914, 0.7227) if mode != "moments" else (None, 1.0, 0.0)
    if layout == "nchw":
        src, strides = raw.contiguous(), (2 * Lc * HW, HW, 1)
    else:
        src = torch.zeros(B, HW, 16, dtype=bf16)
        src[:, :, :2 * Lc] = raw.transpose(1, 2)
        strides = (HW * 16, 1, 16)
    m = {"moments": L.POSTERIOR_MOMENTS, "mean": L.POSTERIOR_MEAN, "sample": L.POSTERIOR_SAMPLE}[mode]
    dv = lambda t: None if t is None else t.to(DEV).contiguous()     # noqa: E731
    y = ops.vae_posterior_latents(dv(src), strides, batch=B, hw=HW, latent_channels=Lc, mode=m, wq=dv(wq), bq=dv(bq),
                                  eps1=dv(eps1), eps2=dv(eps2), scale=scale, shift=shift, a=a, b=b)
    want = _k2_ref(raw.to(DEV), dv(wq), dv(bq), dv(eps1), dv(eps2), mode, scale, shift, a, b)
    torch.cuda.synchronize()
    if mode == "sample":
        # std = exp(...) is the one step whose fp32 value comes from a library function: the kernel's expf and torch's may differ in
        # the last fp32 bit, which moves a bf16 rounding in rare ties -- at most one bf16 ulp
        assert _ulps(y, want) <= 1.0
        assert (y != want).float().mean() < 0.01
    else:
        assert torch.equal(y, want)


def test_add_noise_only_mode():
    from diffusers_amd import ops
    g = torch.Generator().manual_seed(9)
    x = torch.randn(3, 4, 8, 8, generator=g).to(bf16).to(DEV)
    n = torch.randn(3, 4, 8, 8, generator=g).to(bf16).to(DEV)
    # (the schedulers hand over coefficients already rounded to bf16, as the reference's bf16 tensors hold them)
    for a, b in ((1.0, 14.625), (0.69140625, 0.72265625)):
        y = ops.add_noise(x, n, a, b)
        ta, tb = torch.tensor(a, dtype=bf16, device=DEV), torch.tensor(b, dtype=bf16, device=DEV)
        assert torch.equal(y, ta * x + tb * n)                    # the reference's bf16 torch expression


def test_posterior_kernels_keep_their_loads_in_flight(tmp_path):
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)
    if hipcc is None:
        pytest.skip("hipcc not available")
    for unit in ("vae_encode", "misc"):
        out = tmp_path / f"{unit}.s"
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=on", f"-I{ROOT / 'include'}",
                            f"-I{ROOT / 'diffusers_amd' / 'csrc'}", "-S", "--cuda-device-only",
                            str(ROOT / "diffusers_amd" / "csrc" / f"{unit}.hip"), "-o", str(out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-400:]
        runs = _serialised_runs(out.read_text())
        if unit == "vae_encode":
            # (a kernel without any load-then-wait pair is not in `runs` at all: check that the kernels were compiled, then the runs)
            text = out.read_text()
            assert "posterior_latents_kernel" in text and "add_noise_kernel" in text
            assert all(v < 3 for v in runs.values()), runs
        else:   # the image-source conv_in variants: no more than the bf16 kernel's unaligned-bias fallback
            img = {k: v for k, v in runs.items() if "conv_thin_in4_kernel" in k and ("ILi3ELi1E" in k or "ILi3ELi2E" in k)}
            assert len(img) == 2 and max(img.values()) <= 9, img


# ---- AutoencoderKL.encode vs an fp32 restatement of Encoder.forward -------------------------------------------------------
def encoder_ref(sd, cfg, x):
    """Encoder.forward (vae.py:140-184) + quant_conv from oracle.reference_math pieces: the posterior parameters."""
    from oracle import reference_math as R
    groups, eps = cfg["norm_num_groups"], 1e-6
    boc = tuple(cfg["block_out_channels"])
    h = F.conv2d(x, sd["encoder.conv_in.weight"], sd["encoder.conv_in.bias"], padding=1)
    for i in range(len(boc)):
        for j in range(cfg["layers_per_block"]):
            h = R.resnet_block(sd, f"encoder.down_blocks.{i}.resnets.{j}", h, None, groups, eps)
        if i != len(boc) - 1:
            p = f"encoder.down_blocks.{i}.downsamplers.0.conv"
            h = F.conv2d(F.pad(h, (0, 1, 0, 1)), sd[f"{p}.weight"], sd[f"{p}.bias"], stride=2)
    h = R.resnet_block(sd, "encoder.mid_block.resnets.0", h, None, groups, eps)
    if cfg["mid_block_add_attention"]:
        h = R.vae_attention(sd, "encoder.mid_block.attentions.0", h, groups, eps)
    h = R.resnet_block(sd, "encoder.mid_block.resnets.1", h, None, groups, eps)
    h = F.silu(F.group_norm(h, groups, sd["encoder.conv_norm_out.weight"], sd["encoder.conv_norm_out.bias"], eps))
    h = F.conv2d(h, sd["encoder.conv_out.weight"], sd["encoder.conv_out.bias"], padding=1)
    if cfg["use_quant_conv"]:
        h = F.conv2d(h, sd["quant_conv.weight"], sd["quant_conv.bias"])
    return h


def _encode_case(cfg_name, hw, gemm_path, seed=1):
    from diffusers_amd import factory, init as dinit
    cfg = getattr(dinit, cfg_name)
    vae, sd = factory.build_vae(cfg, seed=seed, device=DEV, init_device=str(DEV), with_encoder=True)
    if vae.encoder.mid_attn is not None:
        vae.encoder.mid_attn.force_gemm_path = gemm_path
    full = dict(vae.config)
    g = torch.Generator().manual_seed(5)
    img = (torch.rand(1, 3, hw, hw, generator=g) * 2 - 1).to(bf16)
    dist = vae.encode(img.to(DEV)).latent_dist
    got = dist.parameters
    with torch.no_grad():
        ref = encoder_ref({k: v.float() for k, v in sd.items()}, full, img.float().to(DEV))
        floor = encoder_ref(sd, full, img.to(DEV))
    rr, rf = rel_rms(got, ref), rel_rms(floor, ref)
    print(f"{cfg_name} encode {hw}^2 (gemm_path={gemm_path}): engine vs fp32 rel_rms {rr:.3e}, torch-bf16 floor {rf:.3e}")
    assert got.shape == ref.shape and torch.isfinite(got.float()).all()
    assert rr <= 1.5 * rf + 2e-3, (rr, rf)
    return vae, dist


@pytest.mark.parametrize("gemm_path", [False, True])
def test_tiny_vae_encode_vs_fp32_encoder(gemm_path):
    _encode_case("TINY_VAE", 64, gemm_path)


def test_sdxl_vae_encode_1024_vs_fp32_encoder():
    """The SDXL-width encoder at 1024 x 1024: mid-block attention over S = 16 384 tokens on the D = 512 GEMM path, conv_out on the
    implicit-GEMM route (the posterior kernel reads its channel-padded NHWC output)."""
    _encode_case("SDXL_VAE", 1024, True)


def test_latent_dist_sample_equals_mean_plus_std_randn():
    from diffusers_amd import factory, init as dinit
    vae, _ = factory.build_vae(dinit.TINY_VAE, seed=1, device=DEV, with_encoder=True)
    img = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(2)).to(DEV) * 2 - 1
    dist = vae.encode(img).latent_dist
    g = torch.Generator().manual_seed(11)
    g2 = g.clone_state() if hasattr(g, "clone_state") else torch.Generator().manual_seed(11)
    z = dist.sample(generator=g)
    eps = torch.randn(dist.mean.shape, generator=g2, dtype=torch.float32).to(DEV).to(bf16)   # force_upcast: drawn in fp32
    want = dist.mean + dist.std * eps
    assert _ulps(z, want) <= 1.0 and (z != want).float().mean() < 0.01
    assert torch.equal(dist.mode(), dist.mean)
    assert torch.equal(dist.logvar, dist.parameters[:, 4:].clamp(-30, 20))
