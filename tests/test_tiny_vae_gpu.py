"""AutoencoderTiny on the GPU: the 64-channel ReLU conv (csrc/conv_c64.hip through da_gemm_bf16, act = DA_ACT_RELU), the latent
input kernel, the model against the restated reference (tests/tiny_vae_emulation.py), and the pipelines that take it as ``vae``.

Accuracy gates: ``conftest.assert_close_bf16`` against fp32 torch on the same bf16 operands, and the project's floor rule
(DESIGN.md 8e): the engine's relative rms error is at most 1.5 x that of the same graph run op by op in bf16 by torch on the CPU."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import footprint as FP
import tiny_vae_emulation as TE
import value_domain as V
from conftest import assert_close_bf16, rel_rms

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
DEV = "cuda"
GRIDS = [(1, 1), (3, 5), (8, 8), (17, 33), (64, 64)]


def _rnd(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(bf16)


def _operands(B, H, W, seed, k_valid=0):
    x, r = _rnd((B, H, W, 64), seed), _rnd((B, H, W, 64), seed + 1)
    w, b = _rnd((64, 576), seed + 2, 576 ** -0.5), _rnd((64,), seed + 3, 0.25)
    if k_valid:
        x[..., k_valid:] = 0
        w.view(64, 9, 64)[..., k_valid:] = 0
    return x, w, b, r


def _relu_conv(x, w, b=None, r=None, k_valid=0, out=None):
    from diffusers_amd import _lib as L, ops
    y = ops.conv2d_nhwc(x.to(DEV), w.to(DEV), None if b is None else b.to(DEV), residual=None if r is None else r.to(DEV),
                        act=L.ACT_RELU, k_valid=k_valid, out=out)
    torch.cuda.synchronize()
    return y


def _floor(x, w, b, r):
    """The same op, op by op in bf16 by torch on the CPU: conv (+ bias) rounds, the residual add rounds, ReLU."""
    y = F.conv2d(x.permute(0, 3, 1, 2), w.view(64, 3, 3, 64).permute(0, 3, 1, 2).contiguous(), b, padding=1).permute(0, 2, 3, 1)
    if r is not None:
        y = y + r
    return F.relu(y)


def _gates(got, x, w, b, r, what):
    ref = F.relu(TE.relu_conv_ref(x, w, b, r))
    assert_close_bf16(got, ref, what)
    e, f = rel_rms(got, ref), rel_rms(_floor(x, w, b, r), ref)
    print(f"[tiny-vae] {what}: engine rel rms {e:.3e}, floor {f:.3e}")
    assert e <= 1.5 * f, f"{what}: engine {e:.3e} > 1.5 x floor {f:.3e}"


# ---- kernel 1 against fp32 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("grid", GRIDS)
def test_relu_conv_against_fp32_and_the_bf16_floor(grid, B):
    H, W = grid
    for k_valid in (0, 4, 16):
        x, w, b, r = _operands(B, H, W, 100 * H + W + k_valid, k_valid)
        for bias in (None, b):
            for res in (None, r):
                got = _relu_conv(x, w, bias, res, k_valid).cpu()
                assert got.shape == x.shape and got.dtype == bf16
                _gates(got, x, w, bias, res, f"relu conv {H}x{W} B{B} k_valid {k_valid} bias {bias is not None} residual {res is not None}")


def _relu0(t):
    """relu with the kernel's contract for zeros: torch's CPU relu returns -0 for -0 (max(-0, 0)), the kernel +0 for every non-positive
    value.  Everything else as torch computes it."""
    return torch.where(t > 0, t, torch.zeros_like(t))


def _identity_weight():
    w = torch.zeros(64, 9, 64)
    w[:, 4, :] = torch.eye(64)                       # centre tap = I
    return w.view(64, 576).to(bf16)


def test_relu_conv_to_the_bit():
    w_id = _identity_weight()
    # Gaussian data, and every finite bf16 value (tests/value_domain.py) with the same values in reverse as the residual: sums that
    # cancel, overflow to inf, stay denormal or land on -0
    dom = V.all_finite_bf16()
    cases = [(_rnd((2, 17, 33, 64), 1), _rnd((2, 17, 33, 64), 2)), (dom.view(1, 30, 34, 64), dom.flip(0).view(1, 30, 34, 64).contiguous())]
    for x, r in cases:
        got = _relu_conv(x, w_id, None, r).cpu()
        assert FP.bits_equal(got, _relu0(x + r)), "identity weight: out != relu(x + r) as torch computes it in bf16"
        assert FP.bits_equal(_relu_conv(x, w_id).cpu(), _relu0(x)), "identity weight, no residual: out != relu(x)"
        if torch.isfinite((x.float() + r.float())).all():
            _gates(got, x, w_id, None, r, "identity weight")
    # a zero weight: the bias alone, on every pixel
    x, _, b, _ = _operands(2, 9, 35, 7)
    got = _relu_conv(x, torch.zeros(64, 576, dtype=bf16), b).cpu()
    assert FP.bits_equal(got, _relu0(b).expand(2, 9, 35, 64).contiguous())
    # negative inputs: exactly +0, never -0
    neg = -_rnd((1, 5, 40, 64), 9).abs()
    neg[0, 0, :, :8] = -0.0
    got = _relu_conv(neg, w_id).cpu()
    assert int(got.view(torch.int16).abs().max()) == 0


def _params(x, w, out, bias=None, residual=None):
    from diffusers_amd import _lib as L, ops
    p = ops._conv_params(x, w, 3, None, 1, False, None, 0)
    p.A, p.W, p.C, p.bias, p.residual = x.data_ptr(), w.data_ptr(), out.data_ptr(), ops._ptr(bias), ops._ptr(residual)
    p.ldr = 64 if residual is not None else 0
    p.alpha, p.out_scale, p.act, p.tile, p.staging, p.split_k = 1.0, 1.0, L.ACT_RELU, L.TILE_AUTO, 0, 1
    return p


def test_relu_conv_refusals_launch_nothing():
    from diffusers_amd import _lib as L
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    x, w, b, r = (t.to(DEV) for t in _operands(1, 6, 7, 3))
    out = FP.guarded((1, 6, 7, 64))
    other = torch.zeros(4096, device=DEV, dtype=torch.float32)
    ok = _params(x, w, out.view, b, r)
    assert lib.da_gemm_bf16(C.byref(ok), st) == L.DA_OK                   # the struct the mutations start from is a valid launch
    torch.cuda.synchronize()
    want = _relu_conv(x, w, b, r)
    assert FP.bits_equal(out.view, want)
    out.check("valid launch")
    ptr = other.data_ptr()
    refused = [dict(conv=1), dict(conv=0), dict(stride=2), dict(up=1), dict(pad=0), dict(C1=128), dict(C2=64), dict(N=128), dict(K=1152),
               dict(tile=L.TILE_128x128), dict(tile=L.TILE_K2_128x128), dict(k_valid=65), dict(k_valid=-1), dict(out_f32=1),
               dict(rowvec=ptr, rows_per_batch=42), dict(gate=ptr, rows_per_batch=42), dict(bias_rows=ptr), dict(split_k=2),
               dict(stats_out=ptr, stats_ld=2), dict(ln_stats=ptr), dict(vt=ptr), dict(xa_k=ptr), dict(xa_vt=ptr), dict(alpha=0.5),
               dict(out_scale=2.0), dict(residual=out.view.data_ptr()), dict(Hout=5), dict(ldc=128), dict(A2=ptr)]
    out.view.fill_(float("nan"))
    before = out.snapshot()
    for mut in refused:
        p = _params(x, w, out.view, b, r)
        for k, v in mut.items():
            setattr(p, k, v)
        assert lib.da_gemm_bf16(C.byref(p), st) == 3, f"{mut}: not DA_ERR_UNSUPPORTED"
    # the other entry points that take the struct have no such epilogue either
    pa, pb = _params(x, w, out.view), _params(x, w, out.view)
    assert lib.da_gemm_pair_bf16(C.byref(pa), C.byref(pb), st) != L.DA_OK
    torch.cuda.synchronize()
    assert torch.equal(out.snapshot(), before), "a refused launch wrote to the output"


def test_relu_conv_never_touches_the_tuning_table(monkeypatch):
    from diffusers_amd import ops, tuning

    def boom(*a, **k):
        raise AssertionError("the ReLU conv consulted the tuning table")
    keys = set(tuning.table())
    monkeypatch.setattr(ops, "_select_variant", boom)
    monkeypatch.setattr(tuning, "lookup", boom)
    monkeypatch.setattr(tuning, "tune", boom)
    x, w, b, r = _operands(1, 8, 8, 5)
    _relu_conv(x, w, b, r)
    assert set(tuning.table()) == keys
    for kw in (dict(tile=1), dict(staging=1), dict(split_k=2)):
        with pytest.raises(ValueError, match="one kernel"):
            ops.conv2d_nhwc(x.to(DEV), w.to(DEV), act=7, **kw)
    xr = x.to(DEV)
    with pytest.raises(ValueError, match="in place"):
        ops.conv2d_nhwc(xr, w.to(DEV), residual=xr, out=xr, act=7)


# ---- footprint -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(3, 5), (17, 33)])
def test_relu_conv_footprint(grid):
    from diffusers_amd import _lib as L, ops
    H, W = grid
    x, w, b, r = _operands(2, H, W, 40 + H)
    px, pw, pb, pr = FP.poisoned(x), FP.poisoned(w), FP.poisoned(b), FP.poisoned(r)
    out = FP.guarded((2, H, W, 64))
    out.view.fill_(float("nan"))
    ops.conv2d_nhwc(px.view, pw.view, pb.view, residual=pr.view, act=L.ACT_RELU, out=out.view)
    torch.cuda.synchronize()
    out.check("relu conv output")
    for g, nm in ((px, "input"), (pw, "weight"), (pb, "bias"), (pr, "residual")):
        g.check(nm)
    assert torch.isfinite(out.view.float()).all(), "a halo (or operand) read reached the NaN surroundings"
    cx, cw, cb, cr = px.clean(), pw.clean(), pb.clean(), pr.clean()
    ref = ops.conv2d_nhwc(cx.view, cw.view, cb.view, residual=cr.view, act=L.ACT_RELU)
    torch.cuda.synchronize()
    assert FP.bits_equal(out.view, ref), "the surroundings of the operands changed the result"
    _gates(out.view.cpu(), x, w, b, r, f"footprint {H}x{W}")


# ---- replay ----------------------------------------------------------------------------------------------------------------------
def test_relu_conv_replays_from_a_plan_and_a_hip_graph():
    from diffusers_amd import _lib as L, ops, plan as P
    x, w, b, r = (t.to(DEV) for t in _operands(2, 17, 33, 77, k_valid=4))
    out = torch.empty_like(x)

    def run():
        ops.conv2d_nhwc(x, w, b, residual=r, act=L.ACT_RELU, k_valid=4, out=out)
        return [out]
    run()
    torch.cuda.synchronize()
    eager = out.clone()
    pl, _ = P.record(run, keep=[x, w, b, r, out])
    assert pl.foreign_ops == [] and list(pl.names) == ["da_gemm_bf16"]
    for _ in range(2):
        out.fill_(float("nan"))
        pl.launch()
        torch.cuda.synchronize()
        assert FP.bits_equal(out, eager), "plan replay differs from the eager launch"
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                        # warm launch on the side stream (sets the kernel's LDS attribute)
        s.synchronize()
        with torch.cuda.graph(g, stream=s):
            run()
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert FP.bits_equal(out, eager), "graph replay differs from the eager launch"
    # the latent input kernel has no plan number: its wrapper refuses inside a recording instead of being dropped from the plan
    z = _rnd((1, 4, 3, 5), 3).to(DEV)
    with pytest.raises(RuntimeError, match="not replayable by a launch plan"):
        P.record(lambda: [ops.tiny_vae_latents_in(z)], strict=False)


# ---- kernel 2 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lc", [4, 16])
def test_latents_in_to_the_bit(Lc):
    from diffusers_amd import _lib as L, ops
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    for (B, H, W) in ((1, 3, 5), (2, 7, 9), (1, 1, 1), (2, 32, 31)):
        z = _rnd((B, Lc, H, W), 11 * H + Lc, 4.0)
        z.view(-1)[: min(8, z.numel())] = torch.tensor([0.0, -0.0, 30.0, -30.0, 1e-3, 3.0, -3.0, 0.5], dtype=bf16)[: min(8, z.numel())]
        for div in (1.0, 0.13025):
            for add in (0.0, 0.1159):
                want = TE.tiny_vae_latents_in(z, in_div=div, in_add=add, magnitude=3.0)
                got = ops.tiny_vae_latents_in(z.to(DEV), in_div=div, in_add=add).cpu()
                assert FP.bits_equal(got, want), f"L {Lc} {H}x{W} / {div} + {add}: {int((got != want).sum())} elements differ"
                assert not got[..., Lc:].any() and int(got[..., Lc:].view(torch.int16).abs().max()) == 0
        pz, out = FP.poisoned(z), FP.guarded((B, H, W, 64))
        out.view.fill_(float("nan"))
        assert lib.da_tiny_vae_latents_in(pz.ptr(), out.ptr(), B, Lc, H, W, 0.13025, 0.1159, 3.0, st) == L.DA_OK
        torch.cuda.synchronize()
        out.check("latents_in output"), pz.check("latents")
        assert FP.bits_equal(out.view.cpu(), TE.tiny_vae_latents_in(z, in_div=0.13025, in_add=0.1159))
    z, y = _rnd((1, 4, 2, 2), 1).to(DEV), torch.full((1, 2, 2, 64), float("nan"), device=DEV, dtype=bf16)
    for args in ((None, y.data_ptr(), 1, 4, 2, 2), (z.data_ptr(), None, 1, 4, 2, 2), (z.data_ptr(), y.data_ptr(), 1, 0, 2, 2),
                 (z.data_ptr(), y.data_ptr(), 1, 17, 2, 2), (z.data_ptr(), y.data_ptr(), 0, 4, 2, 2), (z.data_ptr(), y.data_ptr(), 1, 4, 0, 2),
                 (z.data_ptr(), y.data_ptr(), 1, 4, 2, -1)):
        assert lib.da_tiny_vae_latents_in(*args, 1.0, 0.0, 3.0, st) == 1, args          # DA_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.isnan(y.float()).all()


# ---- the model -------------------------------------------------------------------------------------------------------------------
def _floor_gate(got, ref32, ref16, what):
    e, f = rel_rms(got, ref32), rel_rms(ref16, ref32)
    print(f"[tiny-vae] {what}: engine rel rms {e:.3e}, floor {f:.3e}")
    assert torch.isfinite(got.float()).all()
    assert e <= 1.5 * f, f"{what}: engine {e:.3e} > 1.5 x floor {f:.3e}"


@pytest.fixture(scope="module", params=["two-stage", "default"])
def model_case(request):
    from diffusers_amd import init as dinit
    from diffusers_amd.autoencoder_tiny import AutoencoderTiny
    cfg = dinit.TINY_TAESD if request.param == "two-stage" else dinit.TAESD
    sd = dinit.random_state_dict(dinit.tiny_vae_param_shapes(cfg), seed=11)
    f = 2 ** (len(cfg["num_decoder_blocks"]) - 1)
    g = torch.Generator().manual_seed(5)
    z = (torch.randn(2, 4, 8, 8, generator=g) * 2).to(bf16)
    img = (torch.rand(2, 3, 8 * f, 8 * f, generator=g) * 2 - 1).to(bf16)
    ref = dict(dec32=TE.ref_decode(sd, cfg, z, torch.float32, 0.13025), dec16=TE.ref_decode(sd, cfg, z, bf16, 0.13025),
               enc32=TE.ref_encode(sd, cfg, img, torch.float32), enc16=TE.ref_encode(sd, cfg, img, bf16))
    return request.param, AutoencoderTiny(**cfg).load_state_dict(sd, device=DEV), z, img, ref


def test_model_decode(model_case):
    name, vae, z, _, ref = model_case
    got = vae.decode(z.to(DEV), latents_div=0.13025).sample
    assert got.dtype == bf16 and got.shape == ref["dec32"].shape
    _floor_gate(got.cpu(), ref["dec32"], ref["dec16"], f"{name} decode")
    for mode in ("pt", "np", "uint8"):
        out = vae.decode(z.to(DEV), latents_div=0.13025, postprocess=mode).sample.cpu()
        want = TE.ref_postprocess(ref["dec32"], mode)
        assert out.shape == want.shape and out.dtype == want.dtype, mode
        if mode == "uint8":
            d = int((out.int() - want.int()).abs().max())
            print(f"[tiny-vae] {name} decode uint8: max |engine - restatement| = {d} count(s)")
            assert d <= 1
        else:
            assert float((out - TE.ref_postprocess(got.cpu(), mode)).abs().max()) <= 1e-6, mode


def test_model_encode(model_case):
    name, vae, _, img, ref = model_case
    out = vae.encode(img.to(DEV))
    assert out.latents.dtype == bf16 and out.latents.shape == ref["enc32"].shape
    _floor_gate(out.latents.cpu(), ref["enc32"], ref["enc16"], f"{name} encode")
    u8 = ((img.float() + 1) / 2 * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    lat8 = vae.encode_image(u8.to(DEV), nchw=False).latents.cpu()
    assert rel_rms(lat8, ref["enc32"]) < 0.1                      # (a byte-quantised copy of the image: same latents, roughly)


def test_model_against_the_reference_package():
    """Where the reference package ships (oracle/_ref/diffusers_ref.zip): the real AutoencoderTiny, same gate."""
    from oracle import ref_runtime as RR
    if not RR.available():
        pytest.skip("reference package not shipped")
    from diffusers_amd import init as dinit
    from diffusers_amd.autoencoder_tiny import AutoencoderTiny
    ref = RR.load_reference()
    cfg = dinit.TINY_TAESD
    sd = dinit.random_state_dict(dinit.tiny_vae_param_shapes(cfg), seed=11)
    z = _rnd((1, 4, 8, 8), 3, 2.0)
    with torch.no_grad():
        want = RR.build_model(ref, "AutoencoderTiny", cfg, sd, "cpu", torch.float32).decode(z.float()).sample
        floor = RR.build_model(ref, "AutoencoderTiny", cfg, sd, "cpu", bf16).decode(z).sample
    assert torch.allclose(want, TE.ref_decode(sd, cfg, z), atol=1e-5), "the restatement is not the reference"
    got = AutoencoderTiny(**cfg).load_state_dict(sd, device=DEV).decode(z.to(DEV)).sample.cpu()
    _floor_gate(got, want, floor, "decode vs the reference class")


# ---- pipelines -------------------------------------------------------------------------------------------------------------------
def _sdxl_embeds(seed=3):
    g = torch.Generator().manual_seed(seed)
    pe, npe = (torch.randn(1, 7, 64, generator=g).to(bf16).to(DEV) for _ in range(2))
    te, nte = (torch.randn(1, 64, generator=g).to(bf16).to(DEV) for _ in range(2))
    return dict(prompt_embeds=pe, negative_prompt_embeds=npe, pooled_prompt_embeds=te, negative_pooled_prompt_embeds=nte)


def test_sdxl_lcm_pipeline_with_the_tiny_vae():
    from diffusers_amd import factory
    from diffusers_amd.autoencoder_tiny import AutoencoderTiny
    from diffusers_amd.pipelines import decode_postprocessed
    pipe = factory.build_sdxl_pipeline(device=DEV, tiny=True, seed=0, scheduler="lcm", tiny_vae=True)
    assert isinstance(pipe.vae, AutoencoderTiny)
    lat = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(8)).to(bf16).to(DEV)

    def run(mode, output_type="pt", emb=None, **kw):
        out = pipe(latents=lat.clone(), generator=torch.Generator().manual_seed(108), num_inference_steps=2, guidance_scale=1.5,
                   height=32, width=32, use_graph=mode, output_type=output_type, **(emb or _sdxl_embeds()), **kw).images
        torch.cuda.synchronize()
        return out.clone() if torch.is_tensor(out) else out
    eager = run(False)
    assert tuple(eager.shape) == (1, 3, 32, 32) and torch.isfinite(eager).all() and float(eager.min()) >= 0 and float(eager.max()) <= 1
    for mode in (True, "plan"):
        assert torch.equal(run(mode), eager), mode
        graph = pipe._graph
        other = run(mode, emb=_sdxl_embeds(4))                               # another prompt: no recapture
        assert pipe._graph is graph and not torch.equal(other, eager), mode
        assert torch.equal(other, run(False, emb=_sdxl_embeds(4))), mode
    latents = run(True, output_type="latent")
    assert tuple(latents.shape) == (1, 4, 16, 16)
    again = decode_postprocessed(pipe.vae, latents, "pt", latents_div=float(pipe.vae.config.scaling_factor))
    assert torch.equal(again, eager), "the pipeline's image is not vae.decode of its own latents"
    assert run(True, output_type="np").shape == (1, 32, 32, 3) and run(True, output_type="pil")[0].size == (32, 32)
    # a per-step preview through callback_on_step_end decodes the running latents with the same VAE
    previews = []

    def cb(p, i, t, kw):
        previews.append(p.vae.decode(kw["latents"], return_dict=False, postprocess="uint8")[0].clone())
        return {}
    assert torch.equal(run(True, callback_on_step_end=cb, callback_on_step_end_tensor_inputs=["latents"]), eager)
    assert len(previews) == 2 and previews[0].dtype == torch.uint8 and tuple(previews[0].shape) == (1, 32, 32, 3)


def test_flux_pipeline_with_the_tiny_vae():
    from diffusers_amd import factory
    from diffusers_amd.autoencoder_tiny import AutoencoderTiny
    from diffusers_amd.pipelines import decode_postprocessed
    pipe = factory.build_flux_pipeline(device=DEV, tiny=True, seed=5, tiny_vae=True)
    assert isinstance(pipe.vae, AutoencoderTiny) and pipe.vae.config.latent_channels == 16

    def embeds(seed):
        g = torch.Generator().manual_seed(seed)
        return dict(prompt_embeds=torch.randn(1, 16, 64, generator=g).to(bf16).to(DEV),
                    pooled_prompt_embeds=torch.randn(1, 64, generator=g).to(bf16).to(DEV))

    def run(mode, output_type="pt", seed=3):
        out = pipe(height=32, width=32, num_inference_steps=2, generator=torch.Generator().manual_seed(21), max_sequence_length=16,
                   use_graph=mode, output_type=output_type, **embeds(seed)).images
        torch.cuda.synchronize()
        return out.clone()
    eager = run(False)
    assert tuple(eager.shape) == (1, 3, 32, 32) and torch.isfinite(eager).all()
    for mode in (True, "plan"):
        assert torch.equal(run(mode), eager), mode
        graph = pipe._graph
        other = run(mode, seed=4)
        assert pipe._graph is graph and torch.equal(other, run(False, seed=4)) and not torch.equal(other, eager), mode
    packed = run(True, output_type="latent")
    vc = pipe.vae.config
    unp = pipe._unpack_latents(packed, 32, 32, pipe.vae_scale_factor).contiguous()
    again = decode_postprocessed(pipe.vae, unp, "pt", latents_div=float(vc.scaling_factor), latents_add=float(vc.shift_factor))
    assert torch.equal(again, eager)
