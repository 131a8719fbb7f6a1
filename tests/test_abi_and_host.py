"""CPU: the C-ABI library builds/loads and exports every symbol include/diffusers_amd.h declares; host-side logic of the
product (schedule tables, parameter inventories, weight packing, argument validation) -- no kernel is launched."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


def _header_functions():
    src = (ROOT / "include" / "diffusers_amd.h").read_text()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(da_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from diffusers_amd import _lib as L
    from diffusers_amd.build import build_extension
    build_extension()
    lib = L.load()
    declared = _header_functions()
    assert "da_gemm_bf16" in declared and "da_attention_bf16" in declared
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/diffusers_amd.h but not exported"
    assert sorted(L.SIGNATURES) == declared, "ctypes signature table and header disagree"
    assert lib.da_version() == L.ABI_VERSION and lib.da_sizeof_gemm_params() == C.sizeof(L.GemmParams)


def test_struct_layout_matches_header_field_order():
    from diffusers_amd import _lib as L
    src = (ROOT / "include" / "diffusers_amd.h").read_text()
    for cname, cls in (("da_gemm_params", L.GemmParams), ("da_attention_params", L.AttentionParams)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            parts = decl.replace("*", " ").split(",")
            first = parts[0].split()
            names.append(first[-1])
            names += [p.strip() for p in parts[1:]]
        assert names == [f[0] for f in cls._fields_], cname


def test_ops_refuse_cpu_tensors():
    from diffusers_amd import ops
    x = torch.zeros((64, 64), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.linear(x, x)


def test_scheduler_tables_match_reference(golden):
    """Host-side schedule construction of the product schedulers vs tables produced by the reference classes."""
    from diffusers_amd import schedulers as S
    gz = golden("schedulers")
    e = S.EulerDiscreteScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1,
                                 timestep_spacing="leading")
    e.set_timesteps(50, device="cpu")
    assert np.array_equal(e.timesteps.numpy(), gz["euler50_timesteps"])
    assert np.array_equal(e.sigmas.numpy(), gz["euler50_sigmas"])
    assert float(e.init_noise_sigma) == float(gz["euler50_init_sigma"])
    tab = e.device_table.numpy()
    assert tab.shape == (50, 8)
    assert np.array_equal(tab[:, 0], gz["euler50_sigmas"][:-1]) and np.array_equal(tab[:, 1], gz["euler50_sigmas"][1:])
    assert np.array_equal(tab[:, 7], gz["euler50_timesteps"])
    d = S.DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
                        set_alpha_to_one=False, steps_offset=1)
    d.set_timesteps(50, device="cpu")
    assert np.array_equal(d.timesteps.numpy(), gz["ddim50_timesteps"])
    f = S.FlowMatchEulerDiscreteScheduler(shift=1.0)
    f.set_timesteps(sigmas=np.linspace(1.0, 1 / 4, 4), device="cpu")
    assert np.array_equal(f.timesteps.numpy(), gz["flow4_timesteps"])
    assert np.array_equal(f.sigmas.numpy(), gz["flow4_sigmas"])
    fd = S.FlowMatchEulerDiscreteScheduler(shift=3.0, use_dynamic_shifting=True)
    fd.set_timesteps(sigmas=np.linspace(1.0, 1 / 28, 28), mu=1.15, device="cpu")
    assert np.array_equal(fd.sigmas.numpy(), gz["flowdyn28_sigmas"])
    with pytest.raises(ValueError, match="mu"):
        fd.set_timesteps(num_inference_steps=4, device="cpu")
    p = S.DDPMScheduler()
    p.set_timesteps(5, device="cpu")
    assert p.timesteps.tolist() == [800, 600, 400, 200, 0]
    d2 = S.DDIMScheduler(steps_offset=1)
    d2.set_timesteps(5, device="cpu")
    assert d2.timesteps.tolist() == [801, 601, 401, 201, 1]  # reference tests/schedulers/test_scheduler_ddim.py:46-54


def test_scheduler_error_behaviour():
    from diffusers_amd import schedulers as S
    e = S.EulerDiscreteScheduler()
    with pytest.raises(ValueError, match="exactly one"):
        e.set_timesteps(None)
    e.set_timesteps(4, device="cpu")
    with pytest.raises(ValueError, match="integer indices"):
        e.step(torch.zeros(1), 0, torch.zeros(1))
    with pytest.raises(TypeError):
        S.EulerDiscreteScheduler(bogus=1)
    with pytest.raises(NotImplementedError):
        S.EulerDiscreteScheduler(use_beta_sigmas=True)


def test_param_inventory_counts():
    """Parameter counts of the canonical configs (859.52 M, 2567.46 M, decoder 49.49 M)."""
    from diffusers_amd import init as dinit
    from diffusers_amd.autoencoder_kl import _DEFAULTS as VD
    from diffusers_amd.unet_2d_condition import _DEFAULTS as UD

    def count(shapes):
        return sum(int(np.prod(s)) for s in shapes.values())

    sdxl = dict(UD)
    sdxl.update(dinit.SDXL_UNET)
    sd15 = dict(UD)
    sd15.update(dinit.SD15_UNET)
    vae = dict(VD)
    vae.update(dinit.SDXL_VAE)
    assert abs(count(dinit.unet_param_shapes(sdxl)) / 1e6 - 2567.46) < 0.01
    assert abs(count(dinit.unet_param_shapes(sd15)) / 1e6 - 859.52) < 0.01
    assert abs(count(dinit.vae_decoder_param_shapes(vae)) / 1e6 - 49.49) < 0.01


def test_weight_packing_roundtrip():
    from diffusers_amd import ops
    w = torch.arange(2 * 3 * 3 * 3, dtype=torch.float32).reshape(2, 3, 3, 3)
    p = ops.pack_conv_weight(w)
    assert p.shape == (2, 27)
    assert p[1, (2 * 3 + 1) * 3 + 2] == w[1, 2, 2, 1]  # K index = (kh*3+kw)*Cin + c
    wg = torch.arange(256 * 4, dtype=torch.float32).reshape(256, 4)
    bg = torch.arange(256, dtype=torch.float32)
    wp, bp = ops.pack_geglu(wg, bg)
    # group 1 (rows 64..127 of the packed matrix) = value rows 32..63 then gate rows 128+32..128+63
    assert torch.equal(bp[64:96], bg[32:64]) and torch.equal(bp[96:128], bg[160:192])
    assert torch.equal(wp[96], wg[160])


def test_model_config_validation():
    from diffusers_amd.autoencoder_kl import AutoencoderKL
    from diffusers_amd.unet_2d_condition import UNet2DConditionModel
    with pytest.raises(ValueError, match="does not exist"):
        UNet2DConditionModel(down_block_types=("Bogus",) * 4)
    with pytest.raises(ValueError, match="same number"):
        UNet2DConditionModel(block_out_channels=(64, 128))
    with pytest.raises(TypeError):
        UNet2DConditionModel(not_a_key=1)
    m = UNet2DConditionModel()
    assert m.config.cross_attention_dim == 1280 and m.config["norm_num_groups"] == 32
    with pytest.raises(RuntimeError, match="load_state_dict"):
        m.forward(torch.zeros(1), 1, torch.zeros(1))
    with pytest.raises(NotImplementedError):
        AutoencoderKL().encode(None)


def test_flux_host_logic():
    """Host-side pieces of the Flux path: latent packing, the dynamic-shift formula, RoPE tables, config validation."""
    from diffusers_amd import init as dinit
    from diffusers_amd.pipelines import FluxPipeline, calculate_shift
    from diffusers_amd.transformer_flux import FluxTransformer2DModel, rope_tables
    from oracle import reference_math as R
    x = torch.arange(2 * 16 * 8 * 6, dtype=torch.float32).view(2, 16, 8, 6)
    packed = FluxPipeline._pack_latents(x, 2, 16, 8, 6)
    assert packed.shape == (2, 12, 64)
    assert torch.equal(FluxPipeline._unpack_latents(packed, 8 * 8, 6 * 8, 8), x)
    assert abs(calculate_shift(4096) - 1.15) < 1e-9 and abs(calculate_shift(256) - 0.5) < 1e-9
    ids = torch.cat([torch.zeros(16, 3), FluxPipeline._prepare_latent_image_ids(8, 8)], 0)
    c1, s1 = rope_tables(ids, (8, 28, 28))
    c2, s2 = R.rope_tables(ids, (8, 28, 28))
    assert torch.equal(c1, c2) and torch.equal(s1, s2) and c1.shape == (80, 64) and c1.dtype == torch.float32
    assert FluxTransformer2DModel(**dinit.FLUX_SCHNELL).inner_dim == 3072
    with pytest.raises(ValueError):
        FluxTransformer2DModel(guidance_embeds=True)
    with pytest.raises(ValueError):
        FluxTransformer2DModel(attention_head_dim=96, axes_dims_rope=(16, 40, 40))
    with pytest.raises(TypeError):
        FluxTransformer2DModel(not_a_key=1)
    n = sum(int(np.prod(s)) for s in dinit.flux_param_shapes(dinit.FLUX_SCHNELL).values())
    assert n == 11_891_178_560


def test_flowmatch_model_timestep_column():
    from diffusers_amd import schedulers as S
    sch = S.FlowMatchEulerDiscreteScheduler(shift=1.0)
    with pytest.raises(ValueError):
        sch.set_model_timesteps([1.0])


def test_head_dim_padding_is_exact():
    """Zero-padding heads to a kernel size must not change q.k or the to_out product (SD1.5: 40 -> 64, 80 -> 96)."""
    from diffusers_amd.layers import kernel_head_dim, pad_head_cols, pad_head_rows
    assert [kernel_head_dim(d) for d in (8, 40, 64, 80, 96, 128, 160)] == [64, 64, 64, 96, 96, 128, 160]
    with pytest.raises(ValueError):
        kernel_head_dim(192)
    g = torch.Generator().manual_seed(0)
    heads, d, dp, C = 8, 40, 64, 48
    wq, wk, wv = (torch.randn((heads * d, C), generator=g) for _ in range(3))
    wo = torch.randn((C, heads * d), generator=g)
    x = torch.randn((5, C), generator=g)

    def attn(wq_, wk_, wv_, wo_, dd):
        q, k, v = (x @ w_.t() for w_ in (wq_, wk_, wv_))
        q, k, v = (t_.view(5, heads, dd).transpose(0, 1) for t_ in (q, k, v))
        p = torch.softmax(q @ k.transpose(1, 2) * d ** -0.5, -1)
        return (p @ v).transpose(0, 1).reshape(5, heads * dd) @ wo_.t()
    a = attn(wq, wk, wv, wo, d)
    b = attn(pad_head_rows(wq, heads, d, dp), pad_head_rows(wk, heads, d, dp), pad_head_rows(wv, heads, d, dp),
             pad_head_cols(wo, heads, d, dp), dp)
    assert torch.allclose(a, b, atol=1e-5)


def test_attention_backend_registers_with_reference_registry():
    """Boundary B4: the backend function has the argument names the reference's dispatcher filters on and takes over a
    registry slot.  Needs the reference sources (build container only); skipped where they are absent."""
    import importlib
    import inspect
    import sys
    from oracle import build_ref
    ref_src = build_ref.SRC.parent
    if not build_ref.reference_present():
        pytest.skip("reference sources not present")
    sys.path.insert(0, str(ref_src))
    try:
        ad = importlib.import_module("diffusers.models.attention_dispatch")
    finally:
        sys.path.remove(str(ref_src))
    from diffusers_amd.attention_backend import mi355x_flash_attention, register_backend
    ref_params = list(inspect.signature(ad._native_attention).parameters)
    ours = list(inspect.signature(mi355x_flash_attention).parameters)
    assert ours[:3] == ref_params[:3] == ["query", "key", "value"]
    assert set(ref_params) <= set(ours), set(ref_params) - set(ours)
    saved = {k: dict(getattr(ad._AttentionBackendRegistry, k)) for k in ("_backends", "_constraints", "_supported_arg_names")}
    try:
        name = register_backend()
        assert ad._AttentionBackendRegistry._backends[name] is mi355x_flash_attention
    finally:
        for k, v in saved.items():
            getattr(ad._AttentionBackendRegistry, k).clear()
            getattr(ad._AttentionBackendRegistry, k).update(v)


def test_unipc_coefficient_table_reproduces_reference(golden, monkeypatch):
    """Host half of the UniPC step: the per-step coefficient rows, applied in the kernel's operation order (emulated here
    with fp32 torch ops), reproduce the reference's fp32 trajectory bit for bit."""
    from diffusers_amd import schedulers as S
    g = golden("unipc")

    def fake_upload(self, rows, device):
        self._table, self._step_dev = torch.from_numpy(rows), torch.zeros((), dtype=torch.int32)
    monkeypatch.setattr(S._SchedulerBase, "_upload", fake_upload)
    sch = S.UniPCMultistepScheduler(prediction_type="flow_prediction", use_flow_sigmas=True, flow_shift=3.0)
    n = len(g["timesteps"])
    sch.set_timesteps(n, device="cpu")
    assert np.array_equal(sch.timesteps.numpy(), g["timesteps"]) and np.array_equal(sch.sigmas.numpy(), g["sigmas"])
    coef = sch._coef.numpy()
    assert [int(r[9]) for r in coef] == [1] + [2] * (n - 2) + [1]          # warm-up and lower_order_final
    f = lambda a: torch.tensor(a, dtype=torch.float32)  # noqa: E731
    x = torch.from_numpy(g["x0"]).clone()
    last, m1, m2 = (torch.zeros_like(x) for _ in range(3))
    for i in range(n):
        r, v = coef[i], torch.from_numpy(g["v"][i])
        mn = x - f(r[0]) * v
        xc = x
        if r[1] != 0:
            inner = f(r[8]) * (mn - m1)
            if int(r[2]) == 2:
                inner = f(r[7]) * ((m2 - m1) / f(r[6])) + inner
            xc = (f(r[3]) * last - f(r[4]) * m1) - f(r[5]) * inner
        xn = f(r[10]) * xc - f(r[11]) * mn
        if int(r[9]) == 2:
            xn = xn - f(r[12]) * (0.5 * ((m1 - mn) / f(r[13])))
        m2, m1, last, x = m1, mn, xc, xn
        assert torch.equal(x, torch.from_numpy(g["traj_f32"][i])), f"step {i}"
    with pytest.raises(NotImplementedError):
        S.UniPCMultistepScheduler()  # epsilon / VP-sigma configuration is not on the hot path


def test_wan_vae_host_logic_vs_reference(golden, monkeypatch):
    """AutoencoderKLWan's host half (zero padding to 64 channels, one launch per temporal tap accumulating in place over
    frame-shifted views, the "Rep" first frame of the temporal upsamplers, folded V bias / latent de-normalisation) on
    torch-CPU stand-ins of the kernels (tests/ops_emulation.py): bf16 activations vs the reference's fp32 decode."""
    from diffusers_amd import init as dinit, ops
    from diffusers_amd.autoencoder_kl_wan import AutoencoderKLWan
    import ops_emulation
    g = golden("tiny_wan_vae")
    cfg = dinit.TINY_WAN_VAE
    sd = dinit.random_state_dict(dinit.wan_vae_decoder_param_shapes(cfg), seed=21)
    vae = AutoencoderKLWan(**cfg).load_state_dict(sd, device="cpu", strict=True)
    with pytest.raises(ValueError):
        vae.decode(torch.zeros((1, 16, 2, 4, 4)))            # CPU tensor: there is no fallback
    ops_emulation.install(monkeypatch, ops)
    want = torch.from_numpy(g["video"])
    for z, dn in ((g["z"], False), (g["latents"], True)):
        video = vae._decode_one(torch.from_numpy(z)[0].to(torch.bfloat16), dn, True)
        assert tuple(video.shape) == tuple(want.shape)
        rel = float((video - want).pow(2).mean().sqrt() / want.pow(2).mean().sqrt())
        print(f"[host] tiny Wan VAE (denormalize={dn}): rel rms vs reference fp32 = {rel:.3e}")
        assert rel < 2.5e-2
    with pytest.raises(NotImplementedError):
        AutoencoderKLWan(is_residual=True)


def test_cpp_abi_example_compiles_and_links(tmp_path):
    """examples/abi_demo.cpp drives the C ABI from plain C++ (hipMalloc'd memory, no Python, no torch types): it must
    compile against include/diffusers_amd.h and link against the built library.  Running it needs an MI355X."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    from diffusers_amd import build as B
    lib = B.build_extension()
    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "abi_demo"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", f"-I{root / 'include'}", str(root / "examples" / "abi_demo.cpp"),
                        f"-L{lib.parent}", "-ldiffusers_amd", f"-Wl,-rpath,{lib.parent}", "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert exe.exists()


def test_euler_karras_and_exponential_sigma_tables(golden, monkeypatch):
    """`use_karras_sigmas` / `use_exponential_sigmas` only change the host tables (sigma ladder + fractional timesteps)
    the step kernels read: bit-equal to the reference's (tests/golden/euler_karras.npz, oracle/make_golden_euler_karras.py)."""
    from diffusers_amd import schedulers as S
    sys_path_cases = {
        "karras": dict(use_karras_sigmas=True),
        "exponential": dict(use_exponential_sigmas=True),
        "karras_minmax_trailing": dict(use_karras_sigmas=True, sigma_min=0.05, sigma_max=10.0, timestep_spacing="trailing"),
        "karras_sigma_min_last": dict(use_karras_sigmas=True, final_sigmas_type="sigma_min"),
    }

    def fake_upload(self, rows, device):
        self._table, self._step_dev = torch.from_numpy(rows), torch.zeros((), dtype=torch.int32)
    monkeypatch.setattr(S._SchedulerBase, "_upload", fake_upload)
    g = golden("euler_karras")
    base = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1, timestep_spacing="leading")
    for name, extra in sys_path_cases.items():
        for n in (4, 25, 50):
            sch = S.EulerDiscreteScheduler(**dict(base, **extra))
            sch.set_timesteps(n, device="cpu")
            assert np.array_equal(sch.sigmas.numpy(), g[f"{name}_{n}_sigmas"]), (name, n)
            assert np.array_equal(sch.timesteps.numpy(), g[f"{name}_{n}_timesteps"]), (name, n)
            assert np.float32(float(sch.init_noise_sigma)) == g[f"{name}_{n}_init_noise_sigma"]
            t = sch._table.view(-1, 8)
            assert torch.equal(t[:, 0], sch.sigmas[:-1]) and torch.equal(t[:, 1], sch.sigmas[1:])
            assert torch.equal(t[:, 7], sch.timesteps.float())
    with pytest.raises(ValueError):
        S.EulerDiscreteScheduler(use_karras_sigmas=True, use_exponential_sigmas=True)
    with pytest.raises(NotImplementedError):
        S.EulerDiscreteScheduler(use_beta_sigmas=True)


def test_scheduler_from_config_round_trip_and_reference_config():
    """`Scheduler.from_config(other.config)` -- the idiom for swapping schedulers -- incl. a reference-style config that
    carries private keys and options of another scheduler class."""
    from diffusers_amd import schedulers as S
    a = S.EulerDiscreteScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1,
                                 timestep_spacing="leading")
    b = S.EulerDiscreteScheduler.from_config(a.config)
    assert dict(b.config) == dict(a.config)
    ref_like = dict(a.config, _class_name="EulerDiscreteScheduler", _diffusers_version="0.36.0", clip_sample=False,
                    set_alpha_to_one=False, skip_prk_steps=True)
    d = S.DDIMScheduler.from_config(ref_like)
    assert d.config.beta_schedule == "scaled_linear" and d.config.clip_sample is False and d.config.steps_offset == 1
    assert S.EulerDiscreteScheduler.from_config(ref_like, use_karras_sigmas=True).config.use_karras_sigmas is True
    assert S.EulerDiscreteScheduler.from_config(dict(ref_like, prediction_type="v_prediction"))._pred == 1
    with pytest.raises(ValueError):
        S.EulerDiscreteScheduler.from_config(dict(ref_like, prediction_type="flow_prediction"))
    with pytest.raises(NotImplementedError):
        S.EulerDiscreteScheduler.from_config(dict(ref_like, rescale_betas_zero_snr=True))


def test_euler_custom_timesteps_and_sigmas_tables(golden, monkeypatch):
    """`set_timesteps(timesteps=...)` / `set_timesteps(sigmas=...)` (scheduling_euler_discrete.py:378-407: custom schedules such as the
    "align your steps" ladders): sigma ladder, model timesteps and init_noise_sigma bit-equal to the reference's
    (tests/golden/euler_custom.npz, oracle/make_golden_euler_custom.py), the device table rows follow them, and the reference's
    argument checks are kept."""
    from diffusers_amd import schedulers as S

    def fake_upload(self, rows, device):
        self._table, self._step_dev = torch.from_numpy(rows), torch.zeros((), dtype=torch.int32)
    monkeypatch.setattr(S._SchedulerBase, "_upload", fake_upload)
    g = golden("euler_custom")
    base = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1, timestep_spacing="leading")
    TS = {"ays_sdxl": [999, 845, 730, 587, 443, 310, 193, 116, 53, 13], "three": [901, 501, 101]}
    SG = {"ays_sdxl": [14.615, 6.315, 3.771, 2.181, 1.342, 0.862, 0.555, 0.380, 0.234, 0.113, 0.0], "short": [10.0, 2.5, 0.7, 0.0]}

    def check(sch, key):
        assert np.array_equal(sch.sigmas.numpy(), g[key + "_sigmas"]), key
        assert np.array_equal(sch.timesteps.numpy(), g[key + "_timesteps"]), key
        assert np.float32(float(sch.init_noise_sigma)) == g[key + "_init_noise_sigma"], key
        t = sch._table.view(-1, 8)
        assert sch.num_inference_steps == t.shape[0] == len(sch.timesteps)
        assert torch.equal(t[:, 0], sch.sigmas[:-1]) and torch.equal(t[:, 1], sch.sigmas[1:]) and torch.equal(t[:, 7], sch.timesteps.float())
    for name, ts in TS.items():
        for spacing in ("leading", "trailing"):
            sch = S.EulerDiscreteScheduler(**dict(base, timestep_spacing=spacing))
            sch.set_timesteps(timesteps=ts, device="cpu")
            check(sch, f"timesteps_{name}_{spacing}")
    for name, sg in SG.items():
        sch = S.EulerDiscreteScheduler(**base)
        sch.set_timesteps(sigmas=sg, device="cpu")
        check(sch, f"sigmas_{name}")
    sch = S.EulerDiscreteScheduler(**base)
    with pytest.raises(ValueError, match="exactly one"):
        sch.set_timesteps(device="cpu")
    with pytest.raises(ValueError, match="Can only pass one"):
        sch.set_timesteps(10, device="cpu", timesteps=[1.0])
    with pytest.raises(ValueError, match="use_karras_sigmas"):
        S.EulerDiscreteScheduler(**dict(base, use_karras_sigmas=True)).set_timesteps(timesteps=[10.0], device="cpu")
    # the SDXL pipeline's `denoising_end` keeps the steps at or above the cut-off timestep (pipeline_stable_diffusion_xl.py:1164-1183)
    from diffusers_amd.pipelines import denoising_end_steps
    for n in (50, 30):
        sch = S.EulerDiscreteScheduler(**base)
        sch.set_timesteps(n, device="cpu")
        for frac in (0.8, 0.5, 0.25):
            assert denoising_end_steps(sch, frac) == int(g[f"denoising_end_{n}_{frac}"]), (n, frac)
    assert denoising_end_steps(sch, None) == 30 and denoising_end_steps(sch, 1.0) == 30


def test_tuning_keys_bucket_giant_row_counts_only():
    """Variant-table keys: exact shapes up to 2^20 rows (every entry of the shipped table), top-three-bit buckets above --
    the 81 / 80 / 79-frame temporal taps of one video conv share an entry, SDXL's 1024^2-pixel convs keep theirs."""
    import json
    from diffusers_amd import _lib as L, tuning
    assert tuning._m_key(1 << 20) == 1 << 20 and tuning._m_key(2048) == 2048
    taps = {tuning._m_key(t * 480 * 832) for t in (81, 80, 79)}
    assert len(taps) == 1 and next(iter(taps)) <= 79 * 480 * 832
    p = L.GemmParams()
    p.M, p.N, p.K, p.conv, p.act, p.out_f32 = 81 * 480 * 832, 128, 1152, 0, 0, 0
    k81 = tuning.key_of(p)
    p.M = 79 * 480 * 832
    assert tuning.key_of(p) == k81
    import re
    table = json.loads((Path(tuning.__file__).parent / "tuned" / "gfx950.json").read_text())
    assert table["arch"] == "gfx950" and len(table["entries"]) >= 250
    sdxl = set(json.loads((Path(__file__).parent / "golden" / "sdxl_gemm_shape_keys.json").read_text())["keys"])
    for key, (tile, staging, us, *split) in table["entries"].items():
        assert 1 <= tile < len(L.TILE_NAMES) and 0 <= staging <= 7 and us > 0, key
        # a split-K factor (fourth field, 2 .. DA_SPLITK_MAX): first kernel family only, and never on an SDXL shape (the headline path keeps one
        # summation order; the split variants serve the small-M, deep-K convs of the SD1.5 / DDPM U-Nets)
        assert split == [] or (len(split) == 1 and 2 <= split[0] <= L.SPLITK_MAX and tile < L.FIRST_K2_TILE and key not in sdxl), key
        # the eight-phase tile (csrc/gemm3.hip): nn.Linear only, one ring form, unsplit
        if tile in (L.TILE_K3_256x256, L.TILE_K3_256x320):
            assert key.startswith("lin:") and staging == L.STAGE_LDS_DIRECT and split == [], key
        if tile == L.TILE_K3_256x320:   # the GEGLU projection's tile: GEGLU epilogue, whole tiles (what tile_ok admits)
            m, n, act = (int(re.search(p, key).group(1)) for p in (r":M(\d+)", r":N(\d+)", r":a(\d+)"))
            assert act in (L.ACT_GEGLU, L.ACT_GEGLU_TANH) and m % 256 == 0 and n % 320 == 0, key
    n_k3 = sum(1 for v in table["entries"].values() if v[0] == L.TILE_K3_256x256)
    assert n_k3 >= 20, "the round-5 retune moved the large Flux / Wan / VAE nn.Linear entries to k3:256x256"
    header = (Path(__file__).parent.parent / "include" / "diffusers_amd.h").read_text()
    import re
    assert int(re.search(r"#define DA_TILE_COUNT (\d+)", header).group(1)) == len(L.TILE_NAMES)
    assert int(re.search(r"#define DA_TILE_K3_256x256 (\d+)", header).group(1)) == L.TILE_K3_256x256
    assert int(re.search(r"#define DA_TILE_K3_256x320 (\d+)", header).group(1)) == L.TILE_K3_256x320


def test_eight_phase_tiles_refuse_before_any_launch():
    """DA_TILE_K3_256x256 / DA_TILE_K3_256x320 (csrc/gemm3.hip): what the tiles do not implement is refused by name in the host part of
    da_gemm_bf16 (tile_ok / dispatch) -- no launch is attempted, so this runs without a GPU.  nn.Linear only, one ring form, unsplit;
    the 256 x 320 tile: GEGLU epilogue, whole tiles, 16-byte aligned output rows."""
    import ctypes as C
    from diffusers_amd import _lib as L
    lib = L.load()
    buf = (C.c_char * 4096)()
    addr = C.addressof(buf)

    def params(**kw):
        p = L.GemmParams()
        p.A = p.W = p.C = addr
        p.M, p.N, p.K, p.lda, p.ldw, p.ldc = 256, 640, 128, 128, 128, 320
        p.act, p.tile, p.staging = L.ACT_GEGLU, L.TILE_K3_256x320, L.STAGE_LDS_DIRECT
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    UNSUP = 3
    assert L.ERRORS[UNSUP] == "DA_ERR_UNSUPPORTED"
    for kw in (dict(act=L.ACT_NONE), dict(M=300), dict(N=768), dict(ldc=324), dict(C=addr + 8), dict(split_k=2),
               dict(staging=L.STAGE_LDS_DIRECT3), dict(staging=L.STAGE_PINGPONG),
               dict(tile=L.TILE_K3_256x256, split_k=2), dict(tile=L.TILE_K3_256x256, staging=L.STAGE_PINGPONG),
               dict(tile=L.TILE_K3_256x256, stats_out=addr, stats_ld=64, act=L.ACT_NONE),
               dict(tile=L.TILE_K3_256x256, vt=addr, vt_col0=320, ld_vt=256, act=L.ACT_NONE)):
        assert lib.da_gemm_bf16(C.byref(params(**kw)), None) == UNSUP, kw


def test_torch_library_ops_are_registered_with_fake_kernels():
    """torch.ops.mi355x.* (diffusers_amd/torch_ops.py): the reference's binding pattern for native kernels
    (attention_dispatch.py:746-816, custom_op + register_fake).  On a host without a GPU the REAL kernels are unreachable
    (device_types="cuda"), but the fake kernels -- what torch.compile / torch.export trace with -- must give the right
    shapes and dtypes for every op."""
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    import diffusers_amd.torch_ops as T
    ns = torch.ops.mi355x
    assert all(hasattr(ns, n) for n in T.OPS)
    bf16 = torch.bfloat16
    with FakeTensorMode():
        e = lambda *s, dt=bf16: torch.empty(s, dtype=dt, device="cuda")  # noqa: E731
        assert ns.gemm(e(2048, 1280), e(1280, 1280), e(1280), 0).shape == (2048, 1280)
        assert ns.gemm(e(2048, 1280), e(10240, 1280), None, 1).shape == (2048, 5120)          # GEGLU halves N
        assert ns.conv2d_nhwc(e(2, 64, 64, 320), e(640, 2880), e(640), 3, 2, False).shape == (2, 32, 32, 640)
        assert ns.conv2d_nhwc(e(2, 64, 64, 320), e(640, 2880), None, 3, 1, True).shape == (2, 128, 128, 640)
        assert ns.flash_attn(e(2, 4096, 10, 64), e(2, 4096, 10, 64), e(2, 4096, 10, 64), None).shape == (2, 4096, 10, 64)
        y = ns.groupnorm(e(2, 32, 32, 1280), e(1280), e(1280), 32, 1e-5, True)
        assert y.shape == (2, 32, 32, 1280) and y.dtype == bf16
        assert ns.layernorm(e(2048, 1280), e(1280), e(1280), 1e-5).shape == (2048, 1280)
        x = e(1, 4, 128, 128)
        assert ns.euler_step(e(2, 4, 128, 128), x, e(50, 8, dt=torch.float32), e(dt=torch.int32), True, 5.0, 0).shape == x.shape
    # schema: functional ops (nothing mutated), so functionalisation / export need no special handling
    for n in T.OPS:
        assert not getattr(ns, n).default._schema.is_mutable


def test_conv_chunk_query_is_host_only_and_reads_the_knob_per_call(monkeypatch):
    """da_conv_chunk_channels (ops.conv_chunk_channels): the K order a K2 / K1 conv launch walks, from the same launch geometry as the
    launch (gemm2_shared.cuh launch_geom / conv_chunk_slices) -- no GPU needed.  Auto: tap-major (0) unless a tap sweep outgrows the
    L2; the shipped table's deep-K entries are chunked on their own tiles with the chunks below; DA_CONV_CHUNK is read on every call."""
    import json
    from diffusers_amd import _lib as L
    from diffusers_amd import ops
    from diffusers_amd.build import build_extension
    build_extension()
    monkeypatch.delenv("DA_CONV_CHUNK", raising=False)
    conv_tiles = [t for t in range(L.FIRST_K2_TILE, L.TILE_K3_256x256)
                  if t not in (L.TILE_K2_80x128, L.TILE_K1_256x256, L.TILE_K1_256x320)]

    def meta(*s):
        return torch.empty(s, device="meta", dtype=torch.bfloat16)

    def q(B, H, W, C1, C2, Co, tile, ks=3, **kw):
        x2 = meta(B, H, W, C2) if C2 else None
        return ops.conv_chunk_channels(meta(B, H, W, C1), meta(Co, ks * ks * (C1 + C2)), tile, ksize=ks, x2=x2, **kw)

    # tap-major: 1 x 1 convs and the shallow shapes of test_k2_conv_variants, on every tile
    for s in ((2, 32, 32, 1280, 0, 1280), (2, 16, 16, 640, 320, 640), (2, 24, 24, 320, 0, 320), (1, 20, 20, 64, 0, 96),
              (1, 16, 16, 320, 0, 320, 3, dict(stride=2)), (1, 12, 12, 256, 0, 128, 3, dict(up=True)),
              (1, 9, 7, 128, 192, 80), (2, 16, 16, 640, 0, 1280, 1), (1, 16, 16, 64, 64, 128, 1), (2, 128, 128, 960, 0, 320, 1)):
        shape, ks, kw = s[:6], (s[6] if len(s) > 6 else 3), (s[7] if len(s) > 7 else {})
        for t in conv_tiles:
            assert q(*shape, t, ks=ks, **kw) == 0, (s, L.TILE_NAMES[t])
    # the shipped table's chunked entries, on the table's own tile
    entries = json.loads((ROOT / "diffusers_amd" / "tuned" / "gfx950.json").read_text())["entries"]
    for key, shape, want in (("conv3:M32768:N320:C640+0:H128x128:s1:u0:a0:r0", (2, 128, 128, 640, 0, 320), 256),
                             ("conv3:M32768:N320:C960+0:H128x128:s1:u0:a0:r0", (2, 128, 128, 960, 0, 320), 256),
                             ("conv3:M8192:N640:C1920+0:H64x64:s1:u0:a0:r0", (2, 64, 64, 1920, 0, 640), 1024),
                             ("conv3:M65536:N256:C512+0:H256x256:s1:u0:a0:r0", (1, 256, 256, 512, 0, 256), 256),
                             ("conv3:M262144:N256:C512+0:H512x512:s1:u0:a0:r0", (1, 512, 512, 512, 0, 256), 256)):
        tile = entries[key][0]
        got = q(*shape, tile)
        assert got == want and got % 64 == 0 and 256 <= got < shape[3] + shape[4], (key, L.TILE_NAMES[tile], got)
    # the chunk is a function of the tile: one deep-K shape, three chunks (test_gemm_k2_gpu.py invariant (2) holds per chunk size)
    deep = (2, 128, 128, 320, 320, 320)
    assert [q(*deep, t) for t in (L.TILE_K1_128x320, L.TILE_K1_256x128, L.TILE_K1_128x256)] == [256, 320, 0]
    # DA_CONV_CHUNK between two calls of one process
    for v, want in (("0", 0), ("128", 128), ("192", 192), ("100", 64), ("1024", 0), ("auto", 256), (None, 256)):
        if v is None:
            monkeypatch.delenv("DA_CONV_CHUNK")
        else:
            monkeypatch.setenv("DA_CONV_CHUNK", v)
        assert q(2, 128, 128, 640, 0, 320, L.TILE_K1_256x160) == want, v
        assert q(2, 128, 128, 640, 0, 320, L.TILE_K1_256x160, ks=1) == 0, v
    # refused: tiles outside the family or without a conv build, params that are not a conv
    for t in (L.TILE_128x128, L.TILE_K2_80x128, L.TILE_K3_256x256, 0, 99):
        with pytest.raises(RuntimeError, match="DA_ERR_UNSUPPORTED"):
            q(2, 64, 64, 640, 0, 320, t)
    lib = L.load()
    p = L.GemmParams()
    assert lib.da_conv_chunk_channels(C.byref(p), L.TILE_K2_128x128) == -1   # conv = 0: -DA_ERR_INVALID
    p.M, p.N, p.K, p.conv, p.C1, p.Hin, p.Win, p.Hout, p.Wout, p.stride = 64, 64, 9 * 96, 3, 96, 8, 8, 8, 8, 1
    assert lib.da_conv_chunk_channels(C.byref(p), L.TILE_K2_128x128) == -3   # C1 not a multiple of 64
