"""IP-Adapter Plus without a GPU: the checkpoint's key mapping into ip_adapter.Resampler (the weights only move to a device there)
and the binding facts of the one new entry point."""
import torch


def test_key_mapping_and_heads():
    from diffusers_amd import factory, init as dinit, ip_adapter as I
    sd = factory.build_ip_adapter_state_dict(dinit.TINY_SD15_UNET, plus=True, num_tokens=8, image_embed_dim=96, dim=128, depth=3)["image_proj"]
    r = I.Resampler(sd, 64, "cpu")
    inner = 128
    assert (r.heads, r.inner, r.num_tokens, r.dim, r.embed_dim, r.depth) == (inner // 64, inner, 8, 128, 96, 3)
    assert torch.equal(r.latents, sd["latents"][0]) and torch.equal(r.proj_in[0], sd["proj_in.weight"])
    assert torch.equal(r.proj_out[1], sd["proj_out.bias"]) and torch.equal(r.norm_out[0], sd["norm_out.weight"])
    for i, ly in enumerate(r.layers):
        g = lambda n: sd[f"layers.{i}.{n}"]  # noqa: E731
        assert torch.equal(ly["ln0"][0], g("0.norm1.weight")) and torch.equal(ly["ln0"][1], g("0.norm1.bias")), "norm1 is the image side"
        assert torch.equal(ly["ln1"][0], g("0.norm2.weight")) and torch.equal(ly["ln1"][1], g("0.norm2.bias")), "norm2 is the latents"
        assert torch.equal(ly["qkv"][:inner], g("0.to_q.weight"))
        assert torch.equal(ly["qkv"][inner:2 * inner], g("0.to_kv.weight")[:inner]), "to_kv: the K rows first"
        assert torch.equal(ly["qkv"][2 * inner:], g("0.to_kv.weight")[inner:]) and torch.equal(ly["kv"], g("0.to_kv.weight"))
        assert torch.equal(ly["out"], g("0.to_out.weight")) and torch.equal(ly["ff_ln"][0], g("1.0.weight"))
        assert torch.equal(ly["up"], g("1.1.weight")) and torch.equal(ly["down"], g("1.3.weight"))
    # the default keeps the base checkpoint bit for bit
    base = factory.build_ip_adapter_state_dict(dinit.TINY_SD15_UNET, image_embed_dim=64)
    assert sorted(base["image_proj"]) == ["norm.bias", "norm.weight", "proj.bias", "proj.weight"] and not I.is_resampler(base["image_proj"])


def test_lib_facts():
    from diffusers_amd import _lib as L
    name = "da_attention_resampler_bf16"
    assert list(L.PASS_THROUGH)[-1] == name and "refuses under a recording" in L.PASS_THROUGH[name]
    assert name in L.SIGNATURES and name not in L.FN_IDS and name not in L.NOT_PLANNABLE and L.ABI_VERSION == 9
