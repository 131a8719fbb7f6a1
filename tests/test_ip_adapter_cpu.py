"""IP-Adapter, host side: how a cross-attention layer packs to_k_ip | to_v_ip, and where the new entry point sits in the tables."""
import pytest
import torch

bf16 = torch.bfloat16


def _layer(heads, d, cross=24):
    from diffusers_amd import init as dinit
    from diffusers_amd.layers import Attention, Weights
    Cc = heads * d
    sd = dinit.random_state_dict({"a.to_q.weight": (Cc, Cc), "a.to_k.weight": (Cc, cross), "a.to_v.weight": (Cc, cross),
                                  "a.to_out.0.weight": (Cc, Cc), "a.to_out.0.bias": (Cc,)}, seed=1)
    return Attention(Weights(sd, "cpu"), "a", heads, cross=True)


@pytest.mark.parametrize("heads,d,dp", [(2, 40, 64), (2, 64, 64), (1, 80, 96), (1, 160, 160)])
def test_attach_ip_stacks_k_over_v_with_zero_rows_after_each_head(heads, d, dp):
    attn = _layer(heads, d)
    g = torch.Generator("cpu").manual_seed(d)
    pairs = [tuple(torch.randn((heads * d, 24), generator=g).to(bf16) for _ in "kv") for _ in range(2)]
    attn.attach_ip(pairs)
    assert attn.ip_scales == (1.0, 1.0) and len(attn.ip_w) == 2
    for w, (wk, wv) in zip(attn.ip_w, pairs):
        assert w.shape == (2 * heads * dp, 24) and w.is_contiguous()
        halves = w.view(2, heads, dp, 24)
        assert torch.equal(halves[0, :, :d], wk.view(heads, d, 24)) and torch.equal(halves[1, :, :d], wv.view(heads, d, 24))
        assert not bool(halves[:, :, d:].any()), "padded head rows are zero: zero k / v channels"
    attn.attach_ip(None)
    assert attn.ip_w is None and attn.ip_scales == ()
    with pytest.raises(ValueError, match="to_k_ip / to_v_ip must be"):
        attn.attach_ip([(pairs[0][0][:, :16], pairs[0][1][:, :16])])


def test_the_wrapper_refuses_under_a_plan_recording():
    from diffusers_amd import _lib as L, ops, plan as P
    L._tls.recorder = P.Recorder()
    try:
        with pytest.raises(RuntimeError, match="not replayable by a launch plan"):
            ops.ip_attention_accumulate(None, None, [], B=1, H=1, D=64, Sq=1)
    finally:
        L._tls.recorder = None


@pytest.mark.parametrize("cfg,count", [("SD15_UNET", 16), ("SDXL_UNET", 70)])
def test_checkpoint_keys_number_the_cross_attentions_down_up_mid(cfg, count, tmp_path):
    """loaders/unet.py walks attn_processors (down, up, mid), two per transformer block: cross-attention i has key 2 i + 1, the mid
    block's come last (SD 1.5: 1 .. 29 then 31 at 1280 channels).  A flat safetensors file reads back as the two-level dict."""
    from safetensors.torch import save_file
    from diffusers_amd import init as dinit, ip_adapter as I
    config = getattr(dinit, cfg)
    widths = I.cross_attention_widths(config)
    assert len(widths) == count and widths[-1] == 1280
    if cfg == "SD15_UNET":
        assert widths == [320] * 2 + [640] * 2 + [1280] * 2 + [1280] * 3 + [640] * 3 + [320] * 3 + [1280]
    shapes = I.ip_adapter_param_shapes(config, num_tokens=4, image_embed_dim=1024)
    cross = config["cross_attention_dim"]
    assert shapes["image_proj.proj.weight"] == (4 * cross, 1024) and len(shapes) == 4 + 2 * count
    assert all(shapes[f"ip_adapter.{2 * i + 1}.to_{c}_ip.weight"] == (w, cross) for i, w in enumerate(widths) for c in "kv")
    flat = {k: torch.full((2, 2), float(i)).to(bf16) for i, k in enumerate(list(shapes)[:6])}
    save_file(flat, str(tmp_path / "ip.safetensors"))
    for got in (I.read_ip_adapter(tmp_path / "ip.safetensors"), I.read_ip_adapter(tmp_path, None, "ip.safetensors")):
        assert set(got) == {"image_proj", "ip_adapter"} and set(got["image_proj"]) == {"proj.weight", "proj.bias", "norm.weight", "norm.bias"}
        assert all(torch.equal(got[k.split(".", 1)[0]][k.split(".", 1)[1]], v) for k, v in flat.items())
    with pytest.raises(OSError, match="not a local .safetensors file"):
        I.read_ip_adapter(tmp_path / "ip.bin")
