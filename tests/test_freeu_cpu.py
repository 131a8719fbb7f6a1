"""FreeU without a GPU: the four-bin identity da_freeu_nhwc_bf16 rests on, the ABI facts of the entry, and the enable / disable switches
of the U-Net and the pipelines with their effect on the graph key."""
import math
import re
from pathlib import Path

import pytest
import torch

import freeu_reference as FR
from diffusers_amd import _lib as L, factory, ops, pipelines as P

HEADER = (Path(__file__).resolve().parent.parent / "include" / "diffusers_amd.h").read_text()
SHAPES = [(2, 2), (3, 5), (8, 8), (16, 24), (33, 32), (47, 47), (48, 48), (64, 64)]


def seven_sums(x: torch.Tensor, s: float) -> torch.Tensor:
    """The header's formula, float64, on [B][H][W][C]."""
    x = x.double()
    _, H, W, _ = x.shape
    th = (2 * math.pi * torch.arange(H, dtype=torch.float64) / H).view(1, H, 1, 1)
    pw = (2 * math.pi * torch.arange(W, dtype=torch.float64) / W).view(1, 1, W, 1)
    sm = lambda t: (x * t).sum(dim=(1, 2), keepdim=True)  # noqa: E731
    low = (sm(torch.ones(())) + sm(th.cos()) * th.cos() + sm(th.sin()) * th.sin() + sm(pw.cos()) * pw.cos() + sm(pw.sin()) * pw.sin()
           + sm((th + pw).cos()) * (th + pw).cos() + sm((th + pw).sin()) * (th + pw).sin())
    return x + (s - 1) / (H * W) * low


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("s", [0.2, 0.9])
def test_the_filter_is_a_projection_on_four_bins(hw, s):
    x = FR.data(2, *hw, 8, seed=hw[0] * 100 + hw[1])
    assert float((seven_sums(x, s) - FR.fourier_filter(x, s)).abs().max()) <= 1e-12


def test_abi_facts_of_the_entry():
    name = "da_freeu_nhwc_bf16"
    assert re.search(r"^int da_freeu_nhwc_bf16\(void\* hidden, const void\* skip, void\* skip_out, const void\* twiddles, "
                     r"void\* workspace,\s+long long workspace_bytes, int B, int H, int W, int Cx, int Cs, float b, float s, int path, "
                     r"void\* stream\);", HEADER, re.M)
    _i, _ll, _vp, _f = L._i, L._ll, L._vp, L._f
    assert L.SIGNATURES[name] == (_i, [_vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _f, _f, _i, _vp])
    assert name in L.PASS_THROUGH and name not in L.FN_IDS and name not in L.NOT_PLANNABLE
    assert "ops.freeu refuses under a recording" in L.PASS_THROUGH[name]
    assert re.search(r"^#define DA_ABI_VERSION 9\b", HEADER, re.M) and L.ABI_VERSION == 9 and L.FN_COUNT == 36


def test_wrapper_refuses_a_recording_and_degenerate_planes(monkeypatch):
    z = torch.zeros(1, 1, 4, 16, dtype=torch.bfloat16)
    monkeypatch.setattr(ops, "_req", lambda *a, **k: None)
    with pytest.raises(ValueError, match="1 x 4 plane"):
        ops.freeu(z, z, s=0.9, b=1.3)
    monkeypatch.setattr(L._tls, "recorder", object(), raising=False)
    with pytest.raises(RuntimeError, match="not replayable by a launch plan"):
        ops.freeu(z, z, s=0.9, b=1.3)


def test_switches_and_graph_key():
    pipe = factory.build_sd15_pipeline(device="cpu", tiny=True, seed=0)
    unet = pipe.unet
    off = P._model_token(unet)
    assert off == P._weights_token(unet) and unet._freeu_stage(0) is None
    pipe.enable_freeu(s1=0.9, s2=0.2, b1=1.3, b2=1.4)
    assert unet._freeu_stage(0) == (0.9, 1.3) and unet._freeu_stage(1) == (0.2, 1.4) and unet._freeu_stage(2) is None
    on = P._model_token(unet)
    assert on != off and on[0] == off
    pipe.enable_freeu(s1=0.9, s2=0.3, b1=1.3, b2=1.4)
    assert P._model_token(unet) not in (on, off)
    pipe.enable_freeu(s1=0.9, s2=0.0, b1=1.3, b2=1.4)             # a falsy value: the reference's is_freeu_enabled is off
    assert unet._freeu_stage(0) is None and P._model_token(unet) == off
    pipe.enable_freeu(1, 1, 1, 1)
    assert unet._freeu_stage(1) == (1.0, 1.0)
    pipe.disable_freeu()
    assert unet._freeu is None and P._model_token(unet) == off
    pipe.enable_freeu(0.9, 0.2, 1.3, 1.4)
    with pytest.raises(NotImplementedError, match="FreeU"):
        pipe(prompt_embeds=torch.zeros(1, 7, 64), use_graph="plan")
    pipe.unet = None
    with pytest.raises(ValueError, match="must have `unet`"):
        pipe.enable_freeu(0.9, 0.2, 1.3, 1.4)
    assert all(not hasattr(c, "enable_freeu") for c in (P.FluxPipeline, P.WanPipeline, P.DDPMPipeline))
    sd = [f"StableDiffusion{xl}{kind}Pipeline" for xl in ("", "XL") for kind in ("", "Img2Img", "Inpaint", "ControlNet", "InstructPix2Pix")]
    assert all(hasattr(getattr(P, name), "enable_freeu") for name in sd)
