"""FreeU on the GPU: da_freeu_nhwc_bf16 against the float64 transcription of the reference (tests/freeu_reference.py), its exact
structure, footprint and refusals, its place in the U-Net's up walk and the pipelines' eager / captured-graph behaviour."""
import pytest
import torch

import call_sequences as CS
import footprint as FP
import freeu_reference as FR
from conftest import rel_rms
from diffusers_amd import _lib as L, factory, init as dinit, ops

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
DEV = "cuda"
INVALID, UNSUPPORTED = 1, 3
MODEL_REL_RMS = 2.5e-2          # the gate tests/test_models_gpu.py applies to the tiny U-Nets
# (47, 47) x 64 channels is the largest plane whose 32-channel slab fits the LDS-resident path, (48, 48) the first that forces the
# two-launch path (the issue's (96, 96), adjusted); at (64, 64) 8 channels are resident and 24 / 320 run the multi-band partials.
CASES = [(hw, cs) for hw in [(2, 2), (3, 5), (8, 8), (16, 24), (33, 32), (64, 64)] for cs in (8, 24, 320)] + [((47, 47), 64), ((48, 48), 64)]


@pytest.mark.parametrize("s", [0.2, 0.9])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw,Cs", CASES)
def test_kernel_against_float64(hw, Cs, B, s):
    """|skip_out - ref64| <= 2^-8 |ref64| (one bf16 rounding) + 8 x the largest error of the reference's own fp32 torch.fft route
    against the float64 route on these inputs; hidden: torch's x * b to the bit, the other half untouched."""
    b, hidden, skip = 1.4, FR.data(B, *hw, 2 * Cs, seed=1), FR.data(B, *hw, Cs, seed=2)
    want_hidden, ref = FR.apply_freeu(hidden, skip, s, b)
    slack = 8 * float((FR.fourier_filter(skip, s, dtype=torch.float32).double() - ref).abs().max())
    resident = L.load().da_freeu_workspace_bytes(B, *hw, Cs, L.FREEU_AUTO) == 0
    assert resident == (hw[0] * hw[1] * min(Cs, 32) <= 47 * 47 * 32)
    h = hidden.to(DEV)
    out = ops.freeu(h, skip.to(DEV), s=s, b=b)
    assert FP.bits_equal(h.cpu(), want_hidden)
    err = (out.cpu().double() - ref).abs()
    excess = float((err - (2.0 ** -8 * ref.abs() + slack)).max())
    print(f"[freeu] {hw} Cs={Cs} B={B} s={s} resident={resident}: slack/8={slack / 8:.3e} beyond one rounding={float((err - 2.0 ** -8 * ref.abs()).max()):.3e}")
    assert excess <= 0, f"{excess:.3e} over the bound"


@pytest.mark.parametrize("path", [L.FREEU_RESIDENT, L.FREEU_TWO_LAUNCH])
@pytest.mark.parametrize("hw", [(4, 4), (8, 16), (32, 32)])
def test_exact_structure(hw, path):
    """A Nyquist checkerboard has nothing in the four bins and comes back to the bit; a constant plane is its own zero bin and comes
    back as c / 2 with s = 0.5; s = 1, b = 1 is the identity."""
    H, W = hw
    c = torch.tensor([1.0, -3.140625, 0.001, 240.0, 2.0 ** -20, -1e20, 7.5e-10, 96.0] * 3).to(bf16)
    sign = (1 - 2 * ((torch.arange(H).view(H, 1) + torch.arange(W).view(1, W)) % 2)).to(bf16)
    board = (sign.view(1, H, W, 1) * c.view(1, 1, 1, -1)).expand(2, H, W, 24).contiguous()
    flat = c.view(1, 1, 1, -1).expand(2, H, W, 24).contiguous()
    hidden = FR.data(2, H, W, 48, seed=3)
    run = lambda x, s, b=1.3: ops.freeu(hidden.to(DEV), x.to(DEV), s=s, b=b, path=path).cpu()  # noqa: E731
    assert FP.bits_equal(run(board, 0.2), board)
    assert FP.bits_equal(run(flat, 0.5), (flat.float() / 2).to(bf16))
    skip, h = FR.data(2, H, W, 24, seed=4), hidden.to(DEV)
    assert FP.bits_equal(ops.freeu(h, skip.to(DEV), s=1.0, b=1.0, path=path).cpu(), skip) and FP.bits_equal(h.cpu(), hidden)


def _guarded_call(sized_for, poison=True, offsets=(), **over):
    """One raw call on guarded buffers of a 2 x 8 x 8 problem sized for path ``sized_for``; ``over`` replaces arguments, ``offsets`` shifts
    pointers by bytes.  Returns (status, the four guards, their bits before the call, the inputs)."""
    B, H, W, Cs = 2, 8, 8, 24
    hidden, skip = FR.data(B, H, W, 2 * Cs, seed=5), FR.data(B, H, W, Cs, seed=6)
    gh, gs = FP.poisoned(hidden), FP.poisoned(skip)
    if not poison:
        gh, gs = gh.clean(), gs.clean()
    go = FP.guarded((B, H, W, Cs))
    lib = L.load()
    nbytes = lib.da_freeu_workspace_bytes(B, H, W, Cs, sized_for)
    gw = FP.guarded(max(nbytes // 4, 4), dtype=torch.float32)
    a = dict(hidden=gh.ptr(), skip=gs.ptr(), out=go.ptr(), tw=ops.freeu_twiddles(H, W, DEV).data_ptr(), ws=gw.ptr(), nbytes=nbytes, B=B,
             H=H, W=W, Cx=2 * Cs, Cs=Cs, b=1.4, s=0.2, path=sized_for)
    a.update(over)
    for k, off in offsets:
        a[k] += off
    guards = (gh, gs, go, gw)
    before = [g.snapshot() for g in guards]
    rc = lib.da_freeu_nhwc_bf16(*(a[k] for k in ("hidden", "skip", "out", "tw", "ws", "nbytes", "B", "H", "W", "Cx", "Cs", "b", "s", "path")),
                                ops._stream())
    torch.cuda.synchronize()
    return rc, guards, before, (hidden, skip)


@pytest.mark.parametrize("path", [L.FREEU_RESIDENT, L.FREEU_TWO_LAUNCH])
def test_footprint(path):
    rc, (gh, gs, go, gw), before, (hidden, skip) = _guarded_call(path)
    assert rc == L.DA_OK
    for g, what in ((gh, "hidden"), (gs, "skip"), (go, "skip_out"), (gw, "workspace")):
        g.check(what)
    assert torch.equal(gs.snapshot(), before[1])                                           # read only
    rc, clean, _, _ = _guarded_call(path, poison=False)
    assert rc == L.DA_OK and FP.bits_equal(go.view, clean[2].view) and FP.bits_equal(gh.view, clean[0].view)
    assert FP.bits_equal(go.view, ops.freeu(hidden.to(DEV), skip.to(DEV), s=0.2, b=1.4, path=path))
    assert (path == L.FREEU_TWO_LAUNCH) == bool((gw.snapshot() != before[3]).any())


@pytest.mark.parametrize("over,code", [
    (dict(hidden=None), INVALID), (dict(skip=None), INVALID), (dict(out=None), INVALID), (dict(tw=None), INVALID),
    (dict(ws=None), INVALID), (dict(nbytes=16), INVALID), (dict(B=0), INVALID), (dict(H=-1), INVALID), (dict(Cs=0), INVALID),
    (dict(Cx=0), INVALID), (dict(s=float("inf")), INVALID), (dict(b=float("nan")), INVALID), (dict(path=3), INVALID),
    (dict(offsets=(("skip", 2),)), INVALID), (dict(offsets=(("out", 8),)), INVALID), (dict(offsets=(("hidden", 4),)), INVALID),
    (dict(Cs=20), UNSUPPORTED), (dict(Cx=40), UNSUPPORTED), (dict(H=1), UNSUPPORTED), (dict(W=1), UNSUPPORTED),
    (dict(H=64, W=64, Cs=64, path=L.FREEU_RESIDENT), UNSUPPORTED)], ids=str)
def test_refusals_launch_nothing(over, code):
    rc, guards, before, _ = _guarded_call(L.FREEU_TWO_LAUNCH, **over)
    assert rc == code
    assert all(torch.equal(g.snapshot(), b) for g, b in zip(guards, before))


def test_unet_placement_and_forward(monkeypatch):
    """ops.freeu runs once per resnet of up blocks 0 and 1 with the block's (s, b), never later; the forward with the op replaced by
    the float64 restatement agrees within the model tests' bf16 gate."""
    cfg = dict(dinit.TINY_SD15_UNET, block_out_channels=(64, 64, 128), down_block_types=("CrossAttnDownBlock2D", "DownBlock2D", "DownBlock2D"),
               up_block_types=("UpBlock2D", "UpBlock2D", "CrossAttnUpBlock2D"), attention_head_dim=(1, 1, 2))
    unet, _ = factory.build_unet(cfg, seed=0, device=DEV)
    x, ctx = CS._rand((2, 4, 16, 16), 7).to(DEV), CS._rand((2, 7, 64), 8).to(DEV)
    plain = unet(x, 500, ctx, return_dict=False)[0]
    unet.enable_freeu(s1=0.9, s2=0.2, b1=1.3, b2=1.4)
    real, calls = ops.freeu, []

    def spy(hidden, skip, *, s, b, path=0):
        calls.append((s, b, tuple(hidden.shape[1:3])))
        return real(hidden, skip, s=s, b=b, path=path)

    def restated(hidden, skip, *, s, b, path=0):
        h, y = FR.apply_freeu(hidden.cpu(), skip.cpu(), s, b)
        hidden.copy_(h)
        return y.to(bf16).to(DEV)
    monkeypatch.setattr(ops, "freeu", spy)
    got = unet(x, 500, ctx, return_dict=False)[0]
    assert calls == [(0.9, 1.3, (4, 4))] * 2 + [(0.2, 1.4, (8, 8))] * 2
    monkeypatch.setattr(ops, "freeu", restated)
    want = unet(x, 500, ctx, return_dict=False)[0]
    assert bool(torch.isfinite(got.float()).all()) and rel_rms(got, want) < MODEL_REL_RMS
    assert not torch.equal(got, plain)


@pytest.mark.parametrize("family", ["sd15", "sdxl", "sdxl_img2img"])
def test_pipelines(family):
    fam = CS.FAMILIES[family]
    pipe, kw = fam.build(DEV), fam.kwargs
    never = CS.run(pipe, kw, True)
    pipe.enable_freeu(s1=0.9, s2=0.2, b1=1.3, b2=1.4)
    eager, graph = CS.run(pipe, kw, False), CS.run(pipe, kw, True)
    assert torch.equal(eager, graph) and not torch.equal(graph, never) and bool(torch.isfinite(graph.float()).all())
    pipe.enable_freeu(s1=0.9, s2=0.6, b1=1.3, b2=1.4)                       # the second call recaptures: no stale step
    changed = CS.run(pipe, kw, True)
    assert not torch.equal(changed, graph) and torch.equal(changed, CS.run(pipe, kw, False))
    with pytest.raises(NotImplementedError, match="FreeU"):
        CS.run(pipe, kw, "plan")
    pipe.enable_freeu(1, 1, 1, 1)
    assert torch.equal(CS.run(pipe, kw, True), never)
    pipe.disable_freeu()
    assert torch.equal(CS.run(pipe, kw, True), never)
