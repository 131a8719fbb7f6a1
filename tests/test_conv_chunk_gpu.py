"""GPU tests of the CHUNKED K order of the k x k implicit-GEMM convs of the K2 / K1 family (csrc/gemm2_kernel.cuh cursor_step,
c_beg / c_end, w_off and the C1 | C2 source select; the host rule gemm2_shared.cuh conv_chunk_slices).  For each chunk of channels
the kernel walks all k * k taps, then the next chunk; the tap-major order (every other conv test) walks all channels of tap 0, then
tap 1, ...  The two orders are the same K slices summed in another order.

What must hold, for every chunk size DA_CONV_CHUNK pins (read per launch) and for every conv-capable (tile, staging):
(1) right against a float64 reference at the conv tolerances of test_gemm_k2_gpu.py, a reference gate that provably rejects a
lost 64-channel slice of one tap; (2) bit-identical within each family (k2 / k1) for ONE chunk size; (3) within the k1 / k2
ulp budget of the tap-major result of the same variant, and bit-identical to it where the chunk covers every channel or the
conv is 1 x 1; (4) in auto mode (the shipped default), bit-identical to the chunk ops.conv_chunk_channels reports -- and at the
shipped table's chunked shapes that chunk is not 0, so the path these tests cover is the one the engine runs."""
import json
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close_bf16
from test_gemm_k2_gpu import _conv_ref, _ops, k2_variants, one_ulp, rnd, run_all

pytestmark = pytest.mark.gpu
TABLE = Path(__file__).resolve().parent.parent / "diffusers_amd" / "tuned" / "gfx950.json"
CHUNKS = (0, 64, 128, 192, 256, 320, 1024)   # channels; 0 = tap-major, 1024 >= every Ctot below


def _conv_ref64(x, x2, w4, b, stride, up, ksize, rv=None, res=None, drop=None):
    """The conv in float64 as a sum over the k * k taps of (shifted input) @ (the tap's weight) -- im2col, one tap at a time.
    drop = (tap, c0): leave out channels [c0, c0 + 64) of that tap, i.e. what a kernel that lost that K slice computes."""
    xin = (x if x2 is None else torch.cat([x, x2], dim=-1)).double()
    if up:
        xin = xin.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    B, Hv, Wv, _ = xin.shape
    pad = (ksize - 1) // 2
    Ho, Wo = (Hv + 2 * pad - ksize) // stride + 1, (Wv + 2 * pad - ksize) // stride + 1
    xp = F.pad(xin, (0, 0, pad, pad, pad, pad))
    wd = w4.double()
    y = b.double().expand(B, Ho, Wo, -1).clone()
    for tap in range(ksize * ksize):
        kh, kw = divmod(tap, ksize)
        wt = wd[:, :, kh, kw]
        if drop is not None and drop[0] == tap:
            wt = wt.clone()
            wt[:, drop[1]:drop[1] + 64] = 0
        y += xp[:, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride, :] @ wt.t()
    if rv is not None:
        y += rv.double()[:, None, None, :]
    if res is not None:
        y += res.double()
    return y


def _gate(y, ref64, what):
    assert_close_bf16(y, ref64, what, rtol=8e-3, atol_rms=4e-3)


def _gate_rejects(y, mutant, what):
    """The gate must fail on a reference that lacks one slice of one tap: it cannot hide the bug class under test."""
    with pytest.raises(AssertionError):
        _gate(y, mutant, f"{what} (reference without one slice: must be rejected)")


# B, H, W, C1, C2, Cout, ksize, stride, up   (slices per tap = Ctot / 64; chunk edges of 64 .. 320 channels)
@pytest.mark.parametrize("B,H,W,C1,C2,Co,ks,stride,up", [
    (1, 9, 7, 256, 192, 80, 3, 1, False),      # Ctot 448: 7 slices per tap, 63 in all (odd); chunk edges inside C2 and on C1 | C2; ragged M, N
    (2, 10, 12, 128, 320, 132, 3, 1, False),   # Ctot 448, the concat edge inside the first chunk of 192 / 256 / 320; B = 2, ragged N
    (1, 16, 16, 320, 0, 320, 3, 2, False),     # stride 2, Ctot 320: ragged last chunk for 128 / 192 / 256
    (1, 12, 12, 384, 0, 128, 3, 1, True),      # nearest-2x in the gather, Ctot 384: ragged last chunk for 256 / 320
    (2, 8, 8, 576, 0, 64, 3, 1, False),        # Ctot 576 = 9 slices per tap: every chunk but 64 / 192 ragged; 81 slices
    (1, 16, 16, 192, 256, 128, 1, 1, False),   # 1 x 1 over a concat: nothing to chunk
])
def test_pinned_chunk_sweep(B, H, W, C1, C2, Co, ks, stride, up, monkeypatch):
    ops, L = _ops()
    x = rnd((B, H, W, C1), 51)
    x2 = rnd((B, H, W, C2), 52) if C2 else None
    Ct = C1 + C2
    w4 = rnd((Co, Ct, ks, ks), 53, (ks * ks * Ct) ** -0.5)
    w, b = ops.pack_conv_weight(w4), rnd((Co,), 54)
    Ho, Wo = ((2 * H if up else H) + stride - 1) // stride, ((2 * W if up else W) + stride - 1) // stride
    rv, res = rnd((B, Co), 55), rnd((B, Ho, Wo, Co), 56)
    kw = dict(ksize=ks, x2=x2, stride=stride, up=up, rowvec=rv, residual=res)
    ref = _conv_ref64(x, x2, w4, b, stride, up, ks, rv, res)
    assert tuple(ref.shape) == (B, Ho, Wo, Co)
    # the float64 reference is the conv the other tests check against (fp32 F.conv2d), to fp32 precision
    r32 = _conv_ref(x, x2, w4, b, stride, up, ks, rv, res)
    assert float((r32.double() - ref).abs().max()) <= 1e-4 * float(ref.pow(2).mean().sqrt())
    shape = f"conv{ks} {B}x{H}x{W} {C1}+{C2}->{Co} s{stride} u{int(up)}"

    tap_major = {}
    for chunk in CHUNKS:
        monkeypatch.setenv("DA_CONV_CHUNK", str(chunk))
        what = f"{shape} chunk {chunk}"
        outs = {}

        def conv(t, st):
            outs[(t, st)] = y = ops.conv2d_nhwc(x, w, b, tile=t, staging=st, **kw)
            return y
        run_all(conv, L, what, conv=True, min_ok=6)
        # what the launches used: the query reads the same knob, per call
        want = chunk if (ks > 1 and 0 < chunk < Ct) else 0
        for t in {t for t, _ in outs}:
            assert ops.conv_chunk_channels(x, w, t, ksize=ks, x2=x2, stride=stride, up=up) == want, (what, L.TILE_NAMES[t])
        for fam in ("k2", "k1"):
            y = next((y for (t, _), y in outs.items() if L.TILE_NAMES[t].startswith(fam)), None)
            assert y is not None, f"{what}: no {fam} variant ran"
            _gate(y, ref, f"{what} {fam}")
        if chunk == 0:
            tap_major = outs
            continue
        assert set(outs) == set(tap_major), what
        for (t, st), y in outs.items():
            v = f"{what} {L.TILE_NAMES[t]}/{st} vs tap-major"
            if want == 0:   # a chunk that covers every channel, or a 1 x 1 conv: the tap-major order itself
                assert torch.equal(y, tap_major[(t, st)]), v
            else:
                one_ulp(y, tap_major[(t, st)], v, ulps=1.25)

    # gate sensitivity: the reference minus the centre tap's share of the last 64 channels (in C2 when there is one)
    if ks > 1:
        y = tap_major[next(iter(tap_major))]
        mutant = _conv_ref64(x, x2, w4, b, stride, up, ks, rv, res, drop=(ks * ks // 2, Ct - 64))
        _gate_rejects(y, mutant, shape)


def _table_tile(key):
    return json.loads(TABLE.read_text())["entries"][key][0]


# The shipped table's chunked entries (tuned/gfx950.json key, B, H, W, C1, C2, Cout, the auto chunk of the table's tile), and the
# skip concat of SDXL's 128 x 128 up level (640 + 320 channels, which the table keys as one source): chunk edges at 256, 512 and
# 768 (inside C2), ragged last chunk of 192.
SHIPPED = [
    ("conv3:M32768:N320:C640+0:H128x128:s1:u0:a0:r0", 2, 128, 128, 640, 0, 320, 256),
    ("conv3:M32768:N320:C960+0:H128x128:s1:u0:a0:r0", 2, 128, 128, 960, 0, 320, 256),
    ("conv3:M8192:N640:C1920+0:H64x64:s1:u0:a0:r0", 2, 64, 64, 1920, 0, 640, 1024),
    ("conv3:M65536:N256:C512+0:H256x256:s1:u0:a0:r0", 1, 256, 256, 512, 0, 256, 256),
    ("conv3:M262144:N256:C512+0:H512x512:s1:u0:a0:r0", 1, 512, 512, 512, 0, 256, 256),
    ("conv3:M32768:N320:C960+0:H128x128:s1:u0:a0:r0", 2, 128, 128, 640, 320, 320, 256),
]


@pytest.mark.parametrize("key,B,H,W,C1,C2,Co,chunk", SHIPPED, ids=[f"{s[0].split(':H')[0]}:{s[4]}+{s[5]}" for s in SHIPPED])
def test_auto_chunk_at_shipped_shapes(key, B, H, W, C1, C2, Co, chunk, monkeypatch):
    ops, L = _ops()
    monkeypatch.delenv("DA_CONV_CHUNK", raising=False)
    Ct = C1 + C2
    x = rnd((B, H, W, C1), 61)
    x2 = rnd((B, H, W, C2), 62) if C2 else None
    w4 = rnd((Co, Ct, 3, 3), 63, (9 * Ct) ** -0.5)
    w, b = ops.pack_conv_weight(w4), rnd((Co,), 64)
    shape = f"conv3 {B}x{H}x{W} {C1}+{C2}->{Co}"
    tile = _table_tile(key)
    assert ops.conv_chunk_channels(x, w, tile, x2=x2) == chunk, f"{shape}: {L.TILE_NAMES[tile]} no longer takes the chunked order"
    ref = _conv_ref64(x, x2, w4, b, 1, False, 3)
    gated, chunked, ran_table_tile = [], 0, False
    for t, st in k2_variants(L, conv=True):
        monkeypatch.delenv("DA_CONV_CHUNK", raising=False)
        try:
            y = ops.conv2d_nhwc(x, w, b, x2=x2, tile=t, staging=st)
        except RuntimeError as e:
            assert "DA_ERR_UNSUPPORTED" in str(e), f"{shape} {L.TILE_NAMES[t]}/{st}: {e}"
            continue
        q = ops.conv_chunk_channels(x, w, t, x2=x2)
        what = f"{shape} {L.TILE_NAMES[t]}/{st} auto (chunk {q})"
        ran_table_tile |= t == tile
        chunked += q > 0
        monkeypatch.setenv("DA_CONV_CHUNK", str(q))
        assert torch.equal(y, ops.conv2d_nhwc(x, w, b, x2=x2, tile=t, staging=st)), f"{what}: differs from DA_CONV_CHUNK={q}"
        if not any(torch.equal(y, g) for g in gated):   # (one gate per distinct result)
            _gate(y, ref, what)
            gated.append(y)
    assert ran_table_tile, f"{shape}: the table's tile {L.TILE_NAMES[tile]} did not run"
    print(f"[parity] {shape}: {chunked} chunked variants, {len(gated)} distinct results")
    if key.startswith("conv3:M8192"):   # gate sensitivity at full size: one lost slice of the last (ragged) chunk
        mutant = _conv_ref64(x, x2, w4, b, 1, False, 3, drop=(4, Ct - 64))
        _gate_rejects(gated[0], mutant, shape)
