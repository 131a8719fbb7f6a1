"""CPU tests of tests/large_address.py: the conditions the periodic-tensor construction enforces (on meta tensors and tiny tensors),
and its detection power -- a copy kernel whose gather or scatter wraps at 2^31 B, 2^32 B or 2^32 elements fails the periodicity
check or the period-0 comparison, for every operand layout of tests/test_large_address_gpu.py."""
import pytest
import torch

import large_address as LA

LAYOUTS = LA.layouts()


# ---- the conditions ----
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_layout_meets_the_conditions(name):
    pl = LAYOUTS[name]
    # the conditions, restated independently of check_conditions
    for b in (31, 32, 33):
        assert (1 << b) % pl.period_bytes != 0, f"{name}: period divides 2^{b} B"
    for e in (31, 32):
        assert (1 << e) % pl.period_elems != 0, f"{name}: period divides 2^{e} elements"
    assert (pl.P * pl.rows_per_frame) % 256 != 0
    assert pl.T % pl.P == 0
    for label, f in pl.boundary_frames.items():
        b = LA.boundary_bytes(pl.itemsize)[label]
        assert f * pl.frame_bytes < b < (f + 1) * pl.frame_bytes, f"{name}: {label} not strictly inside frame {f}"
        assert pl.T - 1 - f >= LA.TRAIL_FRAMES
    # a meta tensor of the planned shape has the planned size, and the reported frames are where the boundaries are
    t = torch.empty((pl.T, pl.frame_elems), dtype=torch.bfloat16, device="meta")
    assert t.numel() * t.element_size() == pl.nbytes
    print(f"[layout] {pl.name}: T = {pl.T} frames of {pl.frame_bytes} B = {pl.nbytes / 2**30:.3f} GiB, P = {pl.P}, boundaries in frames "
          f"{pl.boundary_frames}")


def test_the_tiers_pass_their_boundaries():
    for name, pl in LAYOUTS.items():
        labels = set(pl.boundary_frames)
        if name in ("A_c128", "A_up_out", "A_lin_out", "A_perm"):
            assert {"2^31 B", "2^32 B", "2^31 elements"} <= labels and "2^33 B" not in labels, (name, labels)
            assert pl.nbytes < 1.4 * 2 ** 32                      # "just over": no more than the boundary asks for
        if name in ("B_c128", "B_perm"):
            assert {"2^31 B", "2^32 B", "2^33 B", "2^31 elements", "2^32 elements"} == labels, (name, labels)
            assert pl.nbytes < 1.01 * 2 ** 33
    assert "2^31 B" in LAYOUTS["A_lin_in"].boundary_frames and "2^31 B" in LAYOUTS["A_up_in"].boundary_frames
    # rows of the GEMM stay below 2^31 (da_gemm_params.M is an int), pixels too
    assert LAYOUTS["B_c128"].T * LA.HW < 2 ** 31


@pytest.mark.parametrize("kw,msg", [
    (dict(frame_elems=1 << 14, rows_per_frame=15, P=8, T=16 * 8), "divides 2^31 B"),          # power-of-two period
    (dict(frame_elems=960 * 128, rows_per_frame=960, P=4, T=4 * 4400), "multiple of 256"),   # 4 * 960 = 15 * 256
    (dict(frame_elems=960 * 128, rows_per_frame=960, P=7, T=7 * 2496), "do not pass"),       # 17472 frames: short of 4 GiB
    (dict(frame_elems=960 * 128, rows_per_frame=960, P=7, T=17479), None),                 # 7 * 2497 frames: exactly two trail frames
    (dict(frame_elems=960 * 128, rows_per_frame=960, P=3, T=17478), "whole frame(s) past"),  # one trail frame only
    (dict(frame_elems=(1 << 20) * 15, rows_per_frame=15, P=7, T=7 * 20), None),
    (dict(frame_elems=1 << 20, rows_per_frame=15, P=7, T=7 * 300), "falls on a frame edge"),  # power-of-two frame, odd period
    (dict(frame_elems=960 * 128, rows_per_frame=960, P=7, T=17480), "no multiple of the period"),
])
def test_conditions_are_enforced(kw, msg):
    if msg is None:
        LA.check_conditions(tier="A", **kw)
        return
    with pytest.raises(ValueError, match=msg.replace("(", r"\(").replace(")", r"\)").replace("^", r"\^")):
        LA.check_conditions(tier="A", **kw)


# ---- building and checking tiny tensors ----
def test_repeat_block_and_first_aperiodic_on_tiny_tensors():
    block = LA.random_block((3, 5, 8), seed=1, zero_from_channel=6)
    assert block.dtype == torch.bfloat16 and bool((block[..., 6:] == 0).all()) and bool((block[..., :6] != 0).any())
    assert torch.equal(block, LA.random_block((3, 5, 8), seed=1, zero_from_channel=6))     # seeded
    t = LA.repeat_block(block, 12)
    assert t.shape == (12, 5, 8) and all(torch.equal(t[3 * k:3 * k + 3], block) for k in range(4))
    assert LA.first_aperiodic(t, 3) is None
    LA.assert_periodic(t, 3, "tiny")
    with pytest.raises(ValueError):
        LA.repeat_block(block, 13)
    # one flipped bit anywhere is found and located: period, frame, flat byte offset
    for frame, r, c in [(3, 0, 0), (7, 4, 7), (11, 2, 3)]:
        u = t.clone()
        u.view(torch.int16)[frame, r, c] ^= 1
        k, f, off = LA.first_aperiodic(u, 3, chunk_periods=2)
        assert (k, f, off) == (frame // 3, frame, ((frame * 5 + r) * 8 + c) * 2)
        with pytest.raises(AssertionError, match=f"period {frame // 3} differs from period 0 first in frame {frame}, flat byte offset {off} "):
            LA.assert_periodic(u, 3, "tiny")
    # integer comparison: -0 is not +0, and a NaN equals itself
    z = torch.zeros((4, 2, 8), dtype=torch.bfloat16)
    z[2, 1, 1] = -0.0
    assert LA.first_aperiodic(z, 2) == (1, 2, (2 * 16 + 9) * 2)
    nan = torch.full((4, 2, 8), float("nan"), dtype=torch.bfloat16)
    assert LA.first_aperiodic(nan, 2) is None
    # a shifted start (the causal conv: periodic from frame 1 on)
    s = torch.cat([torch.full((1, 5, 8), 9.0, dtype=torch.bfloat16), t])
    LA.assert_periodic(s, 3, "shifted", first_frame=1)
    with pytest.raises(AssertionError):
        LA.assert_periodic(s[:12], 3, "unshifted")
    # an incomplete last period must repeat the start of period 0
    assert LA.first_aperiodic(t[:11], 3) is None
    u = t[:11].clone()
    u.view(torch.int16)[10, 1, 2] ^= 4
    assert LA.first_aperiodic(u, 3) == (3, 10, ((10 * 5 + 1) * 8 + 2) * 2)


# ---- detection power ----
def _block_bits(pl):
    g = torch.Generator("cpu").manual_seed(5)
    # distinct-ish integer patterns of finite bf16 values, never the FILL pattern
    return torch.randint(1, 0x7F00, (pl.period_elems,), generator=g, dtype=torch.int32).to(torch.int16)


WRAPS = [("2^31 B", dict(wrap_bytes=1 << 31)), ("2^32 B", dict(wrap_bytes=1 << 32)), ("2^32 elements", dict(wrap_elems=1 << 32)),
         ("2^31 elements", dict(wrap_elems=1 << 31))]


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_wrapped_access_is_detected(name):
    """The correct copy passes both checks; a gather or scatter narrowed at any boundary the tensor passes fails one of them."""
    pl = LAYOUTS[name]
    bits = _block_bits(pl)
    ks = LA.periods_to_look_at(pl)
    assert LA.detected(pl, LA.emulate(pl, bits, ks), bits, ks) is None
    assert LA.detected(pl, LA.emulate(pl, bits, ks, side="write"), bits, ks) is None
    seen = []
    for label, kw in WRAPS:
        if label not in pl.boundary_frames:
            # the tensor ends below this boundary: such a kernel is correct on it, and the checks must not cry wolf
            assert LA.detected(pl, LA.emulate(pl, bits, ks, **kw), bits, ks) is None, (name, label)
            continue
        for side in ("read", "write"):
            got = LA.detected(pl, LA.emulate(pl, bits, ks, side=side, **kw), bits, ks)
            assert got is not None, f"{name}: a {side} wrapped at {label} went unnoticed"
            seen.append(f"{side}@{label}: {got}")
        # the periodicity check names a frame at or after the boundary for a wrapped read (everything before it is untouched)
        out = LA.emulate(pl, bits, ks, **kw)
        k, frame, _ = LA.first_aperiodic(out, pl.P)
        assert ks[k] * pl.P + frame % pl.P >= pl.boundary_frames[label], (name, label, ks[k], frame)
    print(f"[detect] {pl.name}: {', '.join(seen) if seen else 'no boundary reached (companion operand)'}")
    if name not in ("A_n4",):
        assert seen, f"{name}: a large layout that reaches no boundary"


def test_period_zero_check_alone_catches_a_wrapped_write():
    """Looking only at period 0 (what the fp64 reference does) already sees a scatter that wrapped: the tensor's tail landed there."""
    pl = LAYOUTS["A_c128"]
    bits = _block_bits(pl)
    out = LA.emulate(pl, bits, [0], wrap_bytes=1 << 32, side="write")
    assert LA.first_aperiodic(out, pl.P) is None and LA.detected(pl, out, bits, [0]) == "period 0"
