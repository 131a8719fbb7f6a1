"""Periodic multi-GB tensors for the kernel tests: operands whose byte offsets pass 2^31 / 2^32 / 2^33 and whose element indices
pass 2^31 / 2^32, checked everywhere at the cost of one small reference.

A tensor of ``T`` frames is ONE random block of ``P`` frames (values from tests/value_domain.py, a seed) repeated ``T / P`` times.
For an op that is independent per frame (a 2-D conv over frames-as-batch, a row-wise GEMM, a channel norm, a per-frame permute) a
periodic input gives a BIT-periodic output: ``out.view(T / P, P, ...)[k]`` equals ``[0]`` for every ``k``.  That one comparison looks
at every tile of the whole tensor; period 0 (and the frames that hold the boundaries) are then compared with an fp64 reference of
``P`` frames.  A kernel whose address arithmetic wraps at a boundary ``W`` reads (or writes) ``W`` bytes too low; because the period
does not divide ``W`` the wrapped access lands on DIFFERENT data, so the output stops being periodic at the boundary (a wrapped
read), or keeps its initial fill there and is overwritten near the start (a wrapped write: the period-0 reference sees it).

``plan()`` enforces the conditions this argument needs -- they are conditions of the construction, not measurements:

* the period in bytes divides none of 2^31, 2^32, 2^33 and the period in elements divides none of 2^31, 2^32 (the boundaries are
  powers of two: the period must not be one; a 24 x 40 frame, with its factor 15, gives that for every channel count);
* ``P * rows_per_frame`` is no multiple of 256 (the tallest tile), so tiles sit differently in every period;
* every boundary of the tier falls strictly INSIDE a frame, and at least two whole frames follow the highest one;
* the frames that contain each boundary are reported (``Plan.boundary_frames``).

Plain module (no fixtures, no pytest settings); its CPU tests are tests/test_large_address_cpu.py.  The kernel-level tests that feed
these tensors to the kernels are tests/test_large_address_gpu.py.  ``emulate()`` is a lazily
evaluated small emulation of a copy kernel over such a tensor, with a deliberately wrapped gather or scatter: the proof that the
checks detect the bug class (it evaluates only the periods asked for, so the true 2^31 / 2^32 boundaries cost nothing on a CPU).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

import value_domain as V

bf16 = torch.bfloat16
TILE_ROWS = 256                                   # the tallest tile of any kernel in the library
BYTE_BOUNDARIES = (1 << 31, 1 << 32, 1 << 33)
ELEM_BOUNDARIES = (1 << 31, 1 << 32)
TIER_TOP_BYTES = {"A": 1 << 32, "B": 1 << 33}     # tier A: just over 4 GiB (2^31 bf16 elements); tier B: just over 8 GiB (2^32)
TRAIL_FRAMES = 2                                  # whole frames required past the highest boundary
FRAME_HW = (24, 40)                               # 960 pixels: 2^6 * 15


@dataclass(frozen=True)
class Plan:
    """Geometry of one periodic tensor: ``T`` frames of ``frame_elems`` elements, period ``P`` frames."""
    name: str
    frame_elems: int
    rows_per_frame: int
    P: int
    T: int
    tier: str
    itemsize: int = 2
    boundary_frames: Dict[str, int] = field(default_factory=dict, compare=False)   # "2^31 B" -> frame that contains it

    @property
    def frame_bytes(self) -> int:
        return self.frame_elems * self.itemsize

    @property
    def period_elems(self) -> int:
        return self.P * self.frame_elems

    @property
    def period_bytes(self) -> int:
        return self.period_elems * self.itemsize

    @property
    def nbytes(self) -> int:
        return self.T * self.frame_bytes

    @property
    def periods(self) -> int:
        return self.T // self.P


def _label(bytes_: int, elems: bool) -> str:
    return f"2^{bytes_.bit_length() - 1} {'elements' if elems else 'B'}"


def boundary_bytes(itemsize: int = 2) -> Dict[str, int]:
    """label -> byte offset of every boundary, byte and element boundaries alike (the labels of Plan.boundary_frames)."""
    out = {_label(b, False): b for b in BYTE_BOUNDARIES}
    out.update({_label(e, True): e * itemsize for e in ELEM_BOUNDARIES})
    return out


def check_conditions(frame_elems: int, rows_per_frame: int, P: int, T: int, tier: Optional[str], itemsize: int = 2) -> Dict[str, int]:
    """Raise ValueError unless (frame, P, T) meets every condition of the module docstring; returns the boundary frames.
    ``tier`` None: a companion operand that need not reach a boundary (the small side of a conv) -- period conditions only, and the
    boundaries it does pass must still fall inside a frame with the trailing frames behind the highest."""
    fb, pe = frame_elems * itemsize, P * frame_elems
    pb = pe * itemsize
    if T % P:
        raise ValueError(f"T = {T} is no multiple of the period P = {P}")
    for b in BYTE_BOUNDARIES:
        if b % pb == 0:
            raise ValueError(f"the period, {pb} B, divides 2^{b.bit_length() - 1} B: a wrapped address would land on the same data")
    for e in ELEM_BOUNDARIES:
        if e % pe == 0:
            raise ValueError(f"the period, {pe} elements, divides 2^{e.bit_length() - 1} elements")
    if (P * rows_per_frame) % TILE_ROWS == 0:
        raise ValueError(f"P * rows_per_frame = {P * rows_per_frame} is a multiple of {TILE_ROWS}: tiles sit alike in every period")
    total = T * fb
    if tier is not None and total <= TIER_TOP_BYTES[tier]:
        raise ValueError(f"{total} B do not pass the tier's boundary 2^{TIER_TOP_BYTES[tier].bit_length() - 1} B")
    frames, highest = {}, 0
    for label, b in boundary_bytes(itemsize).items():
        if b >= total:
            continue
        if b % fb == 0:
            raise ValueError(f"{label} falls on a frame edge (frame {b // fb})")
        frames[label] = b // fb
        highest = max(highest, b // fb)
    if frames and T - 1 - highest < TRAIL_FRAMES:
        raise ValueError(f"only {T - 1 - highest} whole frame(s) past the highest boundary (frame {highest}); {TRAIL_FRAMES} required")
    return frames


def plan(name: str, frame_elems: int, rows_per_frame: int, tier: str, P: int = 7, itemsize: int = 2, min_frames: int = 0) -> Plan:
    """The shortest tensor of whole periods that passes the tier's top boundary by TRAIL_FRAMES frames (or ``min_frames``)."""
    fb = frame_elems * itemsize
    need = max(TIER_TOP_BYTES[tier] // fb + 1 + TRAIL_FRAMES, min_frames)
    T = (need + P - 1) // P * P
    return Plan(name, frame_elems, rows_per_frame, P, T, tier, itemsize, check_conditions(frame_elems, rows_per_frame, P, T, tier, itemsize))


def companion(name: str, frame_elems: int, rows_per_frame: int, like: Plan, itemsize: int = 2) -> Plan:
    """The other operand of an op whose frame count is set by ``like`` (same T, same P): it passes whatever boundaries its own
    frame size reaches."""
    return Plan(name, frame_elems, rows_per_frame, like.P, like.T, like.tier, itemsize,
                check_conditions(frame_elems, rows_per_frame, like.P, like.T, None, itemsize))


# ----------------------------------------------------------------------------------------------------------------------
# The operand layouts of tests/test_large_address_gpu.py (bf16).  hw = 960 pixels per frame unless noted.
# ----------------------------------------------------------------------------------------------------------------------
HW = FRAME_HW[0] * FRAME_HW[1]


def layouts() -> Dict[str, Plan]:
    a_c128 = plan("A: [T][24][40][128] conv / norm activations", HW * 128, HW, "A")
    a_lin_out = plan("A: [T*960][384] temporal 1x1 conv output", HW * 384, HW, "A")
    a_perm = plan("A: [T][960][2][384] permute operand", HW * 768, HW * 2, "A")
    # the upsampling conv: the N = 128 output passes 4 GiB; its 12 x 20 x 192 input is 2.67 x smaller and passes 2 GiB (an input past
    # 4 GiB would need an 11.5 GB output: more than the tier holds)
    a_up_in_frames = (1 << 31) // (240 * 192 * 2) + 1 + TRAIL_FRAMES
    a_up_out = plan("A: [T][24][40][128] output of the upsampling conv", HW * 128, HW, "A", min_frames=a_up_in_frames)
    b_c128 = plan("B: [T][24][40][128] conv / norm activations", HW * 128, HW, "B")
    b_perm = plan("B: [T][960][2][384] permute operand", HW * 768, HW * 2, "B")
    return {
        "A_c128": a_c128,
        "A_n4": companion("A: [T][24][40][4] thin conv output", HW * 4, HW, a_c128),
        "A_up_out": a_up_out,
        "A_up_in": companion("A: [T][12][20][192] input of the upsampling conv", 240 * 192, 240, a_up_out),
        "A_lin_out": a_lin_out,
        "A_lin_in": companion("A: [T*960][192] temporal 1x1 conv input", HW * 192, HW, a_lin_out),
        "A_perm": a_perm,
        "B_c128": b_c128,
        "B_perm": b_perm,
    }


# ----------------------------------------------------------------------------------------------------------------------
# building and checking real tensors
# ----------------------------------------------------------------------------------------------------------------------
def random_block(shape, seed: int, scale: float = 1.0, zero_from_channel: Optional[int] = None) -> torch.Tensor:
    """One period: bf16 N(0, scale^2) values from value_domain's seeded generator; channels >= ``zero_from_channel`` are zero
    (the channel padding that da_gemm_params.k_valid declares)."""
    x = V._randn(tuple(shape), seed) * scale
    if zero_from_channel is not None:
        x[..., zero_from_channel:] = 0
    return x.to(bf16)


def repeat_block(block: torch.Tensor, T: int, device=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``block`` [P, ...] repeated along dim 0 to T frames (T a multiple of P), written straight into one allocation."""
    P = block.shape[0]
    if T % P:
        raise ValueError(f"T = {T} is no multiple of the period {P}")
    device = block.device if device is None else device
    if out is None:
        out = torch.empty((T,) + tuple(block.shape[1:]), dtype=block.dtype, device=device)
    out.view((T // P, P) + tuple(block.shape[1:])).copy_(block.to(device).unsqueeze(0))
    return out


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def first_aperiodic(t: torch.Tensor, P: int, chunk_periods: int = 64):
    """None if ``t`` (frames on dim 0, contiguous) is bit-periodic with period P, else (period k, frame, flat byte offset) of the
    first element that differs from its image in period 0.  Compared as integers: NaN == NaN, -0 != +0."""
    if not t.is_contiguous():
        raise ValueError("first_aperiodic: contiguous tensor required")
    n, tail = divmod(t.shape[0], P)
    fe = t[0].numel()
    v = _bits(t[:n * P]).view(n, -1)
    for k0 in range(1, n, chunk_periods):
        k1 = min(n, k0 + chunk_periods)
        bad = (v[k0:k1] != v[0]).any(dim=1)
        if bool(bad.any()):
            k = k0 + int(torch.nonzero(bad)[0])
            e = int(torch.nonzero(v[k] != v[0])[0])
            flat = k * v.shape[1] + e
            return k, flat // fe, flat * t.element_size()
    if tail:    # an incomplete last period (a tensor that lost a frame to a temporal shift) repeats the start of period 0
        w = _bits(t[n * P:]).reshape(-1)
        d = w != v[0][:w.numel()]
        if bool(d.any()):
            flat = n * P * fe + int(torch.nonzero(d)[0])
            return n, flat // fe, flat * t.element_size()
    return None


def assert_periodic(t: torch.Tensor, P: int, what: str, first_frame: int = 0) -> None:
    """Periodicity of ``t[first_frame:]``; the failure names the first differing period, the frame and the flat byte offset."""
    hit = first_aperiodic(t[first_frame:], P)
    if hit is not None:
        k, frame, off = hit
        frame_bytes = t[0].numel() * t.element_size()
        off += first_frame * frame_bytes
        raise AssertionError(f"{what}: not periodic -- period {k} differs from period 0 first in frame {frame + first_frame}, flat byte "
                             f"offset {off} (= 2^31 + {off - (1 << 31)}, 2^32 + {off - (1 << 32)}, 2^33 + {off - (1 << 33)})")


# ----------------------------------------------------------------------------------------------------------------------
# CPU emulation: a copy kernel with a wrapped gather / scatter, evaluated lazily
# ----------------------------------------------------------------------------------------------------------------------
FILL = -(1 << 15)       # int16 pattern an output holds before the kernel runs (bf16 -0)


def sample_positions(pl: Plan, step: int = 53) -> torch.Tensor:
    """Element positions inside a frame that the emulation evaluates: all of a small frame, every ``step``-th of a large one (the
    checks are elementwise, so a subset that fails them fails them; 53 is coprime to every channel count, so all channels occur)."""
    return torch.arange(0, pl.frame_elems, 1 if pl.frame_elems <= (1 << 16) else step, dtype=torch.int64)


def emulate(pl: Plan, block_bits: torch.Tensor, periods: Sequence[int], wrap_bytes: Optional[int] = None, wrap_elems: Optional[int] = None,
            side: str = "read") -> torch.Tensor:
    """Periods ``periods`` of the output of ``out[i] = x[i]`` over the periodic tensor of ``pl`` whose period holds the integer
    patterns ``block_bits`` (flat, period_elems long), as [len(periods) * P][sampled frame elements] (sample_positions).  The kernel's
    address arithmetic is narrowed: ``wrap_bytes`` = W reduces the byte offset mod W, ``wrap_elems`` = W the element index -- on the
    gather (``side`` = "read") or on the scatter ("write": elements at i >= W land at i mod W, where the later write wins, and their
    own place keeps FILL).  None / None is the correct kernel."""
    pe, fe, n = pl.period_elems, pl.frame_elems, pl.T * pl.frame_elems
    W = n if (wrap_bytes is None and wrap_elems is None) else (wrap_elems if wrap_elems is not None else wrap_bytes // pl.itemsize)
    inside = (torch.arange(pl.P, dtype=torch.int64)[:, None] * fe + sample_positions(pl)[None, :]).reshape(-1)
    fill = torch.full((inside.numel(),), FILL, dtype=block_bits.dtype)
    out = []
    for k in periods:
        i = k * pe + inside
        if side == "read":
            out.append(block_bits[(i % W) % pe])
        else:
            # element i is written by the LAST j with j mod W == i, j < n; places >= W are never written
            last = i + ((n - 1 - i) // W) * W
            out.append(torch.where(i < W, block_bits[last % pe], fill))
    return torch.stack(out).view(len(periods) * pl.P, -1)


def detected(pl: Plan, out_sel: torch.Tensor, block_bits: torch.Tensor, periods: Sequence[int]) -> Optional[str]:
    """What the two checks (periodicity, period 0 against its reference) say about the selected periods of an emulated output: "periodicity", "period 0" or None
    (nothing noticed).  periods[0] must be 0."""
    assert periods[0] == 0
    if first_aperiodic(out_sel, pl.P) is not None:
        return "periodicity"
    if not torch.equal(out_sel[:pl.P], block_bits.view(pl.P, pl.frame_elems)[:, sample_positions(pl)]):
        return "period 0"
    return None


def periods_to_look_at(pl: Plan) -> List[int]:
    """Period 0, and for every boundary the tensor passes the period that holds it and the next one."""
    ks = {0}
    for f in pl.boundary_frames.values():
        ks.update(k for k in (f // pl.P, f // pl.P + 1) if k < pl.periods)
    return sorted(ks)
