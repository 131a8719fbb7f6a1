// Self-attention over the FRAME axis of a frame-major channels-last token matrix on gfx950: F <= 32 tokens per sequence, D = 40 / 80 /
// 160 (C / 8 of the SD 1.5 U-Net levels), bf16 in / bf16 out, in place on the layout the rest of the engine keeps.
//
// Call site: the two self-attentions of an AnimateDiff motion module (unet_motion_model.py AnimateDiffTransformer3D /
// TransformerTemporalModel -> BasicTransformerBlock with double_self_attention), where the reference permutes the activation to
// (B HW, F, C) and back around every attention.  Here element (b, f, p, h, d) of an operand is at
//   ptr + ((b F + f) HW + p) row_stride + h D + d
// so q, k, v may be the three column blocks of one fused projection output and `out` a column block of a wider buffer; a sequence's
// tokens are HW rows apart and nothing is copied.  V is read token-major: there is no transposed operand and no key padding.
//
// Work split.  ONE WAVE owns one (pixel, head) sequence from its loads to its stores.  All F <= 32 keys fit one 32 x 32 MFMA tile:
// there is no key loop, no running maximum, no rescale and no ring.  A workgroup is kNW = 4 waves and covers the heads of ONE pixel
// (one row of the token matrix per frame): a wave walks heads wave, wave + 4, ...  A pixel's eight heads are 640 contiguous bytes per
// frame (five whole 128-byte lines) at C = 320 and more at the wider levels, so a longer run of pixels buys no better lines, and it
// costs the small levels their parallelism: with four pixels per workgroup (a wave then walks eight sequences in a row, and B = 2,
// HW = 64 is 32 workgroups for 256 CUs) the four shapes of profiles/temporal_attention_numbers.md took 163 / 56 / 54 / 51 us against
// 160 / 56 / 31 / 18 us with one.  The level-0 shape of an SD 1.5 step (B = 2, HW = 4096, C = 320) is 8192 workgroups, 32 per CU.
//
// The swapped products of attention2.hip on v_mfma_f32_32x32x16_bf16 (lane = (c = lane & 31, hi = lane >> 5)):
//
//   S^T[kv][q] = K[kv][:] . Q[q][:]^T      A = K, B = Q, both straight from global memory: lane (c, hi) loads the 16 bytes
//                                          d = 16 ks + 8 hi .. + 7 of token c.  Tokens >= F and the chunk past D (D = 40: ks = 2,
//                                          hi = 1) are zeros made in registers, never read.
//   O^T[d][q]  = V^T[d][kv] . P^T[kv][q]   A = V^T through LDS (below), B = P^T: the S^T accumulators as they are.
//
// Lane (q, hi) ends the first product with the 16 keys kv(r) = 8 (r >> 2) + 4 hi + (r & 3) of ITS query: the row maximum and the row
// sum are in-lane plus one exchange with lane q + 32.  Registers 8 ks .. 8 ks + 7 are the B fragment of k-step ks of the second
// product in the key order kv(8 ks + e); the second product may take its keys in any order as long as V^T uses the same one, so V^T
// is stored with bits 2 and 3 of the key index swapped (pos()) and a V^T fragment is one 16-byte LDS read.  With F <= 16 the second
// k-step holds masked keys only and is skipped (wave-uniform).  A 16 x 16 x 32 variant for F <= 16 is not built: the kernel moves
// 8 F D bytes per sequence for 4 F^2 D flops and is bound by how it streams memory, not by the matrix pipe.
//
// V^T through LDS (the only LDS use; wave-private, so no barrier): a lane scatters the 8 values of each 16-byte chunk of its token's V
// row as 2-byte writes into vt[d][pos(token)], rows kLdv = 40 elements (80 bytes) apart.  The pad is for the 16-byte fragment reads:
// lanes d = 0 .. 7 start at 0, 80, 32, 112, 64, 16, 96, 48 (mod 128), so every group of eight lanes covers all 32 banks once; it is the
// same for the three widths because the pitch runs along the keys, D only sets the number of rows (D 80 bytes per wave: 3.1 / 6.3 /
// 12.5 KiB).  Tokens in [F, 16 or 32) are written as zeros: P is zero there, and 0 x stale bits must not make a NaN.
//
// Arithmetic: scores in fp32, keys >= F set to -inf before the maximum; p = exp2(s scale log2 e - m) in fp32; P is rounded to bf16
// ONCE and the row sum is the sum of the ROUNDED values (the "RSM" convention of attention2.hip, algo 4: numerator and denominator
// see the same P; attention.hip itself sums the unrounded P); O = (P V) / l rounded to bf16 once.  Query columns >= F compute on zeros
// and are never stored.  Stores are 16 bytes per lane (the two halves of a query exchange 8-byte pieces first), only inside columns
// [h D, h D + D) of rows that exist.  No workspace, nothing shared between workgroups; the result depends on the inputs alone.
#include "common.cuh"

namespace da_attn_temporal {

constexpr int kNW = 4;     // waves per workgroup
constexpr int kLdv = 40;   // elements per V^T row in LDS: 32 keys + 8 (see above)

// position of key kv inside a V^T row: bits 2 and 3 swapped, so that the keys of lane half `hi` in k-step ks are 16 ks + 8 hi .. + 7
__device__ __forceinline__ int pos(int kv) { return (kv & 0x13) | ((kv & 8) >> 1) | ((kv & 4) << 1); }

template <int D>
__global__ __launch_bounds__(64 * kNW) void attn_temporal_kernel(const da_attention_temporal_params p) {
#if defined(__HIP_DEVICE_COMPILE__)
  static_assert(D == 40 || D == 80 || D == 160, "head sizes of the temporal kernel");
  constexpr int NKS = (D + 15) / 16;   // k-steps of the first product
  constexpr int NDT = (D + 31) / 32;   // 32-row output tiles of the second
  __shared__ __attribute__((aligned(16))) uint16_t smem[kNW * D * kLdv];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 31, hi = lane >> 5;
  uint16_t* vt = smem + wave * (D * kLdv);

  const int F = p.F, H = p.H;
  const int b = blockIdx.x / p.HW, pix = blockIdx.x - b * p.HW;
  const int fw = F <= 16 ? 16 : 32;                  // keys the second product walks
  const bool tok = c < F;
  const size_t row0 = ((size_t)b * F + (tok ? c : 0)) * p.HW + pix;   // token c of this pixel (tokens >= F: never dereferenced)
  const float sl2 = p.scale * 1.4426950408889634f;
  const int vpos = pos(c);

  for (int h = wave; h < H; h += kNW) {              // wave-uniform
    const uint16_t* __restrict__ qp = (const uint16_t*)p.q + row0 * p.q_row_stride + h * D + 8 * hi;
    const uint16_t* __restrict__ kp = (const uint16_t*)p.k + row0 * p.k_row_stride + h * D + 8 * hi;
    const uint16_t* __restrict__ vp = (const uint16_t*)p.v + row0 * p.v_row_stride + h * D + 8 * hi;

    uint4 qf[NKS], kf[NKS], vf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const bool ok = tok && (16 * ks + 8 * hi < D);
      const uint4 z = make_uint4(0, 0, 0, 0);
      qf[ks] = ok ? *(const uint4*)(qp + 16 * ks) : z;
      kf[ks] = ok ? *(const uint4*)(kp + 16 * ks) : z;
      vf[ks] = ok ? *(const uint4*)(vp + 16 * ks) : z;
    }

    // ---- S^T = K Q^T ----
    f32x16_t sacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
      sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, kf[ks]), __builtin_bit_cast(bf16x8_t, qf[ks]), sacc, 0, 0, 0);

    // ---- V -> V^T in LDS (the previous sequence's fragment reads were waited for before its stores) ----
    if (c < fw) {
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        const int d0 = 16 * ks + 8 * hi;
        if (d0 < D) {
          const uint32_t w[4] = {vf[ks].x, vf[ks].y, vf[ks].z, vf[ks].w};
#pragma unroll
          for (int j = 0; j < 8; ++j) vt[(d0 + j) * kLdv + vpos] = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
        }
      }
    }

    // ---- softmax over the keys of this lane's query: 16 in-lane, 16 in lane ^ 32 ----
    float sc[16];
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kv = 8 * (r >> 2) + 4 * hi + (r & 3);
      sc[r] = kv < F ? sacc[r] * sl2 : -INFINITY;
      m = fmaxf(m, sc[r]);
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));             // finite: key 0 is never masked
    uint32_t pk[8];
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      pk[i] = pack_bf2(__builtin_amdgcn_exp2f(sc[2 * i] - m), __builtin_amdgcn_exp2f(sc[2 * i + 1] - m));
      l += bf_lo(pk[i]) + bf_hi(pk[i]);              // the sum of the ROUNDED probabilities
    }
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;                      // l >= 1: the maximum's own term
    const bf16x8_t pf0 = __builtin_bit_cast(bf16x8_t, make_uint4(pk[0], pk[1], pk[2], pk[3]));
    const bf16x8_t pf1 = __builtin_bit_cast(bf16x8_t, make_uint4(pk[4], pk[5], pk[6], pk[7]));

    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's V^T writes have landed (wave-private region: no barrier)

    // ---- O^T = V^T P^T, normalise, store ----
    const bool qok = c < F;
    uint16_t* __restrict__ op = (uint16_t*)p.out + row0 * p.o_row_stride + h * D;   // (row0 is query c's row for c < F)
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      const int d = 32 * dt + c;                     // A row of this lane
      const bool dok = d < D;
      const uint16_t* vrow = vt + (dok ? d : 0) * kLdv + 8 * hi;
      f32x16_t o;
#pragma unroll
      for (int r = 0; r < 16; ++r) o[r] = 0.f;
      uint4 a0 = *(const uint4*)vrow;
      if (!dok) a0 = make_uint4(0, 0, 0, 0);
      o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a0), pf0, o, 0, 0, 0);
      if (fw == 32) {
        uint4 a1 = *(const uint4*)(vrow + 16);
        if (!dok) a1 = make_uint4(0, 0, 0, 0);
        o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a1), pf1, o, 0, 0, 0);
      }
      // lane (q, hi): o[4 g + e] = O[q][32 dt + 8 g + 4 hi + e].  Halves trade 8-byte pieces: hi = 0 ends with 16 j .. + 7, hi = 1
      // with 16 j + 8 .. + 15 of the tile.
      uint2 pc[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        pc[g].x = pack_bf2(o[4 * g] * inv, o[4 * g + 1] * inv);
        pc[g].y = pack_bf2(o[4 * g + 2] * inv, o[4 * g + 3] * inv);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const uint2 own = hi ? pc[2 * j + 1] : pc[2 * j];
        const uint2 send = hi ? pc[2 * j] : pc[2 * j + 1];
        uint2 recv;
        recv.x = (uint32_t)__shfl_xor((int)send.x, 32, 64);
        recv.y = (uint32_t)__shfl_xor((int)send.y, 32, 64);
        const uint4 val = hi ? make_uint4(recv.x, recv.y, own.x, own.y) : make_uint4(own.x, own.y, recv.x, recv.y);
        const int d0 = 32 * dt + 16 * j + 8 * hi;
        if (qok && d0 < D) *(uint4*)(op + d0) = val;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // fragment reads done before the next sequence overwrites V^T
  }
#endif  // __HIP_DEVICE_COMPILE__
}

template <int D>
int launch(const da_attention_temporal_params& p, hipStream_t s) {
  const long long grid = (long long)p.B * p.HW;
  if (grid > 0x7fffffffLL) return DA_ERR_UNSUPPORTED;
  DA_LAUNCH(attn_temporal_kernel<D>, dim3((unsigned)grid), dim3(64 * kNW), 0, s, p);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

}  // namespace da_attn_temporal

extern "C" int da_attention_temporal_bf16(const da_attention_temporal_params* p, void* stream) {
  if (!p || !p->q || !p->k || !p->v || !p->out) return DA_ERR_INVALID;
  if (p->F < 1 || p->F > 32 || p->B < 1 || p->HW < 1 || p->H < 1) return DA_ERR_UNSUPPORTED;
  if (p->D != 40 && p->D != 80 && p->D != 160) return DA_ERR_UNSUPPORTED;
  if (!(p->scale == p->scale)) return DA_ERR_UNSUPPORTED;
  const long long width = (long long)p->H * p->D;
  const int lds[4] = {p->q_row_stride, p->k_row_stride, p->v_row_stride, p->o_row_stride};
  const void* ptrs[4] = {p->q, p->k, p->v, p->out};
  for (int i = 0; i < 4; ++i)   // 16-byte loads and stores: rows of whole 8-element chunks from a 16-byte aligned base
    if (lds[i] < width || (lds[i] & 7) || ((uintptr_t)ptrs[i] & 15)) return DA_ERR_UNSUPPORTED;
  if ((long long)p->B * p->F * p->HW > 0x7fffffffLL) return DA_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  switch (p->D) {
    case 40: return da_attn_temporal::launch<40>(*p, s);
    case 80: return da_attn_temporal::launch<80>(*p, s);
    case 160: return da_attn_temporal::launch<160>(*p, s);
  }
  return DA_ERR_UNSUPPORTED;
}
