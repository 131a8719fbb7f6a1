// The attention of IP-Adapter Plus's perceiver Resampler (models/embeddings.py IPAdapterPlusImageProjection) on gfx950: for every
// (batch b, head h)
//   out[b, :, h] = softmax(scale q[b, :, h] . [K0[b]; K1[b]]^T) [V0[b]; V1[b]]
// with at most 16 queries (the learned latents), keys and values from TWO token-major matrices of different length (S0 normalised
// image tokens -- 257 for ViT-H -- then the S1 <= 16 normalised latents), bf16 in / bf16 out, D = 64.
//
// Call site: ip_adapter.Resampler, four times per image prompt.  q / out are [B*Nq][ld] token matrices, head h at columns h D ..
// h D + D; k0 / v0 are [B*S0_alloc][ld] and k1 / v1 [B*S1_alloc][ld], in practice the two column halves of the stacked to_k | to_v
// projection applied once to the image rows and once to the latent rows.  Every operand has its own row stride.  Nothing is
// concatenated, padded or transposed on the way in: the flash kernel would need a torch.cat, a zero-padded Skv_alloc and a V-transpose
// launch per layer, and its 128-query block would be one eighth full.
//
// Work split.  One workgroup of kNW = 4 waves per (batch, head); grid = B H (24 .. 40 workgroups at the published sizes -- a
// latency case: what counts is the length of one workgroup's serial chain, so the parallel axis inside it is the KEYS).  The virtual
// key sequence is cut into 32-key blocks that never straddle the two sources: source 0 is ceil(S0 / 32) blocks, the last one partial,
// source 1 is one block.  Wave w takes blocks w, w + 4, ...: at S0 = 257, S1 = 16 that is 10 blocks, 3 / 3 / 2 / 2 per wave instead of
// 10 in a row.  Every wave keeps its own online-softmax triple (m, l, O); the four meet in LDS at the end.
//
// The swapped products on v_mfma_f32_16x16x32_bf16 (lane = (c = lane & 15, g = lane >> 4)):
//   S^T[kv][q] = K[kv][:] . Q[q][:]^T      A = K straight from global memory (lane (c, g): the 16 bytes d = 32 ks + 8 g .. + 7 of key
//                                          16 t + c, t = 0, 1 the two 16-key tiles of a block), B = Q: lane (q, g) holds the same
//                                          columns of query q for the kernel's life (two k-steps, 8 registers).
//   O^T[d][q]  = V^T[d][kv] . P^T[kv][q]   A = V^T through LDS, B = P^T: the S^T accumulators as they are.
// Lane (q, g) ends the first product with the 8 keys 16 t + 4 g + r (r = 0 .. 3) of ITS query: row maximum and row sum are in-lane
// plus two exchanges (lanes ^ 16, ^ 32).  Packed in the order e = 4 t + r these are the B fragment of the ONE k-step of the second
// product with B's k index 8 g + e; the second product may take its keys in any order as long as V^T uses the same one, so V^T is
// stored at pos(16 t + 4 g + r) = 8 g + 4 t + r and a V^T fragment is one 16-byte LDS read.  Four 16-row output tiles: a 16 x 64 fp32
// accumulator of 16 registers per wave, lane (q, g) holding O[q][16 dt + 4 g + r].
//
// V^T through LDS (wave-private, so no barrier): tokens on adjacent lanes, four 16-byte global loads per lane and block, each
// scattered as eight 2-byte writes into vt[d][pos(token)], rows kLdv = 40 elements (80 bytes) apart as in attention_temporal.hip
// (64 x 80 = 5 KiB per wave).  Every global load is unconditional with a clamped row (keys at or past the source's valid count read its
// last valid row; queries >= Nq read query Nq - 1 and are never stored); V^T of such keys is made zero with a select on the loaded
// value (P is zero there, and 0 x stale bits must not make a NaN), their scores are set to -inf with a select before the maximum.
// Rows [S, S_alloc) of a batch are never touched.
//
// Arithmetic: scores in fp32; per block m' = max(m, block maximum), alpha = exp2(m - m') (0 on the first block: m starts at -inf and
// every block has a valid key, so m' is finite); p = exp2(s scale log2 e - m'); P is rounded to bf16 ONCE and the row sum is taken
// from the ROUNDED values (the convention of the temporal and IP kernels); O = alpha O + P V on the matrix pipe.  Merge: the waves
// write (m, l, O) to LDS, one barrier, then wave w owns output columns 16 w .. + 15: M = max_j m_j, then l and O are summed with the
// weights exp2(m_j - M) IN WAVE ORDER 0, 1, 2, 3, so the result depends on the inputs alone.  A wave that owned no block has
// m = -inf, l = 0, O = 0: its weight is exp2(-inf) = 0 and 0 x 0 adds nothing (wave 0 always owns block 0, so M is finite).  out =
// O / l rounded to bf16 once, stored as 16-byte pieces inside columns [h D, h D + D) of rows that exist.  With one valid key in
// total P = l = 1 and the result is that V row to the bit.  LDS: 4 x 5 KiB of V^T + 4 x (4 KiB + 128 B) of partials = 36.5 KiB.
#include "common.cuh"

namespace da_attn_resampler {

constexpr int kNW = 4;     // waves per workgroup: the key blocks are dealt round-robin
constexpr int kD = 64;     // head size of every published Resampler
constexpr int kNq = 16;    // one query tile
constexpr int kBlk = 32;   // keys per block
constexpr int kLdv = 40;   // elements per V^T row in LDS: 32 keys + 8 (16-byte fragment reads spread over the banks)

// position of key kv of a block inside a V^T row: (t, g, r) = (bit 4, bits 3:2, bits 1:0) -> 8 g + 4 t + r
__device__ __forceinline__ int pos(int kv) { return ((kv & 0xc) << 1) | ((kv & 0x10) >> 2) | (kv & 3); }

__global__ __launch_bounds__(64 * kNW) void attn_resampler_kernel(const da_attention_resampler_params p) {
#if defined(__HIP_DEVICE_COMPILE__)
  __shared__ __attribute__((aligned(16))) uint16_t vsm[kNW * kD * kLdv];
  __shared__ __attribute__((aligned(16))) float osm[kNW * kNq * kD];
  __shared__ float msm[kNW * kNq], lsm[kNW * kNq];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  uint16_t* const vt = vsm + wave * (kD * kLdv);

  const int b = blockIdx.x / p.H, h = blockIdx.x - b * p.H;
  const int S0 = p.S0, S1 = p.S1;
  const int nb0 = (S0 + kBlk - 1) / kBlk, nb = nb0 + (S1 > 0 ? 1 : 0);
  const float sl2 = p.scale * 1.4426950408889634f;

  bf16x8_t qf[2];
  {
    const size_t qrow = (size_t)b * p.Nq + (c < p.Nq ? c : p.Nq - 1);     // clamped: a query past the end is a copy, never stored
    const uint16_t* __restrict__ qp = (const uint16_t*)p.q + qrow * p.q_row_stride + h * kD + 8 * g;
    qf[0] = __builtin_bit_cast(bf16x8_t, *(const uint4*)qp);
    qf[1] = __builtin_bit_cast(bf16x8_t, *(const uint4*)(qp + 32));
  }
  f32x4_t o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;

  for (int blk = wave; blk < nb; blk += kNW) {          // wave-uniform
    const bool src0 = blk < nb0;
    const int key0 = src0 ? blk * kBlk : 0;
    const int valid = (src0 ? S0 : S1) - key0;          // >= 1 keys of this block exist (may exceed 32)
    const size_t tok0 = src0 ? (size_t)b * p.S0_alloc + key0 : (size_t)b * p.S1_alloc;
    const int kld = src0 ? p.k0_row_stride : p.k1_row_stride, vld = src0 ? p.v0_row_stride : p.v1_row_stride;
    const uint16_t* __restrict__ kg = (const uint16_t*)(src0 ? p.k0 : p.k1) + tok0 * kld + h * kD;
    const uint16_t* __restrict__ vg = (const uint16_t*)(src0 ? p.v0 : p.v1) + tok0 * vld + h * kD;
    const int last = valid - 1;

    // ---- loads: K fragments (2 tiles x 2 k-steps) and this lane's four V chunks ----
    uint4 kf[2][2], vf[4];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int key = 16 * t + c;
      const uint16_t* kp = kg + (size_t)(key < valid ? key : last) * kld + 8 * g;
      kf[t][0] = *(const uint4*)kp;
      kf[t][1] = *(const uint4*)(kp + 32);
    }
    const int tok = lane & 31, ch0 = lane >> 5;         // chunks ch0, ch0 + 2, ch0 + 4, ch0 + 6 of token `tok`
    const bool live = tok < valid;
    {
      const uint16_t* vp = vg + (size_t)(live ? tok : last) * vld + 8 * ch0;
#pragma unroll
      for (int j = 0; j < 4; ++j) vf[j] = *(const uint4*)(vp + 16 * j);
    }

    // ---- S^T = K Q^T ----
    f32x4_t s[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      s[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, kf[t][ks]), qf[ks], s[t], 0, 0, 0);
    }

    // ---- V -> V^T in LDS (the previous block's fragment reads were waited for at the end of its iteration) ----
    {
      const int vp = pos(tok);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t w[4] = {live ? vf[j].x : 0u, live ? vf[j].y : 0u, live ? vf[j].z : 0u, live ? vf[j].w : 0u};
        const int d0 = 8 * (ch0 + 2 * j);
#pragma unroll
        for (int e = 0; e < 8; ++e) vt[(d0 + e) * kLdv + vp] = (uint16_t)(w[e >> 1] >> (16 * (e & 1)));
      }
    }

    // ---- online softmax over the 8 keys of this lane's query and the 24 of lanes ^ 16, ^ 32, ^ 48 ----
    float sc[8];
    float mb = -INFINITY;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int kv = 16 * (e >> 2) + 4 * g + (e & 3);
      sc[e] = kv < valid ? s[e >> 2][e & 3] * sl2 : -INFINITY;
      mb = fmaxf(mb, sc[e]);
    }
    mb = fmaxf(mb, __shfl_xor(mb, 16, 64));
    mb = fmaxf(mb, __shfl_xor(mb, 32, 64));             // finite: key 0 of a block is never masked
    const float mn = fmaxf(m, mb);
    const float alpha = __builtin_amdgcn_exp2f(m - mn); // first block: exp2(-inf) = 0 on l = 0, O = 0
    m = mn;
    uint32_t pk[4];
    float lb = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      pk[i] = pack_bf2(__builtin_amdgcn_exp2f(sc[2 * i] - mn), __builtin_amdgcn_exp2f(sc[2 * i + 1] - mn));
      lb += bf_lo(pk[i]) + bf_hi(pk[i]);                // the sum of the ROUNDED probabilities
    }
    lb += __shfl_xor(lb, 16, 64);
    lb += __shfl_xor(lb, 32, 64);
    l = l * alpha + lb;
    const bf16x8_t pf = __builtin_bit_cast(bf16x8_t, make_uint4(pk[0], pk[1], pk[2], pk[3]));

    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's V^T writes have landed (wave-private region: no barrier)

    // ---- O^T = alpha O^T + V^T P^T ----
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const uint4 a = *(const uint4*)(vt + (16 * dt + c) * kLdv + 8 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
      o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), pf, o[dt], 0, 0, 0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // fragment reads done before the next block overwrites V^T
  }

  // ---- the four partial triples meet in LDS.  Lane (q, g): o[dt][r] = O[q][16 dt + 4 g + r] ----
  {
    float* om = osm + (wave * kNq + c) * kD + 4 * g;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) *(f32x4_t*)(om + 16 * dt) = o[dt];
    if (g == 0) msm[wave * kNq + c] = m, lsm[wave * kNq + c] = l;
  }
  __syncthreads();

  // ---- wave w: columns 16 w .. + 15, lane -> (query, 8-column piece); merged in wave order, normalised, rounded once ----
  if (lane < 2 * kNq) {
    const int q = lane >> 1, col = 16 * wave + 8 * (lane & 1);
    float M = msm[q];
#pragma unroll
    for (int j = 1; j < kNW; ++j) M = fmaxf(M, msm[j * kNq + q]);
    float L = 0.f, f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = 0.f;
#pragma unroll
    for (int j = 0; j < kNW; ++j) {
      const float wgt = __builtin_amdgcn_exp2f(msm[j * kNq + q] - M);   // a wave without a block: exp2(-inf) = 0
      L += wgt * lsm[j * kNq + q];
      const float* oj = osm + (j * kNq + q) * kD + col;
      const f32x4_t x = *(const f32x4_t*)oj, y = *(const f32x4_t*)(oj + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) f[e] += wgt * x[e], f[4 + e] += wgt * y[e];
    }
    const float inv = 1.0f / L;                         // L >= 1: the maximum's own term
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] *= inv;
    if (q < p.Nq) {
      uint16_t* op = (uint16_t*)p.out + ((size_t)b * p.Nq + q) * p.o_row_stride + h * kD + col;
      *(uint4*)op = pack8(f);
    }
  }
#endif  // __HIP_DEVICE_COMPILE__
}

}  // namespace da_attn_resampler

extern "C" int da_attention_resampler_bf16(const da_attention_resampler_params* p, void* stream) {
  using namespace da_attn_resampler;
  if (!p || !p->q || !p->out || !p->k0 || !p->v0) return DA_ERR_INVALID;
  if (p->S1 > 0 && (!p->k1 || !p->v1)) return DA_ERR_INVALID;
  if (p->D != kD || p->Nq < 1 || p->Nq > kNq || p->S1 < 0 || p->S1 > 16 || p->S0 < 1) return DA_ERR_UNSUPPORTED;
  if (p->B < 1 || p->H < 1 || p->S0_alloc < p->S0 || (p->S1 > 0 && p->S1_alloc < p->S1)) return DA_ERR_UNSUPPORTED;
  if (!(p->scale == p->scale)) return DA_ERR_UNSUPPORTED;
  const long long width = (long long)p->H * p->D, grid = (long long)p->B * p->H;
  if (grid > 0x7fffffffLL || (long long)p->B * p->S0_alloc > 0x7fffffffLL || (long long)p->B * p->S1_alloc > 0x7fffffffLL)
    return DA_ERR_UNSUPPORTED;
  const int lds[6] = {p->q_row_stride, p->o_row_stride, p->k0_row_stride, p->v0_row_stride, p->k1_row_stride, p->v1_row_stride};
  const void* ptrs[6] = {p->q, p->out, p->k0, p->v0, p->k1, p->v1};
  for (int i = 0; i < (p->S1 > 0 ? 6 : 4); ++i)   // 16-byte loads and stores: rows of whole 8-element chunks from a 16-byte aligned base
    if (lds[i] < width || (lds[i] & 7) || ((uintptr_t)ptrs[i] & 15)) return DA_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  DA_LAUNCH(attn_resampler_kernel, dim3((unsigned)grid), dim3(64 * kNW), 0, s, *p);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
