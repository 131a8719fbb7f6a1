// FP8 (OCP e4m3) flash attention for D = 128 on gfx950, with the prepare kernel in front of it.  Opt-in
// (WanTransformer3DModel / FluxTransformer2DModel.enable_fp8_attention); nothing else calls them.  Unmasked, no bias.
//
// (a) da_attention_fp8_prepare: one launch from the layout both models produce -- qk [B*S][2C] bf16 (q in columns 0 .. C, k in
//     C .. 2C, after RMSNorm + RoPE) and vt [C][B*S] bf16 (keys contiguous, batch b at column b*S) -- to
//       q8, k8 e4m3 [B*S][C]  and  sq, sk fp32 [B*S][H]: one scale per (token, head), the arithmetic of da_quantize_rows_e4m3 on rows
//         of 128:  amax = max|x|;  scale = amax / 448 (1 when amax == 0);  inv = 1 / scale;  q = e4m3_rne(min(max(x * inv, -448), 448))
//       vt8 e4m3 [C][B*S8]    and  sv fp32 [B][C]: one scale per (batch, channel), amax over the S keys of that batch, same arithmetic;
//         S8 = S rounded up to a multiple of 128, bytes [S, S8) of every batch segment are written as zero.
//     The first ceil(B*S*2H / 16) workgroups give 16 lanes to each (token, head) row of q|k (one 16-byte load and one 8-byte store per
//     lane, amax by four xor-shuffles); the other C*B workgroups take one (channel, batch) row of V^T each (256 threads, two passes,
//     16-byte loads where the row is 16-byte aligned and single bf16 loads where it is not: S need not be a multiple of anything).
//
// (b) da_attention_fp8.  The numeric contract, per (batch, head), i a query, j a key, d a channel of the head:
//       s_ij = scale * sq_i * sk_j * sum_d q8_id k8_jd                    fp32 accumulation on the fp8 MFMA
//       x_ij = s_ij * log2(e);   m_i = running maximum of x_ij over the keys seen so far (NOT deferred: updated at every key tile)
//       p_ij = exp2(x_ij - m_i + 8)  <= 2^8, rounded to e4m3 (p8).  The shift 2^8 keeps probabilities down to 2^-17 of the row's
//              maximum out of e4m3's flush range (the smallest subnormal is 2^-9); 2^8 (1 + 2^-20) < 448, so the conversion never clamps.
//       l_i  = sum_j p8_ij    the sum of the ROUNDED values (on the matrix pipe, against a row of ones), so that the rounding bias
//              cancels in the normalisation.  Keys [Skv, 128 ceil(Skv / 128)) are masked to -inf: they enter neither m nor l.
//       o_id = bf16(sv_d * (sum_j p8_ij v8_jd) / l_i)                      fp32 accumulation, ONE rounding
//     When a later tile raises m_i, the accumulators and l_i are multiplied by exp2(m_old - m_new) (skipped when no row of the wave
//     moved), so earlier keys were rounded on a finer grid than the contract's, never a coarser one.
//
// Instruction: v_mfma_f32_16x16x128_f8f6f4, both formats e4m3, no block scales (see gemm_fp8.hip for the fragment layout: lane 16 g + c
// holds row c and K bytes 32 g .. 32 g + 31 of either source, the accumulator holds [4 g + r][c] of (first rows) x (second rows)).
// Work split: a workgroup of 4 waves owns 128 queries of one (batch, head), a wave 32 of them (two 16-query fragments Q_0, Q_1, read
// from global memory once and kept in 16 VGPRs).  Keys go by in tiles of 128.  Per tile and wave:
//   S^T = K Q^T: eight MFMAs per query fragment, MFMA t with the K rows {32 a + 4 t + b : a, b = 0 .. 3} as its FIRST source (row
//     4 a + b).  Lane (c, g) then holds, for its query c, the scores of keys 32 g + 4 t + r (t = 0 .. 7, r = 0 .. 3): 32 CONSECUTIVE keys.
//   softmax in registers: the row maximum is the lane's 32 values and two xor-shuffles (lanes 16, 32 apart hold the other keys).
//   P: v_cvt_pk_fp8_f32 packs the lane's 32 values into 8 VGPRs in key order -- which IS the second-source fragment of a 16 x 128 tile
//     whose K bytes 32 g .. 32 g + 31 are keys 32 g .. 32 g + 31, the plain map.  P never touches LDS.
//   O^T += V^T P^T: per 16-channel tile one fragment of the V^T tile (first source, the plain map over keys) and one MFMA per query
//     fragment; one more MFMA per query fragment against a constant fragment of e4m3 ones gives l.  34 MFMAs per tile and wave.
//   The accumulator of O^T holds channels 4 g .. 4 g + 3 of query c: four adjacent bf16, one 8-byte store per 16-channel tile.
// LDS: a ring of 2 stages of 32 KiB (K tile 128 x 128 bytes, then V^T tile 128 x 128 bytes) filled by LDS-DMA (buffer_load ... lds,
// 16 bytes per lane), plus 2 x 128 floats of sk: 65 KiB, two workgroups per CU (<= 256 VGPRs).  The K tile is stored with its rows
// PERMUTED -- LDS row 16 t + 4 a + b holds key 32 a + 4 t + b -- so that both tiles are read by the same fragment() with the same
// XOR swizzle as gemm_fp8.hip (chunk j of LDS row r at slot j ^ ((r >> 1) & 7), applied on the DMA's source address).  Per tile: wait
// for my loads (vmcnt 0: they had a whole tile of arithmetic to land), publish my sk value, ONE barrier, issue the next tile's
// loads into the other stage, compute.  The other workgroup of the CU covers the wait.
// Bounds: K rows past Skv are clamped to key Skv - 1 when staged (and the descriptor ends at that key's last byte) and their scores
// are masked; V^T tiles are whole by the S8 padding; query rows past Sq are clamped when loaded and never stored.
#include "common.cuh"
#include <type_traits>

namespace da_attention_fp8_ns {

typedef __attribute__((ext_vector_type(8))) int i32x8_t;
typedef __attribute__((ext_vector_type(4))) int i32x4_t;

constexpr int D = 128;            // head size = bytes of one K row = one MFMA's K
constexpr int BQ = 128, BK = 128; // queries per workgroup, keys per tile
constexpr int TILE = BK * D;      // bytes of a K tile and of a V^T tile
constexpr int STAGE = 2 * TILE;
constexpr int LDS_BYTES = 2 * STAGE + 2 * BK * 4;
constexpr int LOADS = 4;          // 8-row DMA pieces per wave, tile and operand
constexpr float LOG2E = 1.4426950408889634f;
constexpr float P_SHIFT = 8.0f;
#define AF8_LDS(ptr) ((__attribute__((address_space(3))) void*)(ptr))
#define AF8_FENCE() __builtin_amdgcn_sched_barrier(0)

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* base, long long bytes) {
  const uint64_t v = (uint64_t)base;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  const int n = __builtin_amdgcn_readfirstlane((int)(bytes > 0x7fffffffLL ? 0x7fffffffLL : bytes));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), 0, n, 0x00020000);
}

// LDS row c of a 16-row tile at `tile` (128-byte rows), bytes 32 g .. 32 g + 31: chunks 2 g and 2 g + 1 through the swizzle
__device__ __forceinline__ i32x8_t fragment(const unsigned char* tile, int c, int g) {
  const int sw = (c >> 1) & 7;
  const i32x4_t lo = *(const i32x4_t*)(tile + c * 128 + (((2 * g) ^ sw) << 4));
  const i32x4_t hi = *(const i32x4_t*)(tile + c * 128 + (((2 * g + 1) ^ sw) << 4));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

__global__ __launch_bounds__(256, 2) void attention_fp8_kernel(const da_attention_fp8_params p) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = threadIdx.x;
  const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int c = lane & 15, g = lane >> 4;

  const int qtiles = (p.Sq + BQ - 1) / BQ;
  const int bh = (int)blockIdx.x / qtiles, qt = (int)blockIdx.x - bh * qtiles;
  const int b = bh / p.H, h = bh - b * p.H;
  const int nk = (p.Skv + BK - 1) / BK;

  const unsigned char* Kb = (const unsigned char*)p.k8 + (size_t)b * p.k_batch_stride + h * D;
  const unsigned char* Vb = (const unsigned char*)p.vt8 + (size_t)h * D * p.vt_ld + (size_t)b * p.vt_batch_stride;
  __amdgpu_buffer_rsrc_t rs_k = rsrc(Kb, (long long)(p.Skv - 1) * p.k_row_stride + D);
  __amdgpu_buffer_rsrc_t rs_v = rsrc(Vb, (long long)(D - 1) * p.vt_ld + (long long)nk * BK);
  const float* skb = (const float*)p.sk + (size_t)b * p.sk_batch_stride + h;

  // staging: wave w sends the 8-row pieces w, w + 4, w + 8, w + 12 of either tile; lane -> LDS row 8 piece + (lane >> 3), slot lane & 7
  int key_k[LOADS], ch_k[LOADS], vo_v[LOADS];
#pragma unroll
  for (int i = 0; i < LOADS; ++i) {
    const int R = 8 * (wave + 4 * i) + (lane >> 3);
    ch_k[i] = ((lane & 7) ^ ((R >> 1) & 7)) << 4;
    key_k[i] = 32 * ((R >> 2) & 3) + 4 * (R >> 4) + (R & 3);                   // the K tile's row permutation
    vo_v[i] = R * (int)p.vt_ld + ch_k[i];
  }
  auto stage = [&](int slot, int kt) {
    unsigned char* dst = smem + slot * STAGE + wave * 1024;
#pragma unroll
    for (int i = 0; i < LOADS; ++i)                                            // keys past Skv: the last key again (masked later)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_k, AF8_LDS(dst + i * 4096), 16, min(kt * BK + key_k[i], p.Skv - 1) * p.k_row_stride + ch_k[i],
                                               0, 0, 0);
#pragma unroll
    for (int i = 0; i < LOADS; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_v, AF8_LDS(dst + TILE + i * 4096), 16, vo_v[i], kt * BK, 0, 0);
  };
  auto load_sk = [&](int kt) {                                                 // threads 0 .. 127: the scale of key 128 kt + t
    const int key = min(kt * BK + (t & (BK - 1)), p.Skv - 1);
    return skb[(size_t)key * p.H];
  };

  // Q fragments and the per-query constant sq_i * scale * log2(e)
  i32x8_t qf[2];
  float cq[2];
  int qrow[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    qrow[i] = qt * BQ + wave * 32 + 16 * i + c;
    const int rc = min(qrow[i], p.Sq - 1);
    const unsigned char* qp = (const unsigned char*)p.q8 + (size_t)b * p.q_batch_stride + (size_t)rc * p.q_row_stride + h * D + 32 * g;
    const i32x4_t lo = *(const i32x4_t*)qp, hi = *(const i32x4_t*)(qp + 16);
    qf[i] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    cq[i] = ((const float*)p.sq)[(size_t)b * p.sq_batch_stride + (size_t)rc * p.H + h] * (p.scale * LOG2E);
  }

  f32x4_t acc[2][8], accl[2];
  float m[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    m[i] = -INFINITY;
    accl[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) acc[i][dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  const int one4 = 0x38383838;                                                 // four e4m3 ones
  const i32x8_t ones = {one4, one4, one4, one4, one4, one4, one4, one4};

  stage(0, 0);
  float skreg = load_sk(0);
  float* sk_lds = (float*)(smem + 2 * STAGE);

  auto step = [&](auto slot_c, int kt) {
    constexpr int SLOT = decltype(slot_c)::value, FREE = SLOT ^ 1;
    AF8_FENCE();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                           // my pieces and my sk value of tile kt have landed
    if (t < BK) sk_lds[SLOT * BK + t] = skreg;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                                              // everybody's have; tile kt - 1 is read out
    AF8_FENCE();
    if (kt + 1 < nk) {                                                         // (uniform)
      stage(FREE, kt + 1);
      skreg = load_sk(kt + 1);
    }
    AF8_FENCE();
    const unsigned char* sK = smem + SLOT * STAGE;
    const unsigned char* sV = sK + TILE;
    const float* sS = sk_lds + SLOT * BK + 32 * g;

    // ---- S^T = K Q^T ----
    f32x4_t st[2][8];
#pragma unroll
    for (int tt = 0; tt < 8; ++tt) {
      const i32x8_t kf = fragment(sK + tt * 16 * D, c, g);
#pragma unroll
      for (int i = 0; i < 2; ++i)
        st[i][tt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(kf, qf[i], f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0, 0, 0, 0);
    }
    // ---- x = s log2 e; the lane's keys are 128 kt + 32 g + 4 tt + r ----
    const bool tail = (kt == nk - 1) && (p.Skv & (BK - 1));
    float mx[2] = {-INFINITY, -INFINITY};
#pragma unroll
    for (int tt = 0; tt < 8; ++tt) {
      const f32x4_t skv = *(const f32x4_t*)(sS + 4 * tt);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float x = st[i][tt][r] * (skv[r] * cq[i]);
          if (tail && kt * BK + 32 * g + 4 * tt + r >= p.Skv) x = -INFINITY;
          st[i][tt][r] = x;
          mx[i] = fmaxf(mx[i], x);
        }
    }
    bool moved = false;
    float mm[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      mx[i] = fmaxf(mx[i], __shfl_xor(mx[i], 16, 64));
      mx[i] = fmaxf(mx[i], __shfl_xor(mx[i], 32, 64));
      mx[i] = fmaxf(mx[i], m[i]);
      moved |= mx[i] > m[i];
      mm[i] = mx[i] - P_SHIFT;
    }
    if (__any(moved)) {                                                        // (uniform over the wave)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float alpha = __builtin_amdgcn_exp2f(m[i] - mx[i]);              // 1 exactly where the row did not move; 0 at the first tile
        accl[i] *= alpha;
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) acc[i][dt] *= alpha;
        m[i] = mx[i];
      }
    }
    // ---- P: 32 keys of query c -> 8 VGPRs in key order ----
    i32x8_t pf[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int tt = 0; tt < 8; ++tt) {
        int w = 0;
        w = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_amdgcn_exp2f(st[i][tt][0] - mm[i]), __builtin_amdgcn_exp2f(st[i][tt][1] - mm[i]), w, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_amdgcn_exp2f(st[i][tt][2] - mm[i]), __builtin_amdgcn_exp2f(st[i][tt][3] - mm[i]), w, true);
        pf[i][tt] = w;
      }
    // ---- l += 1 P^T, O^T += V^T P^T ----
#pragma unroll
    for (int i = 0; i < 2; ++i) accl[i] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(ones, pf[i], accl[i], 0, 0, 0, 0, 0, 0);
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
      const i32x8_t vf = fragment(sV + dt * 16 * D, c, g);
#pragma unroll
      for (int i = 0; i < 2; ++i) acc[i][dt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(vf, pf[i], acc[i][dt], 0, 0, 0, 0, 0, 0);
    }
    AF8_FENCE();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                         // my reads of this stage are in registers
  };
  for (int kt = 0; kt < nk; kt += 2) {                                         // (the conditions are uniform over the workgroup)
    step(std::integral_constant<int, 0>{}, kt);
    if (kt + 1 < nk) step(std::integral_constant<int, 1>{}, kt + 1);
  }

  // ---- epilogue: acc[i][dt][r] = O[query c of fragment i][channel 16 dt + 4 g + r] ----
  const float* svb = (const float*)p.sv + (size_t)b * p.H * D + h * D + 4 * g;
  uint16_t* ob = (uint16_t*)p.out + (size_t)b * p.o_batch_stride + h * D + 4 * g;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if (qrow[i] >= p.Sq) continue;
    const float l = accl[i][0];
    uint16_t* orow = ob + (size_t)qrow[i] * p.o_row_stride;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
      const f32x4_t sv = *(const f32x4_t*)(svb + 16 * dt);
      float y[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) y[r] = sv[r] * acc[i][dt][r] / l;
      *(uint2*)(orow + 16 * dt) = make_uint2(pack_bf2(y[0], y[1]), pack_bf2(y[2], y[3]));
    }
  }
#endif  // __HIP_DEVICE_COMPILE__
}

// ---- prepare ----
__device__ __forceinline__ uint2 quant8(const float* f, float inv) {
  float q[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) q[e] = fminf(fmaxf(f[e] * inv, -448.0f), 448.0f);
  int w0 = 0, w1 = 0;
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], w0, false);
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], w0, true);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(q[4], q[5], w1, false);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(q[6], q[7], w1, true);
  return make_uint2((uint32_t)w0, (uint32_t)w1);
}

struct prepare_args {
  const uint16_t* qk;
  const uint16_t* vt;
  unsigned char *q8, *k8, *vt8;
  float *sq, *sk, *sv;
  long long qk_ld, vt_ld, vt_batch_stride;
  int B, S, H, S8;
  unsigned blocks_qk;
};

__global__ __launch_bounds__(256) void prepare_kernel(const prepare_args a) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int t = threadIdx.x;
  const int C = a.H * D;
  if (blockIdx.x < a.blocks_qk) {
    // 16 lanes per (token, q|k head) row of 128
    const long long items = (long long)a.B * a.S * 2 * a.H;
    const long long item = (long long)blockIdx.x * 16 + (t >> 4);
    const long long it = item < items ? item : items - 1;
    const long long token = it / (2 * a.H);
    const int j = (int)(it - token * 2 * a.H), l16 = t & 15;
    const bool is_k = j >= a.H;
    const int head = is_k ? j - a.H : j;
    const uint4 v = *(const uint4*)(a.qk + token * a.qk_ld + j * D + 8 * l16);
    float f[8];
    unpack8(v, f);
    float amax = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(f[e]));
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    const float sc = amax == 0.f ? 1.0f : amax / 448.0f;
    const float inv = 1.0f / sc;
    if (item < items) {
      *(uint2*)((is_k ? a.k8 : a.q8) + token * C + head * D + 8 * l16) = quant8(f, inv);
      if (l16 == 0) (is_k ? a.sk : a.sq)[token * a.H + head] = sc;
    }
    return;
  }
  // one (channel, batch) row of V^T: S keys in, S8 bytes out
  __shared__ float red[4];
  const int idx = (int)(blockIdx.x - a.blocks_qk);
  const int ch_ = idx / a.B, b = idx - ch_ * a.B;
  const uint16_t* src = a.vt + (long long)ch_ * a.vt_ld + (long long)b * a.vt_batch_stride;
  const bool fast = ((uintptr_t)src & 15) == 0;
  auto load8 = [&](int k0, float* f) {
    if (fast && k0 + 8 <= a.S) {
      unpack8(*(const uint4*)(src + k0), f);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = k0 + e < a.S ? bf2f(src[k0 + e]) : 0.f;
    }
  };
  float amax = 0.f;
  for (int k0 = 8 * t; k0 < a.S; k0 += 8 * 256) {
    float f[8];
    load8(k0, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(f[e]));
  }
  amax = wave_max(amax);
  if ((t & 63) == 0) red[t >> 6] = amax;
  __syncthreads();
  amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float sc = amax == 0.f ? 1.0f : amax / 448.0f;
  const float inv = 1.0f / sc;
  if (t == 0) a.sv[(long long)b * C + ch_] = sc;
  unsigned char* dst = a.vt8 + ((long long)ch_ * a.B + b) * a.S8;
  for (int k0 = 8 * t; k0 < a.S8; k0 += 8 * 256) {                             // keys [S, S8) load as zero and store as zero
    float f[8];
    load8(k0, f);
    *(uint2*)(dst + k0) = quant8(f, inv);
  }
#endif  // __HIP_DEVICE_COMPILE__
}

}  // namespace da_attention_fp8_ns

extern "C" int da_attention_fp8_prepare(const void* qk, long long qk_ld, const void* vt, long long vt_ld, long long vt_batch_stride, void* q8,
                                        void* k8, void* vt8, void* sq, void* sk, void* sv, int B, int S, int H, int D, void* stream) {
  using namespace da_attention_fp8_ns;
  if (!qk || !vt || !q8 || !k8 || !vt8 || !sq || !sk || !sv) return DA_ERR_INVALID;
  if (D != da_attention_fp8_ns::D || B < 1 || S < 1 || H < 1) return DA_ERR_UNSUPPORTED;
  const long long C = (long long)H * D, S8 = ((long long)S + 127) / 128 * 128;
  if (qk_ld < 2 * C || (qk_ld & 7) || ((uintptr_t)qk & 15) || ((uintptr_t)vt & 1) || vt_ld < 1 || vt_batch_stride < 0) return DA_ERR_UNSUPPORTED;
  if (((uintptr_t)q8 & 7) || ((uintptr_t)k8 & 7) || ((uintptr_t)vt8 & 7) || ((uintptr_t)sq & 3) || ((uintptr_t)sk & 3) || ((uintptr_t)sv & 3))
    return DA_ERR_UNSUPPORTED;
  const long long blocks_qk = ((long long)B * S * 2 * H + 15) / 16, blocks = blocks_qk + C * B;
  if (blocks > 0x7fffffffLL || S8 > 0x7fffffffLL) return DA_ERR_UNSUPPORTED;
  prepare_args a;
  a.qk = (const uint16_t*)qk, a.vt = (const uint16_t*)vt;
  a.q8 = (unsigned char*)q8, a.k8 = (unsigned char*)k8, a.vt8 = (unsigned char*)vt8;
  a.sq = (float*)sq, a.sk = (float*)sk, a.sv = (float*)sv;
  a.qk_ld = qk_ld, a.vt_ld = vt_ld, a.vt_batch_stride = vt_batch_stride;
  a.B = B, a.S = S, a.H = H, a.S8 = (int)S8, a.blocks_qk = (unsigned)blocks_qk;
  DA_LAUNCH(prepare_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

extern "C" int da_attention_fp8(const da_attention_fp8_params* p, void* stream) {
  using namespace da_attention_fp8_ns;
  if (!p || !p->q8 || !p->k8 || !p->vt8 || !p->sq || !p->sk || !p->sv || !p->out) return DA_ERR_INVALID;
  if (p->D != da_attention_fp8_ns::D || p->B < 1 || p->H < 1 || p->Sq < 1 || p->Skv < 1) return DA_ERR_UNSUPPORTED;
  const long long nk = ((long long)p->Skv + BK - 1) / BK;
  if (p->S8 < nk * BK || (p->S8 & 127)) return DA_ERR_UNSUPPORTED;
  const int C = p->H * da_attention_fp8_ns::D;
  // 16-byte loads of Q and 16-byte DMA pieces of K and V^T; 8-byte stores of four adjacent bf16
  if (p->q_row_stride < C || (p->q_row_stride & 15) || (p->q_batch_stride & 15) || ((uintptr_t)p->q8 & 15)) return DA_ERR_UNSUPPORTED;
  if (p->k_row_stride < C || (p->k_row_stride & 15) || (p->k_batch_stride & 15) || ((uintptr_t)p->k8 & 15)) return DA_ERR_UNSUPPORTED;
  if (p->vt_ld < nk * BK || (p->vt_ld & 15) || (p->vt_batch_stride & 15) || ((uintptr_t)p->vt8 & 15)) return DA_ERR_UNSUPPORTED;
  if (p->o_row_stride < C || (p->o_row_stride & 3) || (p->o_batch_stride & 3) || ((uintptr_t)p->out & 7)) return DA_ERR_UNSUPPORTED;
  if (p->q_batch_stride < 0 || p->k_batch_stride < 0 || p->vt_batch_stride < 0 || p->o_batch_stride < 0 || p->sq_batch_stride < 0 ||
      p->sk_batch_stride < 0)
    return DA_ERR_UNSUPPORTED;
  if (((uintptr_t)p->sq & 3) || ((uintptr_t)p->sk & 3) || ((uintptr_t)p->sv & 15)) return DA_ERR_UNSUPPORTED;
  // 32-bit byte offsets inside one (batch, head)'s K rows and V^T tile rows
  if (((long long)p->Skv + BK) * p->k_row_stride > 0x7fffffffLL || 128LL * p->vt_ld + p->S8 > 0x7fffffffLL) return DA_ERR_UNSUPPORTED;
  const long long grid = (long long)p->B * p->H * ((p->Sq + BQ - 1) / BQ);
  if (grid > 0x7fffffffLL) return DA_ERR_UNSUPPORTED;
  if (hipFuncSetAttribute((const void*)attention_fp8_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) != hipSuccess)
    return DA_ERR_LAUNCH;
  DA_LAUNCH(attention_fp8_kernel, dim3((unsigned)grid), dim3(256), LDS_BYTES, (hipStream_t)stream, *p);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
