// FP8 (OCP e4m3, torch.float8_e4m3fn -- gfx950's native 8-bit float, not the fnuz form) linears on gfx950: a row quantiser and a
// row-scaled GEMM on the 8-bit matrix instruction.  Opt-in (FluxTransformer2DModel.enable_fp8_linears); nothing else calls them.
//
// (a) da_quantize_rows_e4m3: bf16 x[R][K] (row stride ldx) -> e4m3 q[R][K] (row stride ldq bytes) + fp32 scale[R].  Per row, in fp32:
//       amax  = max_k |x[k]|
//       scale = amax / 448          (IEEE division; 448 = the largest finite e4m3)          scale = 1 when amax == 0
//       inv   = 1 / scale           (IEEE division)
//       q[k]  = e4m3_rne(min(max(x[k] * inv, -448), 448))                                   (one fp32 multiply, clamp, RNE convert)
//     so x[k] ~ scale * q[k].  Finite inputs only (a NaN or an infinity in a row makes that row's scale useless).  One wave per row,
//     four rows per workgroup: 16-byte loads (8 bf16), amax across the lanes with five xor-shuffles, then a second pass over the row
//     (it comes back from L2) that converts with v_cvt_pk_fp8_f32, two values per instruction, and stores 8 bytes per lane and chunk.
//     The same kernel quantises activations per token (every step) and weights per output channel (once): a weight [N][K] is just rows.
//
// (b) da_gemm_fp8: out[m][n] = epilogue(sa[m] * sb[n] * sum_k A8[m][k] * B8[n][k]), A8 [M][K] and B8 [N][K] e4m3 with K contiguous,
//     fp32 accumulation, bf16 out with a row stride.  The operand form is symmetric: the transposed-V projection (weights as the M
//     operand, bias along M) is the same kernel with the operands swapped.  K % 128 == 0, K >= 128.
//
// Instruction: v_mfma_f32_16x16x128_f8f6f4 with both formats e4m3 and no block scales (the builtin's scale operands are the constant
// 0, for which the compiler emits the unscaled encoding).  One instruction multiplies a 16 x 128 by a 128 x 16 tile: 128 bytes of K.
// Fragment layout (lane = 16 g + c, c = lane & 15, g = lane >> 4):
//   first / second source  8 VGPRs = 32 bytes: row c of the 16-row operand tile, K bytes 32 g .. 32 g + 31 in register order
//   accumulator            4 VGPRs: element [4 g + r][c] of (first source rows) x (second source rows), r = 0 .. 3
// The two sources use the same (lane, byte) -> k map, so the sum does not depend on which k a byte is taken to be as long as both
// operands are read through the same map; the kernel reads both through fragment() below.  The B tile goes FIRST and the A tile second:
// the accumulator is then C^T, lane (c, g) holds output row c and the four adjacent columns 4 g .. 4 g + 3 -- one 8-byte store.
//
// Tile / waves: 256 x 256 output tile, 8 waves as 2 (M) x 4 (N), a wave owns 128 x 64 = 8 x 4 accumulators of 16 x 16 (128 VGPRs).  A
// second instantiation, 128 x 256 with a wave owning 64 x 64, serves M <= 128 and launches whose 256 x 256 grid would fill the last
// round of CUs worse.  K loop in steps of 128 bytes: both operand tiles of a step are staged by LDS-DMA (buffer_load ... lds, 16 bytes
// per lane, 1 KiB = 8 rows per wave instruction) into a ring of 2 stages of 64 KiB (256 x 256) or 3 stages of 48 KiB (128 x 256).  Per
// step: counted vmcnt wait for the oldest stage, ONE barrier (the stage is everybody's; everybody is done reading the stage before
// it), issue the loads of step kt + NS - 1 into the slot just freed, then 4 B fragments are read once and every A fragment is
// read and used for 4 MFMAs.  Steps past K reload the last step (same load count, one vmcnt immediate, nothing read from them).
// LDS rows are 128 bytes = two rows per 64 banks: the 16-byte chunk j of row r lives at slot j ^ ((r >> 1) & 7) (applied on the SOURCE
// address of the DMA, whose LDS side is linear), which makes the 16 rows of a fragment read hit 16 different bank groups.
// Tails: rows past M / N are clamped to the last valid row when staged (unconditional loads; the buffer descriptor ends at the
// operand's last valid byte) and their products are never stored; epilogue loads use clamped indices, stores are masked.
// Epilogue, all fp32, ONE rounding to bf16:  y = sa[m] sb[n] acc + bias[n] + bias_rows[m];  y = gelu_tanh(y) if act;
// y = gate[m / rows_per_batch][n] * y + residual[m][n] if gate / residual.  (The bf16 da_gemm_bf16 rounds the linear output and the
// gated product to bf16 on the way; this kernel does not.)  No split-K, no workspace: the result depends on the inputs alone.
#include "common.cuh"
#include <type_traits>

namespace da_gemm_fp8_ns {

typedef __attribute__((ext_vector_type(8))) int i32x8_t;
typedef __attribute__((ext_vector_type(4))) int i32x4_t;

constexpr int BN = 256;
constexpr int KSTEP = 128;   // bytes of K per stage = one MFMA
#define F8_LDS(ptr) ((__attribute__((address_space(3))) void*)(ptr))
#define F8_FENCE() __builtin_amdgcn_sched_barrier(0)

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* base, long long bytes) {
  const uint64_t v = (uint64_t)base;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  const int n = __builtin_amdgcn_readfirstlane((int)(bytes > 0x7fffffffLL ? 0x7fffffffLL : bytes));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), 0, n, 0x00020000);
}

// row c of a 16-row tile at `tile` (128-byte rows), K bytes 32 g .. 32 g + 31: chunks 2 g and 2 g + 1 through the swizzle
__device__ __forceinline__ i32x8_t fragment(const unsigned char* tile, int c, int g) {
  const int sw = (c >> 1) & 7;
  const i32x4_t lo = *(const i32x4_t*)(tile + c * 128 + (((2 * g) ^ sw) << 4));
  const i32x4_t hi = *(const i32x4_t*)(tile + c * 128 + (((2 * g + 1) ^ sw) << 4));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <int BM, int NS>
__global__ __launch_bounds__(512) void gemm_fp8_kernel(const da_gemm_fp8_params p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int MI = BM / 32;                  // 16-row tiles of a wave along M (the wave owns BM / 2 rows)
  constexpr int NJ = 4;                        // 16-column tiles of a wave along N (64 columns)
  constexpr int STAGE = (BM + BN) * KSTEP;     // bytes of one ring stage: A tile, then B tile
  constexpr int PA = BM / 64, PB = BN / 64;    // 8-row pieces per wave and stage
  constexpr int LOADS = PA + PB;
  static_assert((NS - 1) * LOADS <= 63, "vmcnt is a 6-bit counter");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = threadIdx.x;
  const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int c = lane & 15, g = lane >> 4;

  const int tiles_n = (p.N + BN - 1) / BN;
  const int tm = (int)blockIdx.x / tiles_n, tn = (int)blockIdx.x - tm * tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  const int nk = p.K / KSTEP;
  const int rows_a = min(BM, p.M - m0), rows_b = min(BN, p.N - n0);      // valid rows of this tile's operands (>= 1)

  const unsigned char* A = (const unsigned char*)p.A + (size_t)m0 * p.lda;
  const unsigned char* B = (const unsigned char*)p.B + (size_t)n0 * p.ldb;
  __amdgpu_buffer_rsrc_t rs_a = rsrc(A, (long long)(rows_a - 1) * p.lda + p.K);
  __amdgpu_buffer_rsrc_t rs_b = rsrc(B, (long long)(rows_b - 1) * p.ldb + p.K);

  // staging: wave w sends pieces w, w + 8, ...; lane -> row 8 piece + (lane >> 3), LDS slot lane & 7 = source chunk slot ^ swizzle
  int vo_a[PA], vo_b[PB];
#pragma unroll
  for (int i = 0; i < PA; ++i) {
    const int row = 8 * (wave + 8 * i) + (lane >> 3);
    vo_a[i] = min(row, rows_a - 1) * p.lda + (((lane & 7) ^ ((row >> 1) & 7)) << 4);
  }
#pragma unroll
  for (int i = 0; i < PB; ++i) {
    const int row = 8 * (wave + 8 * i) + (lane >> 3);
    vo_b[i] = min(row, rows_b - 1) * p.ldb + (((lane & 7) ^ ((row >> 1) & 7)) << 4);
  }
  auto stage = [&](int slot, int ks) {
    const int so = min(ks, nk - 1) * KSTEP;
    unsigned char* dst = smem + slot * STAGE + wave * 1024;
#pragma unroll
    for (int i = 0; i < PA; ++i) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_a, F8_LDS(dst + i * 8192), 16, vo_a[i], so, 0, 0);
#pragma unroll
    for (int i = 0; i < PB; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_b, F8_LDS(dst + BM * KSTEP + i * 8192), 16, vo_b[i], so, 0, 0);
  };

  f32x4_t acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int s = 0; s < NS - 1; ++s) stage(s, s);

  const unsigned char* fa = smem + wr * (BM / 2) * KSTEP;
  const unsigned char* fb = smem + BM * KSTEP + wc * 64 * KSTEP;
  // one K step on ring slot SLOT (a compile-time constant: the compiler then sees that the DMA of the freed slot and the fragment
  // reads of this one do not overlap, and puts no vmcnt(0) of its own between them)
  auto step = [&](auto slot_c, int kt) {
    constexpr int SLOT = decltype(slot_c)::value, FREE = (SLOT + NS - 1) % NS;
    F8_FENCE();
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * LOADS) : "memory");   // my pieces of step kt have landed
    __builtin_amdgcn_s_barrier();                                              // everybody's have; step kt - 1 is read out
    F8_FENCE();
    stage(FREE, kt + NS - 1);
    F8_FENCE();
    const unsigned char* sa_ = fa + SLOT * STAGE;
    const unsigned char* sb_ = fb + SLOT * STAGE;
    i32x8_t bf[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) bf[j] = fragment(sb_ + j * 16 * KSTEP, c, g);
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const i32x8_t af = fragment(sa_ + i * 16 * KSTEP, c, g);
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bf[j], af, acc[i][j], 0, 0, 0, 0, 0, 0);
    }
    F8_FENCE();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                         // my fragment reads of this stage are in registers
  };
  for (int kt = 0; kt < nk; kt += NS) {                                        // (the conditions are uniform over the workgroup)
    step(std::integral_constant<int, 0>{}, kt);
    if (kt + 1 < nk) step(std::integral_constant<int, 1>{}, kt + 1);
    if constexpr (NS == 3) {
      if (kt + 2 < nk) step(std::integral_constant<int, 2>{}, kt + 2);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                             // the reloads of the steps past K

  // ---- epilogue: acc[i][j][r] = C[row][col + r], row = .. + 16 i + c, col = .. + 16 j + 4 g ----
  const float* __restrict__ sa = (const float*)p.scale_a;
  const float* __restrict__ sb = (const float*)p.scale_b;
  const uint16_t* __restrict__ bias = (const uint16_t*)p.bias;
  const uint16_t* __restrict__ bias_rows = (const uint16_t*)p.bias_rows;
  const uint16_t* __restrict__ gate = (const uint16_t*)p.gate;
  const uint16_t* __restrict__ res = (const uint16_t*)p.residual;
  uint16_t* __restrict__ C = (uint16_t*)p.C;
  const bool vec = ((p.ldc & 3) == 0) && (((uintptr_t)p.C & 7) == 0);       // 8-byte stores of four adjacent columns
  const int rpb = p.rows_per_batch > 0 ? p.rows_per_batch : p.M;
  const int col_w = n0 + wc * 64 + 4 * g;

  float sbv[NJ][4], bv[NJ][4];
  int colc[NJ][4];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      colc[j][r] = min(col_w + 16 * j + r, p.N - 1);
      sbv[j][r] = sb[colc[j][r]];
      bv[j][r] = bias ? bf2f(bias[colc[j][r]]) : 0.f;
    }
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int row = m0 + wr * (BM / 2) + 16 * i + c;
    const int rowc = min(row, p.M - 1);
    const float sar = sa[rowc];
    const float br = bias_rows ? bf2f(bias_rows[rowc]) : 0.f;
    const uint16_t* grow = gate ? gate + (size_t)(rowc / rpb) * p.ld_gate : nullptr;
    const uint16_t* rrow = res ? res + (size_t)rowc * p.ldr : nullptr;
    uint16_t* crow = C + (size_t)rowc * p.ldc;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      float y[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        y[r] = acc[i][j][r] * (sar * sbv[j][r]) + bv[j][r] + br;
        if (p.act == DA_ACT_GELU_TANH) y[r] = gelu_tanh_f(y[r]);
        if (grow) y[r] *= bf2f(grow[colc[j][r]]);
        if (rrow) y[r] += bf2f(rrow[colc[j][r]]);
      }
      const int col = col_w + 16 * j;
      if (row < p.M) {
        if (vec && col + 3 < p.N) {
          *(uint2*)(crow + col) = make_uint2(pack_bf2(y[0], y[1]), pack_bf2(y[2], y[3]));
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (col + r < p.N) crow[col + r] = f2bf(y[r]);
        }
      }
    }
  }
#endif  // __HIP_DEVICE_COMPILE__
}

constexpr int QW = 4;   // rows (waves) per workgroup of the quantiser

__global__ __launch_bounds__(64 * QW) void quantize_rows_kernel(const uint16_t* __restrict__ x, long long ldx, unsigned char* __restrict__ q,
                                                                long long ldq, float* __restrict__ scale, int rows, int K) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const long long row = (long long)blockIdx.x * QW + wave;
  if (row >= rows) return;                              // wave-uniform; the kernel has no barrier
  const uint16_t* xr = x + row * ldx;
  const int chunks = K >> 3;
  float amax = 0.f;
  for (int ch = lane; ch < chunks; ch += 64) {
    const uint4 v = *(const uint4*)(xr + 8 * ch);
    float f[8];
    unpack8(v, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(f[e]));
  }
  amax = wave_max(amax);
  const float sc = amax == 0.f ? 1.0f : amax / 448.0f;
  const float inv = 1.0f / sc;
  if (lane == 0) scale[row] = sc;
  unsigned char* qr = q + row * ldq;
  for (int ch = lane; ch < chunks; ch += 64) {
    const uint4 v = *(const uint4*)(xr + 8 * ch);
    float f[8];
    unpack8(v, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = fminf(fmaxf(f[e] * inv, -448.0f), 448.0f);
    int w0 = 0, w1 = 0;
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], w0, false);
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w0, true);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], w1, false);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], w1, true);
    *(uint2*)(qr + 8 * ch) = make_uint2((uint32_t)w0, (uint32_t)w1);
  }
#endif  // __HIP_DEVICE_COMPILE__
}

template <int BM, int NS>
int launch(const da_gemm_fp8_params* p, hipStream_t s) {
  constexpr int LDSB = NS * (BM + BN) * KSTEP;
  auto kern = gemm_fp8_kernel<BM, NS>;
  if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, LDSB) != hipSuccess) return DA_ERR_LAUNCH;
  const long long grid = (long long)((p->M + BM - 1) / BM) * ((p->N + BN - 1) / BN);
  if (grid > 0x7fffffffLL) return DA_ERR_UNSUPPORTED;
  DA_LAUNCH(kern, dim3((unsigned)grid), dim3(512), LDSB, s, *p);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

}  // namespace da_gemm_fp8_ns

extern "C" int da_quantize_rows_e4m3(const void* x, long long ldx, void* q, long long ldq, void* scale, int rows, int K, void* stream) {
  using namespace da_gemm_fp8_ns;
  if (!x || !q || !scale) return DA_ERR_INVALID;
  if (rows < 1 || K < 128 || (K & 127) || ldx < K || ldq < K) return DA_ERR_UNSUPPORTED;
  if ((ldx & 7) || ((uintptr_t)x & 15) || (ldq & 7) || ((uintptr_t)q & 7) || ((uintptr_t)scale & 3)) return DA_ERR_UNSUPPORTED;
  DA_LAUNCH(quantize_rows_kernel, dim3((unsigned)((rows + QW - 1) / QW)), dim3(64 * QW), 0, (hipStream_t)stream, (const uint16_t*)x, ldx,
            (unsigned char*)q, ldq, (float*)scale, rows, K);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

extern "C" int da_gemm_fp8(const da_gemm_fp8_params* p, void* stream) {
  using namespace da_gemm_fp8_ns;
  if (!p || !p->A || !p->B || !p->scale_a || !p->scale_b || !p->C) return DA_ERR_INVALID;
  if (p->M < 1 || p->N < 1 || p->K < 128 || (p->K & 127)) return DA_ERR_UNSUPPORTED;
  if (p->act != DA_ACT_NONE && p->act != DA_ACT_GELU_TANH) return DA_ERR_UNSUPPORTED;
  if (p->tile < DA_FP8_TILE_AUTO || p->tile > DA_FP8_TILE_128x256) return DA_ERR_UNSUPPORTED;
  // 16-byte DMA pieces from rows of whole chunks; 32-bit byte offsets inside a tile's 256 rows
  if (p->lda < p->K || p->ldb < p->K || (p->lda & 15) || (p->ldb & 15) || ((uintptr_t)p->A & 15) || ((uintptr_t)p->B & 15))
    return DA_ERR_UNSUPPORTED;
  if (256LL * p->lda > 0x7fffffffLL || 256LL * p->ldb > 0x7fffffffLL) return DA_ERR_UNSUPPORTED;
  if (p->ldc < p->N || ((uintptr_t)p->C & 1) || ((uintptr_t)p->scale_a & 3) || ((uintptr_t)p->scale_b & 3)) return DA_ERR_UNSUPPORTED;
  if (p->residual && p->ldr < p->N) return DA_ERR_UNSUPPORTED;
  if (p->gate && (p->ld_gate < p->N || p->rows_per_batch < 0)) return DA_ERR_UNSUPPORTED;
  int tile = p->tile;
  if (tile == DA_FP8_TILE_AUTO) {
    // the tile whose grid fills its rounds of 256 CUs better; 256 x 256 on a tie (half the operand traffic per output)
    const long long tn = (p->N + 255) / 256, t256 = ((p->M + 255) / 256) * tn, t128 = ((p->M + 127) / 128) * tn;
    const long long r256 = (t256 + 255) / 256, r128 = (t128 + 255) / 256;      // time ~ rounds x tile height
    tile = (p->M <= 128 || r128 < 2 * r256) ? DA_FP8_TILE_128x256 : DA_FP8_TILE_256x256;
  }
  hipStream_t s = (hipStream_t)stream;
  return tile == DA_FP8_TILE_256x256 ? launch<256, 2>(p, s) : launch<128, 3>(p, s);
}
