// Flash attention forward for ONE WIDE HEAD per (batch, head) pair on gfx950: unmasked, D = 256 / 384 / 512, bf16 in / bf16 out.
//
// Call sites: the single-head mid-block attention of the VAEs (vae.py / unet_2d_blocks.py:736-748 through attention_processor.py:2767:
// head_dim = channels = 512 for the SD / SDXL / FLUX AutoencoderKL; autoencoder_kl_wan.py:389-431: 384 for AutoencoderKLWan).
// Reached through da_attention_bf16 (attention.hip); operand layouts and stride rules are the header's.
//
// The swapped products of the other two generations, on the 16 x 16 x 32 MFMA:
//
//   S^T[kv][q] = K[kv][:] . Q[q][:]^T      A = K tile (LDS), B = Q (registers, resident for the whole key loop)
//   O^T[d][q]  = V^T[d][kv] . P^T[kv][q]   A = V^T tile (LDS), B = P^T (registers, straight from the S^T accumulators)
//
// A workgroup is four waves x 16 queries (one wave per SIMD); a wave owns its 16 query columns AND the whole D-wide fp32 output
// accumulator for them (D / 16 tiles of 4 registers: 128 registers at D = 512, next to 64 registers of Q), so every score is computed
// exactly once, no score or probability crosses a wave, and a lane (q = lane & 15, g = lane >> 4) sees only its own query: the row
// maximum is two lane exchanges per tile (over g), the row sum stays a per-lane partial until the epilogue.
//
//  * Key tiles of 32: K [32][D] and V^T [D][32] (32 KB + 32 KB at D = 512) are staged ONCE per workgroup by buffer-addressed LDS-DMA
//    (attention2.hip): per-lane byte offsets are loop constants, the tile advance is a scalar offset, chunks past Skv_alloc carry bit
//    31 in the offset (the range check writes zeros to LDS and reads nothing).  Two ring slots (128 KB at D = 512): tile j + 1 flies
//    while tile j is consumed; one rendezvous per tile.
//  * K rows are fed to the first product PERMUTED: A-row i = 4 a + b of key block kb takes key 8 a + 4 kb + b.  The C layout of the
//    16 x 16 MFMA then leaves lane g with keys 8 g .. 8 g + 7 of the tile in its two accumulators, which IS the B fragment of the
//    32-deep second product in natural key order, and a V^T A-fragment is one ds_read_b128.
//  * 16-byte-slot XOR swizzles applied on the DMA's source side keep both kinds of fragment reads free of bank conflicts: K slot ^
//    (4 (row >> 3) | row & 3) -- for the permuted rows of a lane group that is simply lane & 15 --, V^T slot ^ ((d >> 2) & 3).
//  * Deferred maximum (attention2.hip): O / l are rescaled only when some row of the wave outgrows its shift by more than 2^THR
//    (128 multiplies at D = 512: not something to spend on every tile); otherwise P = exp2(s c - m) with the old shift, <= 2^THR.
//  * Arithmetic as in the first generation: exp2 with scale * log2 e folded in, fp32 running maximum and sum (of the unrounded P), P
//    rounded to bf16 for the second product only, O normalised once and stored as whole rows through LDS (16 bytes per lane).
//
// What bounds the loop: every A fragment is used by ONE MFMA (16 queries per wave), so a wave reads the whole 64 KB tile pair from LDS
// per tile -- 64 ds_read_b128 for 64 MFMAs at D = 512.  Budgets per D (registers: accumulator + Q; LDS: two slots):
//   D = 256:  64 + 32 registers,  64 KB;   D = 384:  96 + 48 registers,  96 KB;   D = 512: 128 + 64 registers, 128 KB.
#include "common.cuh"

namespace da_attn_wide {

constexpr int kQB = 64;              // queries per workgroup (4 waves x 16)
constexpr int kKT = 32;              // keys per tile
constexpr int kNW = kQB / 16;
constexpr float kDeferLog2 = 8.0f;   // THR: P stays <= 2^8 between rescales

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t uniform_rsrc(const void* base) {
  const uint64_t v = (uint64_t)base;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), 0, 0x7fffffff, 0x00020000);
}
#endif

template <int D>
struct Cfg {
  static constexpr int CPR = D / 8;                 // 16-byte chunks per K row
  static constexpr int KBYTES = kKT * D * 2;        // K tile   [32][D]
  static constexpr int VBYTES = D * kKT * 2;        // V^T tile [D][32]
  static constexpr int STAGE = KBYTES + VBYTES;
  static constexpr int RING = 2 * STAGE;
  static constexpr int PCS = KBYTES / 1024 / kNW;   // 1 KiB pieces per wave per tile, of K and of V^T alike
  static constexpr int OROW = 2 * D + 16;           // bytes per staged output row (pad: the 8-byte writes spread over the banks)
};

__device__ __forceinline__ int k_swz(int row) { return ((row >> 1) & 12) | (row & 3); }

template <int D>
__global__ __launch_bounds__(64 * kNW, 1) void attn_wide_kernel(const da_attention_params p) {
#if defined(__HIP_DEVICE_COMPILE__)
  using C = Cfg<D>;
  static_assert(D == 256 || D == 384 || D == 512, "head sizes of the wide kernel");
  static_assert(C::CPR % 16 == 0, "the K swizzle permutes slots inside groups of 16");
  static_assert(C::PCS * kNW * 1024 == C::KBYTES && C::KBYTES == C::VBYTES, "pieces divide among the waves");
  static_assert(C::RING <= 160 * 1024, "K / V^T ring exceeds the LDS of a CU");
  static_assert(kNW * 16 * C::OROW <= C::RING, "output staging does not fit the ring");
  constexpr int NKS = D / 32;                       // k-steps of the first product
  constexpr int NDB = D / 16;                       // output tiles of the second product
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int r16 = lane & 15, g = lane >> 4;

  const int qtiles = (p.Sq + kQB - 1) / kQB;
  const int ntiles = (p.Skv + kKT - 1) / kKT;
  const int pair = blockIdx.x / qtiles, qt = blockIdx.x - pair * qtiles;
  const int b = pair / p.H, h = pair - b * p.H;
  const int q0 = qt * kQB + wave * 16;

  const uint16_t* __restrict__ Q = (const uint16_t*)p.q + (size_t)b * p.q_batch_stride + (size_t)h * D;
  const uint16_t* __restrict__ K = (const uint16_t*)p.k + (size_t)b * p.k_batch_stride + (size_t)h * D;
  const uint16_t* __restrict__ VT = (const uint16_t*)p.vt + (size_t)h * D * p.vt_ld + (size_t)b * p.vt_batch_stride;
  uint16_t* __restrict__ O = (uint16_t*)p.out + (size_t)b * p.o_batch_stride + (size_t)h * D;
  const float sl2 = p.scale * 1.4426950408889634f;

  // ---- staging: piece pi = i * 4 + wave is 64 lanes x 16 B of a ring slot.  K: chunk pch = 64 pi + lane -> (row = pch / CPR,
  // slot = pch % CPR) takes source chunk slot ^ k_swz(row); V^T: (d = pch / 4, slot = pch % 4) takes source chunk slot ^ ((d >> 2) & 3).
  // Offsets are bytes from the (batch, head) base.  Only the LAST tile can reach past Skv_alloc: its offsets (vl_*) carry bit 31 on
  // the chunks that do.
  const __amdgpu_buffer_rsrc_t rs_k = uniform_rsrc(K);
  const __amdgpu_buffer_rsrc_t rs_v = uniform_rsrc(VT);
  int vo_k[C::PCS], vl_k[C::PCS], vo_v[C::PCS], vl_v[C::PCS];
  {
    const int rem_last = p.Skv_alloc - (ntiles - 1) * kKT;       // keys of the last tile that exist in memory
#pragma unroll
    for (int i = 0; i < C::PCS; ++i) {
      const int pch = (i * kNW + wave) * 64 + lane;
      const int row = pch / C::CPR, slot = pch % C::CPR;
      vo_k[i] = (row * p.k_row_stride + ((slot ^ k_swz(row)) << 3)) * 2;
      vl_k[i] = vo_k[i] | (row >= rem_last ? (int)0x80000000 : 0);
      const int d = pch >> 2, c = (pch & 3) ^ ((d >> 2) & 3);
      vo_v[i] = (d * p.vt_ld + c * 8) * 2;
      vl_v[i] = vo_v[i] | (c * 8 >= rem_last ? (int)0x80000000 : 0);   // Skv_alloc % 8 == 0: a chunk is all in or all out
    }
  }
#define DA_LDS(ptr) ((__attribute__((address_space(3))) void*)(ptr))
  auto issue = [&](int tile, int buf_off) {
    unsigned char* kb = smem + buf_off;
    unsigned char* vb = kb + C::KBYTES;
    const int so_k = tile * kKT * p.k_row_stride * 2, so_v = tile * kKT * 2;
    if (tile == ntiles - 1) {                                     // wave-uniform
#pragma unroll
      for (int i = 0; i < C::PCS; ++i) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_k, DA_LDS(kb + (i * kNW + wave) * 1024), 16, vl_k[i], so_k, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_v, DA_LDS(vb + (i * kNW + wave) * 1024), 16, vl_v[i], so_v, 0, 0);
      }
    } else {
#pragma unroll
      for (int i = 0; i < C::PCS; ++i) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_k, DA_LDS(kb + (i * kNW + wave) * 1024), 16, vo_k[i], so_k, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_v, DA_LDS(vb + (i * kNW + wave) * 1024), 16, vo_v[i], so_v, 0, 0);
      }
    }
  };
#undef DA_LDS
  issue(0, 0);

  // ---- Q fragments (MFMA B operand): lane (q = r16, g) holds Q[q][32 ks + 8 g + 0..7]; rows past Sq are zeros ----
  bf16x8_t qf[NKS];
  {
    const int q = q0 + r16;
    const bool ok = q < p.Sq;
    const uint16_t* qp = Q + (size_t)(ok ? q : 0) * p.q_row_stride + 8 * g;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      uint4 v = *(const uint4*)(qp + 32 * ks);
      if (!ok) v = make_uint4(0, 0, 0, 0);
      qf[ks] = __builtin_bit_cast(bf16x8_t, v);
    }
  }

  f32x4_t o[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i) o[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m_run = -1e30f, l_run = 0.f;               // l_run: this lane's partial over its 8 keys of every tile

  // fragment addresses (bytes inside a ring slot): lane constants, the rest are immediates
  const int krow = 8 * (r16 >> 2) + (r16 & 3);     // key row this lane feeds as A-row r16 of key block 0 (block 1: + 4); k_swz = r16
  const int kbase = krow * (2 * D);
  const int vbase = C::KBYTES + r16 * 64 + ((g ^ (r16 >> 2)) << 4);

  int cur = 0;
  for (int j = 0; j < ntiles; ++j) {
    // tile j has landed (every wave's pieces) and every wave is done with tile j - 1: its slot takes tile j + 1
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (j + 1 < ntiles) issue(j + 1, cur ^ C::STAGE);
    const unsigned char* sb = smem + cur;

    f32x4_t s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const int off = kbase + (((4 * ks + g) ^ r16) << 4);
      const bf16x8_t a0 = *(const bf16x8_t*)(sb + off);
      const bf16x8_t a1 = *(const bf16x8_t*)(sb + off + 4 * (2 * D));
      s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, qf[ks], s0, 0, 0, 0);
      s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, qf[ks], s1, 0, 0, 0);
    }
    // lane (q, g): s0[e] / s1[e] = key 32 j + 8 g + e / + 4 + e of query q, in log2-units from here on
    float sc[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) sc[e] = s0[e] * sl2, sc[4 + e] = s1[e] * sl2;
    if ((j + 1) * kKT > p.Skv) {                                  // ragged last tile (wave-uniform): keys past Skv exponentiate to 0
#pragma unroll
      for (int e = 0; e < 8; ++e) sc[e] = (j * kKT + 8 * g + e >= p.Skv) ? -1e30f : sc[e];
    }
    float mx = fmaxf(fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3])), fmaxf(fmaxf(sc[4], sc[5]), fmaxf(sc[6], sc[7])));
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    // deferred maximum: keep the shift while no row of the wave outgrows it by more than 2^THR (m starts at -1e30: the first tile
    // always takes the branch, with alpha = 0 on accumulators that are still zero)
    if (__builtin_amdgcn_ballot_w64(mx - m_run > kDeferLog2) != 0) {
      const float m_new = fmaxf(m_run, mx);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      m_run = m_new;
      l_run *= alpha;
#pragma unroll
      for (int i = 0; i < NDB; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) o[i][e] *= alpha;
    }
    float ps = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sc[e] = __builtin_amdgcn_exp2f(sc[e] - m_run);
      ps += sc[e];
    }
    l_run += ps;
    const bf16x8_t pf = __builtin_bit_cast(bf16x8_t, pack8(sc));   // P^T B fragment: keys 8 g .. 8 g + 7
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
      const bf16x8_t av = *(const bf16x8_t*)(sb + vbase + db * 1024);
      o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, pf, o[db], 0, 0, 0);
    }
    cur ^= C::STAGE;
  }

  // ---- epilogue: O^T registers -> LDS (per wave) -> whole rows, 16 bytes per lane ----
  float l_tot = l_run + __shfl_xor(l_run, 16, 64);
  l_tot += __shfl_xor(l_tot, 32, 64);
  const float inv = 1.0f / l_tot;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();                                   // every wave is out of the ring
  asm volatile("" ::: "memory");
  if ((p.o_row_stride & 7) == 0 && ((size_t)p.out & 15) == 0 && (p.o_batch_stride & 7) == 0) {
    unsigned char* stg = smem + wave * (16 * C::OROW);
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
      uint2 pk;
      pk.x = pack_bf2(o[db][0] * inv, o[db][1] * inv);
      pk.y = pack_bf2(o[db][2] * inv, o[db][3] * inv);
      *(uint2*)(stg + r16 * C::OROW + (16 * db + 4 * g) * 2) = pk;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");            // wave-private region: no barrier
#pragma unroll
    for (int i = 0; i < (16 * C::CPR) / 64; ++i) {
      const int pc = i * 64 + lane;
      const int row = pc / C::CPR, c = pc % C::CPR;
      const uint4 v = *(const uint4*)(stg + row * C::OROW + c * 16);
      if (q0 + row < p.Sq) *(uint4*)(O + (size_t)(q0 + row) * p.o_row_stride + c * 8) = v;
    }
  } else {
    const int q = q0 + r16;
    if (q < p.Sq) {
      uint16_t* op = O + (size_t)q * p.o_row_stride;
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
        uint2 pk;
        pk.x = pack_bf2(o[db][0] * inv, o[db][1] * inv);
        pk.y = pack_bf2(o[db][2] * inv, o[db][3] * inv);
        *(uint2*)(op + 16 * db + 4 * g) = pk;
      }
    }
  }
#endif  // __HIP_DEVICE_COMPILE__
}

template <int D>
int launch(const da_attention_params& p, hipStream_t s) {
  auto kern = attn_wide_kernel<D>;
  static bool attr_set = false;   // per instantiation
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, Cfg<D>::RING) != hipSuccess) return DA_ERR_LAUNCH;
    attr_set = true;
  }
  const long long grid = (long long)p.B * p.H * ((p.Sq + kQB - 1) / kQB);
  if (grid > 0x7fffffffLL) return DA_ERR_UNSUPPORTED;
  DA_LAUNCH(kern, dim3((unsigned)grid), dim3(64 * kNW), (uint32_t)Cfg<D>::RING, s, p);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

}  // namespace da_attn_wide

// Entry used by da_attention_bf16 (attention.hip) for D = 256 / 384 / 512.  This is the only kernel of these head sizes: a mask or a
// pinned variant of the other generations is DA_ERR_UNSUPPORTED, and so are operands beyond the 31-bit byte offsets of the staging.
// kv_split / split_ws are ignored (no key split here).
int da_attn_wide_dispatch(const da_attention_params& p, hipStream_t s) {
  if (p.bias || p.causal) return DA_ERR_UNSUPPORTED;
  if (p.algo != 0 || p.ring_slots != 0 || p.q_block != 0 || p.pv_delay != 0) return DA_ERR_UNSUPPORTED;
  if ((size_t)p.Skv_alloc * (size_t)p.k_row_stride * 2 + (size_t)da_attn_wide::kKT * p.k_row_stride * 2 >= 0x7fffffffull) return DA_ERR_UNSUPPORTED;
  if ((size_t)p.D * (size_t)p.vt_ld * 2 + (size_t)p.Skv_alloc * 2 >= 0x7fffffffull) return DA_ERR_UNSUPPORTED;
  switch (p.D) {
    case 256: return da_attn_wide::launch<256>(p, s);
    case 384: return da_attn_wide::launch<384>(p, s);
    case 512: return da_attn_wide::launch<512>(p, s);
  }
  return DA_ERR_UNSUPPORTED;
}
