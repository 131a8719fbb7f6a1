// The image branch of IP-Adapter's decoupled cross-attention on gfx950: for up to four adapters in ONE launch,
//   out[b, s, h, :] = bf16( float(out[b, s, h, :]) + sum_a scale_a softmax_n(sm_scale q[b, s, h] . k_a[b, n, h]) v_a[b, n, h, :] )
// in place on the output the text cross-attention has already written.  bf16 operands, D = 64 / 96 / 160 (the padded kernel head
// sizes of layers.kernel_head_dim for 40 / 64 / 80 / 160; the padded channels are zero in q, k and v), 1 <= N_a <= 32 image tokens.
//
// Call site: IPAdapterAttnProcessor2_0 (attention_processor.py), `hidden_states = hidden_states + scale * ip_hidden_states` for every
// adapter, between the text attention and to_out.  q and out are the [B*Sq][>= H*D] token matrices layers.Attention hands to and
// takes from ops.attention (head h at columns h D .. h D + D, own row strides); k_a / v_a are token-major [B*N_alloc_a][>= H*D], the
// two halves of one stacked to_k_ip | to_v_ip projection of the image tokens.  V is not transposed on the host.
//
// Work split.  Unlike the temporal kernel (one wave = one sequence with its own keys), thousands of queries share ONE tiny K / V per
// (batch, head), and the output is a read-modify-write.  A workgroup is kNW = 4 waves and owns one (batch, head) and 128 consecutive
// queries, 32 per wave.  Per adapter the workgroup stages that head's K (row-major, rows D + 8 elements apart) and V^T (rows
// kLdv = 40 elements apart, the key order of the second product) into LDS ONCE -- 32 x 160 x 2 operands x 2 B = 20 KiB at most, bank-
// padded 23 KiB -- between two barriers; the four waves then read their fragments from it.  One adapter is resident at a time: four
// adapters would be 92 KiB at D = 160 and cost the CU its second workgroup, and the two barriers per adapter are nothing beside the
// loads.  A wave keeps its Q fragments (D / 16 x 16 bytes per lane) and ONE fp32 accumulator (D / 32 tiles of 16 registers) over all
// adapters in registers, and touches `out` once: one 16-byte load per lane and row segment, add, one rounding, one 16-byte store.
//
// Grid: workgroup index = ((b H + h) nblk + blk), nblk = ceil(Sq / 128), the query blocks of one (batch, head) adjacent so that they
// find its K / V in the L2.  The smallest cross-attention level of SDXL (B = 2 under CFG, H = 20, Sq = 1024, D = 64) is 2 x 20 x 8 =
// 320 workgroups of 9.6 KiB LDS and 4 waves: all resident at once on 256 CUs (64 CUs hold two); SD 1.5's 8 x 8 level (B = 2, H = 8,
// Sq = 64, D = 160) is 16 workgroups of two live waves -- a launch-latency case whatever the split, 3 Sq D 2 = 61 KB per (b, h).
// The large levels are thousands of workgroups (SDXL 64 x 64: 2 x 10 x 32 = 640; SD 1.5 64 x 64: 2 x 8 x 32 = 512).
//
// The swapped products of attention_temporal.hip on v_mfma_f32_32x32x16_bf16 (lane = (c = lane & 31, hi = lane >> 5)):
//   S^T[kv][q] = K[kv][:] . Q[q][:]^T      A = K from LDS (lane (c, hi): the 16 bytes d = 16 ks + 8 hi .. + 7 of token c; the pitch
//                                          of D + 8 elements puts eight lanes' 16-byte reads on all 32 banks once: 144 / 208 / 336
//                                          bytes = 16 / 80 / 80 mod 128), B = Q from registers.
//   O^T[d][q]  = V^T[d][kv] . P^T[kv][q]   A = V^T from LDS, one 16-byte read per k-step, B = P^T: the S^T accumulators as they are.
// Lane (q, hi) ends the first product with the 16 keys kv(r) = 8 (r >> 2) + 4 hi + (r & 3) of ITS query; registers 8 ks .. 8 ks + 7
// are the B fragment of k-step ks of the second product, so V^T is stored with bits 2 and 3 of the key index swapped (pos()).  With
// N_a <= 16 the second k-step holds masked keys only and is skipped, and only 16 tokens are staged (workgroup-uniform).
//
// Loads: every global load is unconditional with a clamped index (queries >= Sq read row Sq - 1 and are never stored; tokens >= N_a
// read token N_a - 1), and V^T rows of tokens >= N_a are made zero with a select on the loaded value: P is zero there, and 0 x stale
// bits must not make a NaN.  K rows in [N_a, 16 or 32) hold a copy of the last token, and with N_a <= 16 rows 16 .. 31 are not staged
// at all: the first product reads stale LDS there.  Rows of the MFMA are independent and those scores are replaced by -inf with a
// select before the maximum, so whatever they hold reaches nothing.
//
// Arithmetic: scores in fp32; p = exp2(s sm_scale log2 e - m) in fp32; P is rounded to bf16 ONCE and the row sum l is the sum of the
// ROUNDED values (the temporal kernel's convention); P V accumulates in fp32 on the matrix pipe; acc += (scale_a / l) (P V) in fp32,
// adapters in index order; out = bf16(float(out) + acc), one rounding.  With one key P = l = 1 and the result is
// bf16(float(out) + scale v) exactly.  Nothing outside columns [0, H D) of the B Sq rows of out is written, nothing outside the named
// blocks is read.  No workspace, nothing shared between workgroups; the result depends on the inputs alone.
#include "common.cuh"

namespace da_attn_ip {

constexpr int kNW = 4;     // waves per workgroup, 32 queries each
constexpr int kLdv = 40;   // elements per V^T row in LDS: 32 keys + 8 (eight lanes' 16-byte reads cover the 32 banks once)

// position of key kv inside a V^T row: bits 2 and 3 swapped, so that the keys of lane half `hi` in k-step ks are 16 ks + 8 hi .. + 7
__device__ __forceinline__ int pos(int kv) { return (kv & 0x13) | ((kv & 8) >> 1) | ((kv & 4) << 1); }

template <int D>
__global__ __launch_bounds__(64 * kNW) void attn_ip_kernel(const da_attention_ip_params p) {
#if defined(__HIP_DEVICE_COMPILE__)
  static_assert(D == 64 || D == 96 || D == 160, "head sizes of the image-prompt kernel");
  constexpr int NKS = D / 16;    // k-steps of the first product
  constexpr int NDT = D / 32;    // 32-row output tiles of the second
  constexpr int CH = D / 8;      // 16-byte chunks of a head row
  constexpr int kLdk = D + 8;    // elements per K row in LDS
  __shared__ __attribute__((aligned(16))) uint16_t smem[32 * kLdk + D * kLdv];
  uint16_t* const ksm = smem;
  uint16_t* const vt = smem + 32 * kLdk;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 31, hi = lane >> 5;

  const int nblk = (p.Sq + 32 * kNW - 1) / (32 * kNW);
  const int bh = blockIdx.x / nblk, blk = blockIdx.x - bh * nblk;
  const int b = bh / p.H, h = bh - b * p.H;
  const int s = (blk * kNW + wave) * 32 + c;
  const bool qok = s < p.Sq;
  const size_t row = (size_t)b * p.Sq + (qok ? s : p.Sq - 1);      // clamped: a query past the end reads the last row, stores nothing
  const float sl2 = p.sm_scale * 1.4426950408889634f;

  uint4 qf[NKS];
  {
    const uint16_t* __restrict__ qp = (const uint16_t*)p.q + row * p.q_row_stride + h * D + 8 * hi;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = *(const uint4*)(qp + 16 * ks);
  }
  f32x16_t acc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[dt][r] = 0.f;

#pragma unroll
  for (int a = 0; a < DA_IP_MAX_ADAPTERS; ++a) {       // unrolled: the per-adapter fields are read at constant offsets
    if (a < p.A) {                                     // workgroup-uniform
      const int N = p.n[a];
      const int fw = N <= 16 ? 16 : 32;                // tokens staged, keys the second product walks
      const size_t tok0 = (size_t)b * p.n_alloc[a];
      const uint16_t* __restrict__ kg = (const uint16_t*)p.k[a] + tok0 * p.k_row_stride[a] + h * D;
      const uint16_t* __restrict__ vg = (const uint16_t*)p.v[a] + tok0 * p.v_row_stride[a] + h * D;

      __syncthreads();                                 // the previous adapter's fragment reads are done
      for (int i = tid; i < fw * CH; i += 64 * kNW) {  // K: a row's chunks on adjacent lanes, 16-byte LDS writes
        const int tok = i / CH, ch = i - tok * CH;
        const int tk = tok < N ? tok : N - 1;
        *(uint4*)(ksm + tok * kLdk + 8 * ch) = *(const uint4*)(kg + (size_t)tk * p.k_row_stride[a] + 8 * ch);
      }
      for (int i = tid; i < fw * CH; i += 64 * kNW) {  // V -> V^T: tokens on adjacent lanes, 2-byte scatter
        const int tok = i & (fw - 1), ch = i / fw;
        const int tk = tok < N ? tok : N - 1;
        uint4 x = *(const uint4*)(vg + (size_t)tk * p.v_row_stride[a] + 8 * ch);
        const bool live = tok < N;
        const uint32_t w[4] = {live ? x.x : 0u, live ? x.y : 0u, live ? x.z : 0u, live ? x.w : 0u};
        const int vp = pos(tok);
#pragma unroll
        for (int j = 0; j < 8; ++j) vt[(8 * ch + j) * kLdv + vp] = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
      }
      __syncthreads();

      // ---- S^T = K Q^T ----
      f32x16_t sacc;
#pragma unroll
      for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
      const uint16_t* krow = ksm + c * kLdk + 8 * hi;
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        const uint4 kf = *(const uint4*)(krow + 16 * ks);
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, kf), __builtin_bit_cast(bf16x8_t, qf[ks]), sacc, 0, 0, 0);
      }

      // ---- softmax over the keys of this lane's query: 16 in-lane, 16 in lane ^ 32 ----
      float sc[16];
      float m = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kv = 8 * (r >> 2) + 4 * hi + (r & 3);
        sc[r] = kv < N ? sacc[r] * sl2 : -INFINITY;
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
      const float wgt = p.scale[a] * (1.0f / l);       // l >= 1: the maximum's own term
      const bf16x8_t pf0 = __builtin_bit_cast(bf16x8_t, make_uint4(pk[0], pk[1], pk[2], pk[3]));
      const bf16x8_t pf1 = __builtin_bit_cast(bf16x8_t, make_uint4(pk[4], pk[5], pk[6], pk[7]));

      // ---- O^T = V^T P^T, weighted into the accumulator all adapters share ----
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        const uint16_t* vrow = vt + (32 * dt + c) * kLdv + 8 * hi;
        f32x16_t o;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] = 0.f;
        o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, *(const uint4*)vrow), pf0, o, 0, 0, 0);
        if (fw == 32)
          o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, *(const uint4*)(vrow + 16)), pf1, o, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[dt][r] += wgt * o[r];
      }
    }
  }

  // ---- out += acc.  Lane (q, hi): acc[dt][4 g + e] = O[q][32 dt + 8 g + 4 hi + e].  Halves trade 16-byte pieces of fp32: hi = 0 ends
  // with columns 16 j .. + 7 of the tile, hi = 1 with 16 j + 8 .. + 15, one 16-byte segment of the out row each.
  uint16_t* __restrict__ op = (uint16_t*)p.out + row * p.o_row_stride + h * D + 8 * hi;
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float f[8], cur[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float own = hi ? acc[dt][4 * (2 * j + 1) + e] : acc[dt][4 * (2 * j) + e];
        const float send = hi ? acc[dt][4 * (2 * j) + e] : acc[dt][4 * (2 * j + 1) + e];
        const float recv = __shfl_xor(send, 32, 64);
        f[e] = hi ? recv : own;
        f[4 + e] = hi ? own : recv;
      }
      uint16_t* seg = op + 32 * dt + 16 * j;
      // unconditional like every load here: a lane past the end reads the clamped last row, possibly while its owner stores it, and
      // throws the value away (qok guards the store)
      const uint4 old = *(const uint4*)seg;
      unpack8(old, cur);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] += cur[e];
      if (qok) *(uint4*)seg = pack8(f);
    }
  }
#endif  // __HIP_DEVICE_COMPILE__
}

template <int D>
int launch(const da_attention_ip_params& p, hipStream_t s) {
  const long long grid = (long long)p.B * p.H * ((p.Sq + 32 * kNW - 1) / (32 * kNW));
  if (grid > 0x7fffffffLL) return DA_ERR_UNSUPPORTED;
  DA_LAUNCH(attn_ip_kernel<D>, dim3((unsigned)grid), dim3(64 * kNW), 0, s, p);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

}  // namespace da_attn_ip

extern "C" int da_attention_ip_bf16(const da_attention_ip_params* p, void* stream) {
  if (!p || !p->q || !p->out) return DA_ERR_INVALID;
  if (p->A < 1 || p->A > DA_IP_MAX_ADAPTERS) return DA_ERR_UNSUPPORTED;
  for (int a = 0; a < p->A; ++a)
    if (!p->k[a] || !p->v[a]) return DA_ERR_INVALID;
  if (p->B < 1 || p->H < 1 || p->Sq < 1) return DA_ERR_UNSUPPORTED;
  if (p->D != 64 && p->D != 96 && p->D != 160) return DA_ERR_UNSUPPORTED;
  if (!(p->sm_scale == p->sm_scale)) return DA_ERR_UNSUPPORTED;
  const long long width = (long long)p->H * p->D;
  if ((long long)p->B * p->Sq > 0x7fffffffLL) return DA_ERR_UNSUPPORTED;
  // 16-byte loads and stores: rows of whole 8-element chunks from a 16-byte aligned base
  if (p->q_row_stride < width || (p->q_row_stride & 7) || ((uintptr_t)p->q & 15)) return DA_ERR_UNSUPPORTED;
  if (p->o_row_stride < width || (p->o_row_stride & 7) || ((uintptr_t)p->out & 15)) return DA_ERR_UNSUPPORTED;
  da_attention_ip_params live = *p;   // the adapters that contribute, in order: one with scale 0 is skipped
  live.A = 0;
  for (int a = 0; a < p->A; ++a) {
    if (p->n[a] < 1 || p->n[a] > 32 || p->n_alloc[a] < p->n[a]) return DA_ERR_UNSUPPORTED;
    if ((long long)p->B * p->n_alloc[a] > 0x7fffffffLL || !(p->scale[a] == p->scale[a])) return DA_ERR_UNSUPPORTED;
    if (p->k_row_stride[a] < width || (p->k_row_stride[a] & 7) || ((uintptr_t)p->k[a] & 15)) return DA_ERR_UNSUPPORTED;
    if (p->v_row_stride[a] < width || (p->v_row_stride[a] & 7) || ((uintptr_t)p->v[a] & 15)) return DA_ERR_UNSUPPORTED;
    if (p->scale[a] == 0.0f) continue;
    const int j = live.A++;
    live.k[j] = p->k[a], live.v[j] = p->v[a], live.n[j] = p->n[a], live.n_alloc[j] = p->n_alloc[a];
    live.k_row_stride[j] = p->k_row_stride[a], live.v_row_stride[j] = p->v_row_stride[a], live.scale[j] = p->scale[a];
  }
  if (live.A == 0) return DA_OK;      // all scales zero: nothing launches, out keeps its bits
  hipStream_t s = (hipStream_t)stream;
  switch (p->D) {
    case 64: return da_attn_ip::launch<64>(live, s);
    case 96: return da_attn_ip::launch<96>(live, s);
    case 160: return da_attn_ip::launch<160>(live, s);
  }
  return DA_ERR_UNSUPPORTED;
}
