// AutoencoderTiny (TAESD / TAESDXL / TAEF1) on gfx950: the 64 -> 64 channel 3x3 conv with bias + residual + ReLU that is all of
// the model's trunk, and the head of its decoder.
//
// Reference (diffusers src/diffusers/models/autoencoders/vae.py): AutoencoderTinyBlock
//   conv = Sequential(Conv3x3(c, c), ReLU, Conv3x3(c, c), ReLU, Conv3x3(c, c));  forward = relu(conv(x) + skip(x))
// and DecoderTiny.forward = layers(tanh(x / 3) * 3) * 2 - 1 (autoencoder_tiny.py decodes latents / scaling_factor).
//
// conv_c64_kernel (da_gemm_bf16 with act == DA_ACT_RELU): out = max(bf16(acc + bias + residual), 0) on channels-last bf16.
//   * The whole weight, [64][9 * 64] bf16 = 72 KiB, stays in LDS for the life of a workgroup; the grid is at most one workgroup per
//     CU and each walks output tiles of 8 rows x 32 pixels (grid-stride), so the weight is fetched once per CU and not once per tile.
//   * 512 threads = 8 waves, wave w owns row w of the tile: 64 channels x 32 pixels = two 32 x 32 accumulators of
//     v_mfma_f32_32x32x16_bf16 with the WEIGHT as the A operand and the ACTIVATION as the B operand, so a lane ends up with 4
//     consecutive output channels of one pixel (8-byte loads of bias / residual, 8-byte stores), as in gemm_kernel.cuh.
//   * The tile's input is its 10 x 34 pixel halo, staged once in LDS and read by all nine taps.  Halo pixels outside the image are
//     loaded from the clamped in-image address, unconditionally, and replaced by zeros with a select when they are written to LDS
//     (never `cond ? *p : 0`).  The next tile's halo is loaded into registers (6 x 16 bytes per thread) before the MFMA loop of the
//     current one and written to LDS after it: one LDS image, HBM latency behind 72 MFMAs per wave.  The lane's 8 x 8 bytes of
//     residual are loaded ahead of the same loop.
//   * LDS rows are padded by 16 bytes (weight rows 1152 -> 1168, halo pixels 128 -> 144): consecutive rows then start 9 sixteen-byte
//     slots apart, a permutation of the 16 slots of the 256-byte bank row, so every 16-lane group of a ds_read_b128 is conflict free.
//   * k_valid in [1, 16] (the decoder's conv_in: 4 or 16 latent channels, zero padded to 64 in both operands) runs one 16-channel
//     MFMA step per tap instead of four; other values run all four (multiplying the zero padding changes nothing).
//   * No scratch; every global offset is size_t (B H W 64 passes 2^31 elements at 4096 x 4096 x 2).
//
// tiny_vae_latents_in_kernel (da_tiny_vae_latents_in): NCHW latents -> the padded NHWC input of the first conv, with the pipeline's
// latents / scaling_factor (+ shift_factor) and DecoderTiny's tanh(x / 3) * 3 at the reference's rounding points (fp32 arithmetic,
// every torch op's result rounded to bf16).
#include "common.cuh"

namespace da_c64 {

constexpr int TH = 8, TW = 32;                       // output tile (rows x pixels); one row per wave
constexpr int HALO_H = TH + 2, HALO_W = TW + 2;
constexpr int THREADS = 64 * TH;
constexpr int PIX_BYTES = 64 * 2 + 16;               // halo pixel in LDS: 64 channels + one 16-byte slot of padding
constexpr int WROW_BYTES = 576 * 2 + 16;             // weight row in LDS: 9 taps x 64 channels + one slot of padding
constexpr int W_BYTES = 64 * WROW_BYTES;             // 74 752
constexpr int HALO_BYTES = HALO_H * HALO_W * PIX_BYTES;   // 48 960
constexpr int LDS_BYTES = W_BYTES + HALO_BYTES;      // 123 712 of the CU's 163 840
constexpr int HALO_CHUNKS = HALO_H * HALO_W * 8;     // 16-byte chunks of the halo: 2 720
constexpr int HALO_REGS = (HALO_CHUNKS + THREADS - 1) / THREADS;   // 6 per thread
constexpr int W_CHUNKS = 64 * 72;                    // 16-byte chunks of the weight: 4 608 = 9 per thread
static_assert(W_CHUNKS % THREADS == 0, "the weight copy has no tail");
static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");

struct Tile {
  int b, y0, x0;
};
__device__ __forceinline__ Tile tile_of(int t, int tiles_x, int tiles_y) {
  const int per_image = tiles_x * tiles_y;
  const int b = t / per_image, r = t - b * per_image;
  const int ty = r / tiles_x;
  return {b, ty * TH, (r - ty * tiles_x) * TW};
}

// The halo of tile `tl` -> registers: chunk c = tid + i * THREADS is 16 bytes (8 channels) of halo pixel c / 8.  Bit i of the
// returned mask: the pixel lies inside the image (outside: the load reads the clamped pixel and the value is dropped at the LDS
// write).  Chunks past the halo's end (the last register of the high threads) repeat the last chunk and are not written.
__device__ __forceinline__ unsigned load_halo(const uint16_t* __restrict__ x, const Tile& tl, int H, int W, int tid,
                                              uint4 (&v)[HALO_REGS]) {
  unsigned inside = 0;
#pragma unroll
  for (int i = 0; i < HALO_REGS; ++i) {
    int c = tid + i * THREADS;
    c = c < HALO_CHUNKS ? c : HALO_CHUNKS - 1;
    const int p = c >> 3, q = c & 7;
    const int hy = p / HALO_W, hx = p - hy * HALO_W;
    const int iy = tl.y0 + hy - 1, ix = tl.x0 + hx - 1;
    const bool ok = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
    const int cy = min(max(iy, 0), H - 1), cx = min(max(ix, 0), W - 1);
    const size_t off = (((size_t)tl.b * (size_t)H + (size_t)cy) * (size_t)W + (size_t)cx) * 64 + (size_t)q * 8;
    v[i] = *(const uint4*)(x + off);
    inside |= (ok ? 1u : 0u) << i;
  }
  return inside;
}

__device__ __forceinline__ void store_halo(unsigned char* halo, int tid, const uint4 (&v)[HALO_REGS], unsigned inside) {
#pragma unroll
  for (int i = 0; i < HALO_REGS; ++i) {
    const int c = tid + i * THREADS;
    const bool ok = (inside >> i) & 1u;
    uint4 o;
    o.x = ok ? v[i].x : 0u; o.y = ok ? v[i].y : 0u; o.z = ok ? v[i].z : 0u; o.w = ok ? v[i].w : 0u;
    if (c < HALO_CHUNKS) *(uint4*)(halo + (c >> 3) * PIX_BYTES + (c & 7) * 16) = o;
  }
}

// max(bf16(v), 0) as bf16 bits: negative values and -0 give +0, NaN stays NaN (torch.relu)
__device__ __forceinline__ float relu_rounded(float v) {
  const float r = bf2f(f2bf(v));
  return (r > 0.0f || r != r) ? r : 0.0f;
}

// NCS: 16-channel MFMA steps per tap (4: all 64 input channels; 1: k_valid <= 16)
template <int NCS>
__global__ __launch_bounds__(THREADS, 2) void conv_c64_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ w,
                                                              const uint16_t* __restrict__ bias, const uint16_t* __restrict__ residual,
                                                              uint16_t* __restrict__ out, int H, int W, int tiles_x, int tiles_y,
                                                              int tiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* const wl = smem;
  unsigned char* const halo = smem + W_BYTES;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;

  int t = blockIdx.x;                                  // (the host launches no more workgroups than tiles)
  Tile tl = tile_of(t, tiles_x, tiles_y);
  uint4 hv[HALO_REGS];
  unsigned inside = load_halo(x, tl, H, W, tid, hv);
  {
    uint4 wv[W_CHUNKS / THREADS];
#pragma unroll
    for (int i = 0; i < W_CHUNKS / THREADS; ++i) wv[i] = *(const uint4*)(w + (size_t)(tid + i * THREADS) * 8);
#pragma unroll
    for (int i = 0; i < W_CHUNKS / THREADS; ++i) {
      const int c = tid + i * THREADS, row = c / 72, q = c - row * 72;
      *(uint4*)(wl + row * WROW_BYTES + q * 16) = wv[i];
    }
  }
  // this lane's bias: channels mt * 32 + 8 g + 4 h + {0 .. 3} (the C / D layout of the 32 x 32 MFMA)
  float bv[2][4][4];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      uint2 b2 = make_uint2(0u, 0u);
      if (bias) b2 = *(const uint2*)(bias + mt * 32 + 8 * g + 4 * h);
      bv[mt][g][0] = bf_lo(b2.x); bv[mt][g][1] = bf_hi(b2.x); bv[mt][g][2] = bf_lo(b2.y); bv[mt][g][3] = bf_hi(b2.y);
    }
  const unsigned char* const a_lane = wl + r * WROW_BYTES + h * 16;                         // A: weight row r (+ 32), k = 8 h + j
  const unsigned char* const b_lane = halo + (wave * HALO_W + r) * PIX_BYTES + h * 16;      // B: pixel r of row `wave`, same k

  for (;;) {
    store_halo(halo, tid, hv, inside);
    __syncthreads();
    const Tile cur = tl;
    const int tn = t + gridDim.x;
    if (tn < tiles) {                                  // (uniform) the next tile's halo, in flight under the MFMA loop
      tl = tile_of(tn, tiles_x, tiles_y);
      inside = load_halo(x, tl, H, W, tid, hv);
    }
    // this lane's output pixel; its residual is loaded here, ahead of the MFMA loop that hides the latency
    const int oy = cur.y0 + wave, ox = cur.x0 + r;
    const bool live = oy < H && ox < W;
    const size_t o = (((size_t)cur.b * (size_t)H + (size_t)min(oy, H - 1)) * (size_t)W + (size_t)min(ox, W - 1)) * 64 + (size_t)(4 * h);
    uint2 rv[2][4];
    if (residual) {                                    // (uniform; a lane off the image reads the clamped pixel and stores nothing)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int g = 0; g < 4; ++g) rv[mt][g] = *(const uint2*)(residual + o + mt * 32 + 8 * g);
    }
    f32x16_t acc0 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16_t acc1 = acc0;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - 3 * ky;
#pragma unroll
      for (int cs = 0; cs < NCS; ++cs) {
        const bf16x8_t bf = *(const bf16x8_t*)(b_lane + (ky * HALO_W + kx) * PIX_BYTES + cs * 32);
        const bf16x8_t a0 = *(const bf16x8_t*)(a_lane + (tap * 64 + cs * 16) * 2);
        const bf16x8_t a1 = *(const bf16x8_t*)(a_lane + 32 * WROW_BYTES + (tap * 64 + cs * 16) * 2);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, bf, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, bf, acc1, 0, 0, 0);
      }
    }
    if (live) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float v[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = (mt ? acc1[4 * g + j] : acc0[4 * g + j]) + bv[mt][g][j];
          if (residual) {
            v[0] += bf_lo(rv[mt][g].x); v[1] += bf_hi(rv[mt][g].x); v[2] += bf_lo(rv[mt][g].y); v[3] += bf_hi(rv[mt][g].y);
          }
          *(uint2*)(out + o + mt * 32 + 8 * g) = make_uint2(pack_bf2(relu_rounded(v[0]), relu_rounded(v[1])),
                                                            pack_bf2(relu_rounded(v[2]), relu_rounded(v[3])));
        }
    }
    if (tn >= tiles) break;
    t = tn;
    __syncthreads();                                   // every wave has read the halo: it may be overwritten
  }
}

int launch(const da_gemm_params& p, hipStream_t s) {
  if (!p.A || !p.W || !p.C) return DA_ERR_INVALID;
  const bool shape = p.conv == 3 && p.stride == 1 && p.up == 0 && p.pad == 1 && p.C1 == 64 && p.C2 == 0 && !p.A2 && p.N == 64 &&
                     p.K == 576 && p.ldw == 576 && p.ldc == 64 && p.tile == DA_TILE_AUTO && p.Hin > 0 && p.Win > 0 &&
                     p.Hout == p.Hin && p.Wout == p.Win && p.M > 0 && p.M % (p.Hin * p.Win) == 0;
  const bool plain = !p.rowvec && !p.gate && !p.bias_rows && p.split_k <= 1 && !p.stats_out && !p.ln_stats && !p.vt && !p.xa_k &&
                     !p.xa_vt && !p.out_f32 && (p.alpha == 0.0f || p.alpha == 1.0f) && (p.out_scale == 0.0f || p.out_scale == 1.0f) &&
                     p.k_valid >= 0 && p.k_valid <= 64 && (!p.residual || (p.ldr == 64 && p.residual != p.C));
  // 16-byte loads of x and w, 8-byte accesses of bias, residual and out
  const bool aligned = !(((uintptr_t)p.A | (uintptr_t)p.W) & 15) && !(((uintptr_t)p.C | (uintptr_t)p.residual | (uintptr_t)p.bias) & 7);
  if (!shape || !plain || !aligned) return DA_ERR_UNSUPPORTED;
  const int B = p.M / (p.Hin * p.Win), H = p.Hin, W = p.Win;
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  const long long tiles = (long long)B * tiles_x * tiles_y;
  if (tiles > 0x7fffffffLL) return DA_ERR_UNSUPPORTED;
  int cus = 256;
  {
    static int cached = 0;
    if (!cached) {
      int dev = 0, n = 0;
      if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
        cached = n;
      else
        cached = 256;
    }
    cus = cached;
  }
  const int grid = (int)(tiles < cus ? tiles : cus);
  const bool narrow = p.k_valid > 0 && p.k_valid <= 16;
  auto kern = narrow ? conv_c64_kernel<1> : conv_c64_kernel<4>;
  static bool attr_set[2] = {false, false};
  if (!attr_set[narrow]) {
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) != hipSuccess) return DA_ERR_LAUNCH;
    attr_set[narrow] = true;
  }
  DA_LAUNCH(kern, dim3(grid), dim3(THREADS), LDS_BYTES, s, (const uint16_t*)p.A, (const uint16_t*)p.W, (const uint16_t*)p.bias,
            (const uint16_t*)p.residual, (uint16_t*)p.C, H, W, tiles_x, tiles_y, (int)tiles);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

namespace {

__device__ __forceinline__ float rbf(float v) { return bf2f(f2bf(v)); }

// one thread per 16-byte chunk of the output: pixel i / 8, channels 8 (i % 8) .. + 7
__global__ __launch_bounds__(256) void tiny_vae_latents_in_kernel(const uint16_t* __restrict__ x, uint16_t* __restrict__ y, int L,
                                                                  long long HW, long long total, float in_div, float in_add, float m) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long pix = i >> 3;
    const int c0 = (int)(i & 7) * 8;
    const long long b = pix / HW, p = pix - b * HW;
    if (c0 >= L) {                                      // a chunk of padding only
      *(uint4*)(y + (size_t)i * 8) = make_uint4(0u, 0u, 0u, 0u);
      continue;
    }
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + j;
      const int cc = c < L ? c : L - 1;                 // (clamped, unconditional load; the padding channels are zeros)
      float v = bf2f(x[((size_t)b * (size_t)L + (size_t)cc) * (size_t)HW + (size_t)p]);
      if (in_div != 1.0f) v = rbf(__fdiv_rn(v, in_div));
      if (in_add != 0.0f) v = rbf(__fadd_rn(v, in_add));
      v = rbf(__fdiv_rn(v, m));
      v = rbf(tanhf(v));
      v = rbf(__fmul_rn(v, m));
      f[j] = c < L ? v : 0.0f;
    }
    *(uint4*)(y + (size_t)i * 8) = pack8(f);
  }
}

}  // namespace
}  // namespace da_c64

extern "C" int da_tiny_vae_latents_in(const void* x, void* y, int B, int L, int H, int W, float in_div, float in_add, float magnitude,
                                      void* stream) {
  if (!x || !y || B <= 0 || H <= 0 || W <= 0 || L < 1 || L > 16 || in_div == 0.0f || magnitude == 0.0f || ((uintptr_t)y & 15))
    return DA_ERR_INVALID;
  const long long HW = (long long)H * W, total = (long long)B * HW * 8;
  long long blocks = (total + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  DA_LAUNCH(da_c64::tiny_vae_latents_in_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x,
            (uint16_t*)y, L, HW, total, in_div, in_add, magnitude);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
