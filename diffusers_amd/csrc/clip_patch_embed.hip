// The front of a CLIP vision transformer (transformers modeling_clip.py CLIPVisionEmbeddings + CLIPVisionTransformer.pre_layrnorm, with
// CLIPImageProcessor's centre crop, rescale and normalise in front of it) as ONE launch: image -> the first encoder layer's input.
//
// da_clip_patch_embed.  Image: `u8` mode, packed uint8 [B][Hs][Ws][3] (what da_resample_u8 writes) with a row stride, a crop origin
// (top, left) and mean[3] / inv_std[3]; or `f32` mode, float32 [B][3][S][S] pixel_values that are normalised already.  Weight: the
// P x P stride-P patch convolution (3 -> hidden, no bias) as [hidden][Kp] bf16, K = 3 P P in (c, i, j) order, zero-padded to Kp = ceil32(K)
// (ops.pack_clip_patch_weight).  G = S / P, S_alloc = ceil16(1 + G G).  Per image b:
//   e[0]      = class + pos[0]
//   e[1 + p]  = sum_k v[p][k] W[:][k] + pos[1 + p]          p = py G + px, v[p][(c, i, j)] = pixel (c, py P + i, px P + j) of the crop
//   x_out[b S_alloc + r]   = LayerNorm(e[r]) gamma + beta    r <= G G;   rows 1 + G G .. S_alloc - 1 are written as zeros
//   emb_out[b S_alloc + r] = e[r]                            (optional; the reference's hidden_states[0]); its padding rows are zeros too
// Arithmetic: a pixel is v = (u8 / 255 - mean_c) * inv_std_c in fp32 (`f32` mode: the given value), rounded to bf16 as the MFMA operand;
// fp32 accumulation over K; + pos in fp32; the LayerNorm's mean and its variance (two passes: sum, then sum of squared differences) in fp32
// over the un-rounded fp32 row; ONE rounding to bf16 per output element (emb_out rounds the pre-LayerNorm fp32 value).
//
// Split.  A workgroup of four waves owns 32 consecutive patches of one image and ALL hidden columns, so a row's LayerNorm statistics
// never leave the workgroup: grid = B * ceil(G G / 32).  Wave w owns columns [w hidden / 4, (w + 1) hidden / 4) as NT = hidden / 128
// tiles of 32 x 32 (v_mfma_f32_32x32x16_bf16; NT = 13 at hidden = 1664: 208 accumulator registers; one wave per SIMD has the whole
// 512-register file).  The MFMA "A" operand is the weight, "B" the activations: a lane (c = lane & 31, hi = lane >> 5) ends with patch
// p0 + c and 16 channels per tile.  A-row r of a tile is given channel hi(r) 16 + (r >> 3) 4 + (r & 3), hi(r) = (r >> 2) & 1 -- the
// lane picks which weight row it loads -- so that accumulator i of a lane is channel 16 hi + i: sixteen CONSECUTIVE channels, two 16-byte
// stores per tile, and pos / gamma / beta arrive as 16-byte loads.
//
// Activations.  The 32 x Kp tile is gathered once per workgroup into LDS, in chunks of at most 768 K (one chunk for P = 14 and 16, four
// for P = 32), 32 x (768 + 8) bf16 = 48.5 KiB.  An item is one pixel run (patch row r, channel c, kernel row i): P pixels that are
// contiguous in the source (3 bytes apart in HWC uint8), normalised and stored as bf16 at k = (c P + i) P + j.  Neighbouring lanes take
// neighbouring patches, so one load instruction of the wave walks one image row.  A patch index past the image's last is clamped to it:
// every load is unconditional and in bounds, the duplicate rows are computed and not stored.  Columns K .. Kp - 1 are zeroed.  The row
// pitch of chunk + 8 elements (1552 bytes = 16 mod 128) puts eight lanes' 16-byte reads on all 32 banks once.
//
// Weights stream from L2 straight into registers, 32 K a slab: lane (c, hi) loads the 32 contiguous bytes k = 32 s + 16 hi .. + 15 of its
// row (two lanes: one 64-byte piece of a row), the first 16 bytes feed the slab's first MFMA and the second 16 the second; the B
// fragment is read from LDS with the same k mapping (any K order is a valid one as long as both operands agree).  The next slab's
// weights are loaded before this slab's MFMAs issue (a register double buffer: 2 x 8 NT registers).
//
// Epilogue: + pos; per-row sum over the lane's 16 NT values, lane ^ 32, then over the four waves through LDS; the same for the squared
// differences; normalise, gamma / beta, stores.  The image's first workgroup also writes the class row (256 threads, 8 channels each,
// the same two-pass statistics) and the zero rows.  Nothing else is written.
#include "common.cuh"

namespace {

constexpr int CP_THREADS = 256;
constexpr int CP_ROWS = 32;                      // patches of a workgroup
constexpr int CP_KC = 768;                       // K of an activation chunk in LDS
constexpr int CP_PITCH = CP_KC + 8;              // elements of an LDS row
constexpr int CP_MAX_HIDDEN = 1664, CP_MAX_KP = 3072;

struct ClipPatchArgs {
  const unsigned char* image;                    // u8: bytes; f32: floats
  const uint16_t* w;
  const uint16_t* cls;
  const uint16_t* pos;
  const uint16_t* gamma;
  const uint16_t* beta;
  uint16_t* x_out;
  uint16_t* emb_out;
  long long img_batch_stride;                    // bytes
  long long img_row_stride;                      // bytes
  int u8, top, left;
  float mean[3], inv_std[3], eps;
  int S, P, G, hidden, K, Kp, S_alloc, x_ld, emb_ld, tiles;
};

__device__ __forceinline__ void cp_unpack16(const uint16_t* p, float* f) {
  unpack8(*(const uint4*)p, f);
  unpack8(*(const uint4*)(p + 8), f + 8);
}

// sum of `v` over the workgroup's four waves for the 32 rows of the tile: lane (c, hi) holds a partial of row c
__device__ __forceinline__ float cp_row_sum(float v, float (*red)[CP_ROWS], int wave, int c, int hi) {
  v += __shfl_xor(v, 32, 64);
  __syncthreads();                               // the previous use of `red` is over
  if (hi == 0) red[wave][c] = v;
  __syncthreads();
  return (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

// sum of `v` over all 256 threads
__device__ __forceinline__ float cp_block_sum(float v, float (*red)[CP_ROWS], int wave) {
  v = wave_sum(v);
  __syncthreads();
  red[wave][0] = v;
  __syncthreads();
  return (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
}

// slab `slab` (32 K) of the lane's weight row in each of the wave's NT tiles: 32 contiguous bytes a tile
template <int NT>
__device__ __forceinline__ void cp_load_w(uint4 (&w)[NT][2], const uint16_t* wrow, int Kp, int slab) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const uint16_t* p = wrow + (long long)t * 32 * Kp + 32 * slab;
    w[t][0] = *(const uint4*)p, w[t][1] = *(const uint4*)(p + 8);
  }
}

template <int NT>
__device__ __forceinline__ void cp_mma(f32x16_t (&acc)[NT], const uint4 (&w)[NT][2], const uint16_t* brow) {
  const bf16x8_t b0 = __builtin_bit_cast(bf16x8_t, *(const uint4*)brow);
  const bf16x8_t b1 = __builtin_bit_cast(bf16x8_t, *(const uint4*)(brow + 8));
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, w[t][0]), b0, acc[t], 0, 0, 0);
    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, w[t][1]), b1, acc[t], 0, 0, 0);
  }
}

template <int NT>
__global__ __launch_bounds__(CP_THREADS) void clip_patch_embed_kernel(const ClipPatchArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t act[CP_ROWS * CP_PITCH];
  __shared__ float red[4][CP_ROWS];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, hi = lane >> 5;
  const int tile = (int)(blockIdx.x % (unsigned)a.tiles);
  const long long b = blockIdx.x / (unsigned)a.tiles;
  const int np = a.G * a.G, p0 = tile * CP_ROWS;
  const int hidden = a.hidden, Kp = a.Kp, P = a.P;

  f32x16_t acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

  // the weight row of this lane in tile t: + t * 32 * Kp
  const int arow_ch = ((c >> 2) & 1) * 16 + (c >> 3) * 4 + (c & 3);
  const uint16_t* wrow = a.w + (long long)(wave * NT * 32 + arow_ch) * Kp + 16 * hi;
  const int slabs = Kp >> 5;
  uint4 wq[NT][2], wn[NT][2];
  cp_load_w<NT>(wq, wrow, Kp, 0);

  for (int k0 = 0; k0 < Kp; k0 += CP_KC) {
    const int kc = Kp - k0 < CP_KC ? Kp - k0 : CP_KC;                          // a multiple of 32
    if (k0) __syncthreads();                                                   // the MFMAs of the previous chunk have read it
    // ---- gather: pixel runs q = c P + i that meet [k0, k0 + kc) ----
    {
      const int q0 = k0 / P;
      int q1 = (k0 + kc - 1) / P;
      q1 = q1 > 3 * P - 1 ? 3 * P - 1 : q1;
      const int items = CP_ROWS * (q1 - q0 + 1);
      for (int item = tid; item < items; item += CP_THREADS) {
        const int r = item & (CP_ROWS - 1), q = q0 + (item >> 5);
        const int ch = q / P, i = q - ch * P;
        int p = p0 + r;
        p = p < np ? p : np - 1;
        const int py = p / a.G, px = p - py * a.G;
        const int kb = q * P - k0;                                             // chunk column of j = 0
        const int jlo = kb < 0 ? -kb : 0, jhi = kc - kb < P ? kc - kb : P;
        uint16_t* dst = act + r * CP_PITCH + kb;
        if (a.u8) {
          const unsigned char* src = a.image + b * a.img_batch_stride + (long long)(a.top + py * P + i) * a.img_row_stride +
                                     (long long)(a.left + px * P) * 3 + ch;
          const float m = ch == 0 ? a.mean[0] : ch == 1 ? a.mean[1] : a.mean[2];
          const float s = ch == 0 ? a.inv_std[0] : ch == 1 ? a.inv_std[1] : a.inv_std[2];
          for (int j = jlo; j < jhi; ++j) dst[j] = f2bf(((float)src[3 * j] / 255.0f - m) * s);
        } else {
          const float* src = (const float*)(a.image + b * a.img_batch_stride) + ((long long)ch * a.S + py * P + i) * a.S + px * P;
          for (int j = jlo; j < jhi; ++j) dst[j] = f2bf(src[j]);
        }
      }
      const int zlo = a.K - k0;                                                // columns K .. Kp - 1: zeros (at most 31, in the last chunk)
      if (zlo < kc) {
        const int nz = kc - (zlo < 0 ? 0 : zlo), z0 = kc - nz;
        for (int item = tid; item < CP_ROWS * nz; item += CP_THREADS) act[(item & (CP_ROWS - 1)) * CP_PITCH + z0 + (item >> 5)] = 0;
      }
    }
    __syncthreads();

    // ---- K loop over the chunk: 32 K a slab, two MFMAs per tile ----
    const uint16_t* brow = act + c * CP_PITCH + 16 * hi;
    const int s0 = k0 >> 5, ns = kc >> 5;
    int s = 0;
    for (; s + 1 < ns; s += 2) {                                               // ping-pong: no register copies
      cp_load_w<NT>(wn, wrow, Kp, s0 + s + 1);
      cp_mma<NT>(acc, wq, brow + 32 * s);
      cp_load_w<NT>(wq, wrow, Kp, s0 + s + 2 < slabs ? s0 + s + 2 : slabs - 1);  // past the end: the last slab again, no branch
      cp_mma<NT>(acc, wn, brow + 32 * (s + 1));
    }
    if (s < ns) {
      cp_load_w<NT>(wn, wrow, Kp, s0 + s + 1 < slabs ? s0 + s + 1 : slabs - 1);
      cp_mma<NT>(acc, wq, brow + 32 * s);
#pragma unroll
      for (int t = 0; t < NT; ++t) wq[t][0] = wn[t][0], wq[t][1] = wn[t][1];
    }
  }

  // ---- epilogue: lane (c, hi) holds patch p0 + c, channels col0 + 32 t + i ----
  const int p = p0 + c;
  const bool valid = p < np;
  const int pc = valid ? p : np - 1;
  const int col0 = wave * NT * 32 + 16 * hi;
  const long long orow = b * a.S_alloc + 1 + pc;
  const uint16_t* prow = a.pos + (long long)(1 + pc) * hidden + col0;
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    float f[16];
    cp_unpack16(prow + 32 * t, f);
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] += f[i], sum += acc[t][i];
    if (a.emb_out && valid) {
#pragma unroll
      for (int i = 0; i < 16; ++i) f[i] = acc[t][i];
      uint16_t* o = a.emb_out + orow * a.emb_ld + col0 + 32 * t;
      *(uint4*)o = pack8(f), *(uint4*)(o + 8) = pack8(f + 8);
    }
  }
  const float inv_n = 1.0f / (float)hidden;
  const float mean = cp_row_sum(sum, red, wave, c, hi) * inv_n;
  float sq = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float d = acc[t][i] - mean;
      acc[t][i] = d, sq += d * d;
    }
  const float rstd = 1.0f / sqrtf(cp_row_sum(sq, red, wave, c, hi) * inv_n + a.eps);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    float g[16], be[16], y[16];
    cp_unpack16(a.gamma + col0 + 32 * t, g);
    cp_unpack16(a.beta + col0 + 32 * t, be);
#pragma unroll
    for (int i = 0; i < 16; ++i) y[i] = acc[t][i] * rstd * g[i] + be[i];
    if (valid) {
      uint16_t* o = a.x_out + orow * a.x_ld + col0 + 32 * t;
      *(uint4*)o = pack8(y), *(uint4*)(o + 8) = pack8(y + 8);
    }
  }
  if (tile) return;

  // ---- the image's first workgroup: the class row and the zero rows ----
  const int c8 = hidden >> 3;                                                  // <= 208 threads carry 8 channels each
  const bool on = tid < c8;
  const int ch0 = on ? 8 * tid : 0;
  float e[8], f[8];
  unpack8(*(const uint4*)(a.cls + ch0), e);
  unpack8(*(const uint4*)(a.pos + ch0), f);
  float s1 = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) e[i] += f[i], s1 += e[i];
  const float cmean = cp_block_sum(on ? s1 : 0.f, red, wave) * inv_n;
  const long long crow = b * a.S_alloc;
  if (on && a.emb_out) *(uint4*)(a.emb_out + crow * a.emb_ld + ch0) = pack8(e);
  float s2 = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) e[i] -= cmean, s2 += e[i] * e[i];
  const float crstd = 1.0f / sqrtf(cp_block_sum(on ? s2 : 0.f, red, wave) * inv_n + a.eps);
  if (on) {
    float g[8], be[8];
    unpack8(*(const uint4*)(a.gamma + ch0), g);
    unpack8(*(const uint4*)(a.beta + ch0), be);
#pragma unroll
    for (int i = 0; i < 8; ++i) e[i] = e[i] * crstd * g[i] + be[i];
    *(uint4*)(a.x_out + crow * a.x_ld + ch0) = pack8(e);
  }
  const int zrows = a.S_alloc - 1 - np;
  for (int item = tid; item < zrows * c8; item += CP_THREADS) {
    const int zr = item / c8, zc = (item - zr * c8) * 8;
    const long long row = crow + 1 + np + zr;
    *(uint4*)(a.x_out + row * a.x_ld + zc) = make_uint4(0u, 0u, 0u, 0u);
    if (a.emb_out) *(uint4*)(a.emb_out + row * a.emb_ld + zc) = make_uint4(0u, 0u, 0u, 0u);
  }
}

template <int NT>
void cp_launch(const ClipPatchArgs& a, unsigned grid, hipStream_t st) {
  DA_LAUNCH(clip_patch_embed_kernel<NT>, dim3(grid), dim3(CP_THREADS), 0, st, a);
}

}  // namespace

extern "C" int da_clip_patch_embed(const void* image, int mode, int Hs, int Ws, int image_row_stride, int top, int left, float mean_r,
                                   float mean_g, float mean_b, float inv_std_r, float inv_std_g, float inv_std_b, const void* weight,
                                   const void* class_embedding, const void* position_embedding, const void* gamma, const void* beta,
                                   float eps, void* x_out, int x_ld, void* emb_out, int emb_ld, int B, int S, int P, int hidden,
                                   void* stream) {
  if (!image || !weight || !class_embedding || !position_embedding || !gamma || !beta || !x_out) return DA_ERR_INVALID;
  if (mode != DA_CLIP_IMAGE_U8 && mode != DA_CLIP_IMAGE_F32) return DA_ERR_INVALID;
  if (B <= 0 || S <= 0 || P <= 0 || hidden <= 0) return DA_ERR_UNSUPPORTED;
  if (hidden % 128 || hidden > CP_MAX_HIDDEN || S % P) return DA_ERR_UNSUPPORTED;
  const int K = 3 * P * P, Kp = (K + 31) & ~31;
  if (Kp > CP_MAX_KP) return DA_ERR_UNSUPPORTED;
  if (x_ld % 8 || x_ld < hidden || (emb_out && (emb_ld % 8 || emb_ld < hidden))) return DA_ERR_UNSUPPORTED;
  if (((uintptr_t)weight | (uintptr_t)class_embedding | (uintptr_t)position_embedding | (uintptr_t)gamma | (uintptr_t)beta |
       (uintptr_t)x_out | (uintptr_t)emb_out) & 15)
    return DA_ERR_UNSUPPORTED;
  ClipPatchArgs a;
  if (mode == DA_CLIP_IMAGE_U8) {
    if (Hs <= 0 || Ws <= 0 || image_row_stride < 3 * Ws || top < 0 || left < 0 || top > Hs - S || left > Ws - S) return DA_ERR_UNSUPPORTED;
    a.img_row_stride = image_row_stride, a.img_batch_stride = (long long)Hs * image_row_stride;
  } else {
    if ((uintptr_t)image & 3) return DA_ERR_UNSUPPORTED;
    a.img_row_stride = 4LL * S, a.img_batch_stride = 12LL * S * S;
  }
  const int G = S / P;
  if ((long long)G * G > 0x7fffffLL) return DA_ERR_UNSUPPORTED;
  a.tiles = (G * G + CP_ROWS - 1) / CP_ROWS;
  if ((long long)B * a.tiles > 0x7fffffffLL) return DA_ERR_UNSUPPORTED;
  a.image = (const unsigned char*)image, a.w = (const uint16_t*)weight, a.cls = (const uint16_t*)class_embedding;
  a.pos = (const uint16_t*)position_embedding, a.gamma = (const uint16_t*)gamma, a.beta = (const uint16_t*)beta;
  a.x_out = (uint16_t*)x_out, a.emb_out = (uint16_t*)emb_out;
  a.u8 = mode == DA_CLIP_IMAGE_U8, a.top = top, a.left = left;
  a.mean[0] = mean_r, a.mean[1] = mean_g, a.mean[2] = mean_b;
  a.inv_std[0] = inv_std_r, a.inv_std[1] = inv_std_g, a.inv_std[2] = inv_std_b, a.eps = eps;
  a.S = S, a.P = P, a.G = G, a.hidden = hidden, a.K = K, a.Kp = Kp, a.S_alloc = (1 + G * G + 15) & ~15, a.x_ld = x_ld, a.emb_ld = emb_ld;
  const unsigned grid = (unsigned)(B * a.tiles);
  hipStream_t st = (hipStream_t)stream;
  switch (hidden / 128) {
#define CP_CASE(n) case n: cp_launch<n>(a, grid, st); break;
    CP_CASE(1) CP_CASE(2) CP_CASE(3) CP_CASE(4) CP_CASE(5) CP_CASE(6) CP_CASE(7) CP_CASE(8) CP_CASE(9) CP_CASE(10) CP_CASE(11)
    CP_CASE(12) CP_CASE(13)
#undef CP_CASE
    default: return DA_ERR_UNSUPPORTED;
  }
  DA_CHECK_LAUNCH();
  return DA_OK;
}
