// Tiled AutoencoderKL.decode (models/autoencoders/autoencoder_kl.py tiled_decode / blend_v / blend_h): one launch per tile that
// reads the tile's conv_out result where the conv left it, blends it with its finished upper and left neighbours, and writes the
// finished pixels once -- cropped, in the type and layout the caller asked for, at their place in the full image.
//
// Reference, per tile pair and row y < min(a.rows, b.rows, E) (blend_h: the same along x):
//   b[:, :, y, :] = a[:, :, -E + y, :] * (1 - y / E) + b[:, :, y, :] * (y / E)            -- three bf16 torch ops
// = bf16(bf16(float(a) * w0) + bf16(float(b) * w1)) with w0 = float32(1 - y / E), w1 = float32(y / E) evaluated in double: the two
// weights come from a host table [E][2] (1.0f - (float)y / E in fp32 is another number when E is no power of two).  The vertical
// blend comes first, the horizontal blend works on its result; the neighbours are the tiles AFTER their own blends (`fin` of an
// earlier launch), so a corner depends on the upper neighbour's horizontal blend.  A NaN result (inf * 0, inf - inf) is stored as
// 0x7FC0 (torch's scalar fp32 -> bf16 conversion stores that, its vectorised CPU one 0xFFFF); a pixel no blend touches keeps its bits.
//
// One thread per pixel of the tile, C <= 4 channels.  Every load is unconditional from a clamped address and a select drops what
// does not apply (never `cond ? *p : 0`): a pixel outside the blend bands reads row / column 0 of the band and ignores it, a missing
// neighbour is replaced by the source's own first element.  All loads of a pixel are issued before its arithmetic.  Where the
// source is channels-last with 8-byte aligned pixels (the implicit-GEMM route of conv_thin_out: sC == 1, sP == 16) its <= 4
// channels are one 8-byte load.  BLEND == false (no neighbour, or E == 0) is the plain crop-and-place and loads the source only.
// One grid row per sample and a 32-bit pixel index inside the tile (no 64-bit division); every offset is size_t: a 4096 x 4096 x 3 x 2
// image is past 2^31 bytes in fp32.
#include "common.cuh"

namespace {

__device__ __forceinline__ uint16_t rbf_bits(float v) { return v != v ? (uint16_t)0x7FC0 : f2bf(v); }

// bf16(bf16(a * w0) + bf16(b * w1)), nothing contracted
__device__ __forceinline__ uint16_t blend_bits(uint16_t a, uint16_t b, float w0, float w1) {
  const float pa = bf2f(rbf_bits(__fmul_rn(bf2f(a), w0)));
  const float pb = bf2f(rbf_bits(__fmul_rn(bf2f(b), w1)));
  return rbf_bits(__fadd_rn(pa, pb));
}

struct TileArgs {
  const uint16_t* src;      // the tile's conv_out result: element (b, c, p) at b sB + c sC + p sP, p = y w + x
  long long sB, sC, sP;
  const uint16_t* up;       // finished upper tile, NCHW bf16 [B][C][hu][w], or the source (never read through then)
  const uint16_t* left;     // finished left tile, NCHW bf16 [B][C][h][wl], or the source
  const float* wt;          // [E][2] = (w0, w1)
  uint16_t* fin;            // NCHW bf16 [B][C][h][w] or NULL
  void* img;                // the full image
  int C, h, w, hu, wl, E;
  int ev, eh;               // rows / columns that blend: min(hu, h, E) with an upper tile, min(wl, w, E) with a left one, else 0
  int keep_h, keep_w;
  long long IH, IW, y0, x0;
};

template <int MODE, bool BLEND, bool VEC>
__global__ __launch_bounds__(256) void vae_tile_blend_kernel(const TileArgs a) {
  // grid: x over the tile's pixels (a 32-bit index: h w < 2^31 is checked by the host), y = the sample; only the offsets are 64-bit
  const unsigned hw = (unsigned)a.h * (unsigned)a.w, uw = (unsigned)a.w;
  const size_t b = blockIdx.y;
  for (unsigned p = blockIdx.x * 256u + threadIdx.x; p < hw; p += gridDim.x * 256u) {
    const int y = (int)(p / uw), x = (int)(p - (unsigned)y * uw);
    uint16_t s[4], u[4], l[4];
    float wv0 = 0.f, wv1 = 0.f, wh0 = 0.f, wh1 = 0.f;
    const bool bv = BLEND && y < a.ev, bh = BLEND && x < a.eh;
    // ---- loads ----
    const size_t soff = b * (size_t)a.sB + (size_t)p * (size_t)a.sP;
    if (VEC) {
      const uint2 q = *(const uint2*)(a.src + soff);
      s[0] = (uint16_t)(q.x & 0xffffu), s[1] = (uint16_t)(q.x >> 16), s[2] = (uint16_t)(q.y & 0xffffu), s[3] = (uint16_t)(q.y >> 16);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) s[c] = a.src[soff + (size_t)(c < a.C ? c : a.C - 1) * (size_t)a.sC];
    }
    if (BLEND) {
      const bool has_up = a.ev > 0, has_left = a.eh > 0;
      const size_t yu = bv ? (size_t)(a.hu - a.E + y) : 0, xu = has_up ? (size_t)x : 0;
      const size_t xl = bh ? (size_t)(a.wl - a.E + x) : 0, yl = has_left ? (size_t)y : 0;
      const size_t bu = has_up ? b : 0, bl = has_left ? b : 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const size_t cc = (size_t)(c < a.C ? c : a.C - 1);
        const size_t cu = has_up ? cc : 0, cl = has_left ? cc : 0;
        u[c] = a.up[((bu * a.C + cu) * (size_t)a.hu + yu) * (size_t)a.w + xu];
        l[c] = a.left[((bl * a.C + cl) * (size_t)a.h + yl) * (size_t)a.wl + xl];
      }
      const float2 wv = *(const float2*)(a.wt + 2 * (bv ? y : 0));
      const float2 wh = *(const float2*)(a.wt + 2 * (bh ? x : 0));
      wv0 = wv.x, wv1 = wv.y, wh0 = wh.x, wh1 = wh.y;
    }
    // ---- blend, store ----
    const bool kept = y < a.keep_h && x < a.keep_w;
    const size_t Y = (size_t)(a.y0 + y), X = (size_t)(a.x0 + x);
    const size_t pix = (b * (size_t)a.IH + Y) * (size_t)a.IW + X;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c >= a.C) break;
      uint16_t v = s[c];
      if (BLEND) {
        const uint16_t tv = blend_bits(u[c], v, wv0, wv1);
        v = bv ? tv : v;
        const uint16_t th = blend_bits(l[c], v, wh0, wh1);
        v = bh ? th : v;
      }
      if (a.fin) a.fin[((b * a.C + c) * (size_t)a.h + (size_t)y) * (size_t)a.w + (size_t)x] = v;
      if (kept) {
        const size_t plane = ((b * a.C + c) * (size_t)a.IH + Y) * (size_t)a.IW + X;
        if (MODE < 0) {
          ((uint16_t*)a.img)[plane] = v;
        } else {
          const float o = fminf(fmaxf(bf2f(v) * 0.5f + 0.5f, 0.f), 1.f);
          if (MODE == 0) ((float*)a.img)[plane] = o;
          else if (MODE == 1) ((float*)a.img)[pix * a.C + c] = o;
          else ((uint8_t*)a.img)[pix * a.C + c] = (uint8_t)rintf(o * 255.f);
        }
      }
    }
  }
}

template <int MODE>
void launch_mode(const TileArgs& a, bool blend, bool vec, const dim3& blocks, hipStream_t s) {
#define DA_TILE(B_, V_) DA_LAUNCH((vae_tile_blend_kernel<MODE, B_, V_>), blocks, dim3(256), 0, s, a)
  if (blend) { if (vec) DA_TILE(true, true); else DA_TILE(true, false); }
  else { if (vec) DA_TILE(false, true); else DA_TILE(false, false); }
#undef DA_TILE
}

// ---- tiled AutoencoderKL.encode (autoencoder_kl.py _tiled_encode): the moments of one encoded tile -------------------------------
// One launch per tile does everything between the tile's conv_out and the assembled moments: quant_conv (as
// posterior_latents_kernel: p[o] = bf16(bq[o] + sum_k wq[o][k] x[k]), k ascending, fp32 fma, one rounding), the vertical blend
// against the finished upper tile, the horizontal blend against the finished left tile on the vertical blend's result (blend_bits:
// the rounding points and the NaN rule above), `fin` for the tiles that come later and the kept rectangle at its place in the NCHW
// moments tensor.  One thread per latent pixel holds all C2 = 2 L channels of it; the house rules above apply: every load
// unconditional from a clamped address with a select afterwards, all loads of a pixel before its arithmetic, size_t offsets, a
// 32-bit pixel index.  VEC: a channels-last source (sC == 1) whose pixels are 16-byte aligned is read as C2 / 8 16-byte loads -- the
// 16-padded result of the thin conv_out (C2 = 8) and the NHWC result of the 16-channel VAEs' conv_out (C2 = 32) both are.  The
// quant_conv weights live in registers (C2 = 8 only, as in the posterior kernel).
struct MomentsArgs {
  const uint16_t* src;      // the tile's conv_out result: element (b, c, p) at b sB + c sC + p sP, p = y w + x
  long long sB, sC, sP;
  const uint16_t* wq;       // [C2][C2], QC only
  const uint16_t* bq;       // [C2]
  const uint16_t* up;       // finished upper tile, NCHW bf16 [B][C2][hu][w], or the source (never read through then)
  const uint16_t* left;     // finished left tile, NCHW bf16 [B][C2][h][wl], or the source
  const float* wt;          // [E][2] = (w0, w1)
  uint16_t* fin;            // NCHW bf16 [B][C2][h][w] or NULL
  uint16_t* out;            // the assembled moments, NCHW bf16 [B][C2][HL][WL]
  int h, w, hu, wl, E;
  int ev, eh;               // rows / columns that blend
  int keep_h, keep_w;
  long long HL, WL, y0, x0;
};

template <int C2, bool QC, bool BLEND, bool VEC>
__global__ __launch_bounds__(256) void vae_moments_tile_blend_kernel(const MomentsArgs a) {
  static_assert(C2 % 8 == 0 && (!QC || C2 == 8), "whole 16-byte groups; a quant_conv in registers at C2 = 8 only");
  // quant_conv weights and bias, loaded once per thread before the pixel loop (uniform addresses: scalar loads)
  float wf[QC ? C2 * C2 : 1], bfv[QC ? C2 : 1];
  if (QC) {
#pragma unroll
    for (int j = 0; j < C2 * C2; ++j) wf[j] = bf2f(a.wq[j]);
#pragma unroll
    for (int o = 0; o < C2; ++o) bfv[o] = bf2f(a.bq[o]);
  }
  const unsigned hw = (unsigned)a.h * (unsigned)a.w, uw = (unsigned)a.w;
  const size_t b = blockIdx.y;
  for (unsigned p = blockIdx.x * 256u + threadIdx.x; p < hw; p += gridDim.x * 256u) {
    const int y = (int)(p / uw), x = (int)(p - (unsigned)y * uw);
    uint16_t s[C2], u[BLEND ? C2 : 1], l[BLEND ? C2 : 1];
    float wv0 = 0.f, wv1 = 0.f, wh0 = 0.f, wh1 = 0.f;
    const bool bv = BLEND && y < a.ev, bh = BLEND && x < a.eh;
    // ---- loads ----
    const size_t soff = b * (size_t)a.sB + (size_t)p * (size_t)a.sP;
    if (VEC) {
#pragma unroll
      for (int g = 0; g < C2 / 8; ++g) {
        const uint4 q = *(const uint4*)(a.src + soff + 8 * g);
        const uint32_t r[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) s[8 * g + 2 * k] = (uint16_t)(r[k] & 0xffffu), s[8 * g + 2 * k + 1] = (uint16_t)(r[k] >> 16);
      }
    } else {
#pragma unroll
      for (int c = 0; c < C2; ++c) s[c] = a.src[soff + (size_t)c * (size_t)a.sC];
    }
    if (BLEND) {
      const bool has_up = a.ev > 0, has_left = a.eh > 0;
      const size_t yu = bv ? (size_t)(a.hu - a.E + y) : 0, xu = has_up ? (size_t)x : 0;
      const size_t xl = bh ? (size_t)(a.wl - a.E + x) : 0, yl = has_left ? (size_t)y : 0;
      const size_t bu = has_up ? b : 0, bl = has_left ? b : 0;
#pragma unroll
      for (int c = 0; c < C2; ++c) {
        const size_t cu = has_up ? (size_t)c : 0, cl = has_left ? (size_t)c : 0;
        u[c] = a.up[((bu * C2 + cu) * (size_t)a.hu + yu) * (size_t)a.w + xu];
        l[c] = a.left[((bl * C2 + cl) * (size_t)a.h + yl) * (size_t)a.wl + xl];
      }
      const float2 wv = *(const float2*)(a.wt + 2 * (bv ? y : 0));
      const float2 wh = *(const float2*)(a.wt + 2 * (bh ? x : 0));
      wv0 = wv.x, wv1 = wv.y, wh0 = wh.x, wh1 = wh.y;
    }
    // ---- quant_conv, blend, store ----
    uint16_t pm[C2];
    if (QC) {
#pragma unroll
      for (int o = 0; o < C2; ++o) {
        float acc = bfv[o];
#pragma unroll
        for (int k = 0; k < C2; ++k) acc = fmaf(wf[o * C2 + k], bf2f(s[k]), acc);
        pm[o] = f2bf(acc);
      }
    } else {
#pragma unroll
      for (int o = 0; o < C2; ++o) pm[o] = s[o];
    }
    const bool kept = y < a.keep_h && x < a.keep_w;
    const size_t Y = (size_t)(a.y0 + y), X = (size_t)(a.x0 + x);
#pragma unroll
    for (int c = 0; c < C2; ++c) {
      uint16_t v = pm[c];
      if (BLEND) {
        const uint16_t tv = blend_bits(u[c], v, wv0, wv1);
        v = bv ? tv : v;
        const uint16_t th = blend_bits(l[c], v, wh0, wh1);
        v = bh ? th : v;
      }
      if (a.fin) a.fin[((b * C2 + c) * (size_t)a.h + (size_t)y) * (size_t)a.w + (size_t)x] = v;
      if (kept) a.out[((b * C2 + c) * (size_t)a.HL + Y) * (size_t)a.WL + X] = v;
    }
  }
}

template <int C2, bool QC>
void launch_moments(const MomentsArgs& a, bool blend, bool vec, const dim3& blocks, hipStream_t s) {
#define DA_MTILE(B_, V_) DA_LAUNCH((vae_moments_tile_blend_kernel<C2, QC, B_, V_>), blocks, dim3(256), 0, s, a)
  if (blend) { if (vec) DA_MTILE(true, true); else DA_MTILE(true, false); }
  else { if (vec) DA_MTILE(false, true); else DA_MTILE(false, false); }
#undef DA_MTILE
}

}  // namespace

extern "C" int da_vae_moments_tile_blend(const void* src, long long sB, long long sC, long long sP, const void* wq, const void* bq,
                                         const void* up, int hu, const void* left, int wl, const void* weights, int E, void* fin,
                                         void* moments, int B, int L, int h, int w, int keep_h, int keep_w, long long moments_h,
                                         long long moments_w, long long y0, long long x0, void* stream) {
  if (B > 65535 || (long long)h * w > 0x7fffffffLL) return DA_ERR_INVALID;                      // grid y = B, 32-bit pixel index
  if (!src || !moments || B <= 0 || L <= 0 || h <= 0 || w <= 0 || E < 0 || sB < 0 || sC < 0 || sP < 0) return DA_ERR_INVALID;
  if (!wq != !bq) return DA_ERR_INVALID;                                                       // quant_conv: weight and bias, or neither
  if ((up && hu < E) || (left && wl < E) || (up && hu <= 0) || (left && wl <= 0)) return DA_ERR_INVALID;
  if (keep_h <= 0 || keep_w <= 0 || keep_h > h || keep_w > w) return DA_ERR_INVALID;
  if (moments_h <= 0 || moments_w <= 0 || y0 < 0 || x0 < 0 || y0 + keep_h > moments_h || x0 + keep_w > moments_w) return DA_ERR_INVALID;
  const bool blend = E > 0 && (up || left);
  if (blend && !weights) return DA_ERR_INVALID;
  if (L != 4 && !(L == 16 && !wq)) return DA_ERR_UNSUPPORTED;    // as da_vae_posterior_latents: 32 x 32 weights per thread would spill
  MomentsArgs a;
  a.src = (const uint16_t*)src, a.sB = sB, a.sC = sC, a.sP = sP;
  a.wq = (const uint16_t*)wq, a.bq = (const uint16_t*)bq;
  a.up = up ? (const uint16_t*)up : (const uint16_t*)src;
  a.left = left ? (const uint16_t*)left : (const uint16_t*)src;
  a.wt = (const float*)weights;
  a.fin = (uint16_t*)fin, a.out = (uint16_t*)moments;
  a.h = h, a.w = w, a.hu = up ? hu : 0, a.wl = left ? wl : 0, a.E = E;
  a.ev = up ? (hu < h ? (hu < E ? hu : E) : (h < E ? h : E)) : 0;
  a.eh = left ? (wl < w ? (wl < E ? wl : E) : (w < E ? w : E)) : 0;
  a.keep_h = keep_h, a.keep_w = keep_w, a.HL = moments_h, a.WL = moments_w, a.y0 = y0, a.x0 = x0;
  // 16-byte loads: channels-last, every pixel 16-byte aligned; exactly the 2 L channels are read, so nothing past them need exist
  const bool vec = sC == 1 && sP >= 2 * L && (sP & 7) == 0 && (sB & 7) == 0 && ((uintptr_t)src & 15) == 0;
  const long long nb = ((long long)h * w + 255) / 256;
  const dim3 blocks((unsigned)(nb < 65535 * 16 ? nb : 65535 * 16), (unsigned)B);
  hipStream_t s = (hipStream_t)stream;
  if (L == 16) launch_moments<32, false>(a, blend, vec, blocks, s);
  else if (wq) launch_moments<8, true>(a, blend, vec, blocks, s);
  else launch_moments<8, false>(a, blend, vec, blocks, s);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

extern "C" int da_vae_tile_blend(const void* src, long long sB, long long sC, long long sP, const void* up, int hu, const void* left,
                                 int wl, const void* weights, int E, void* fin, void* image, int B, int C, int h, int w, int keep_h,
                                 int keep_w, long long image_h, long long image_w, long long y0, long long x0, int mode,
                                 void* stream) {
  if (B > 65535 || (long long)h * w > 0x7fffffffLL) return DA_ERR_INVALID;                      // grid y = B, 32-bit pixel index
  if (!src || !image || B <= 0 || C < 1 || C > 4 || h <= 0 || w <= 0 || E < 0 || sB < 0 || sC < 0 || sP < 0) return DA_ERR_INVALID;
  if ((up && hu < E) || (left && wl < E) || (up && hu <= 0) || (left && wl <= 0)) return DA_ERR_INVALID;
  if (keep_h <= 0 || keep_w <= 0 || keep_h > h || keep_w > w) return DA_ERR_INVALID;
  if (image_h <= 0 || image_w <= 0 || y0 < 0 || x0 < 0 || y0 + keep_h > image_h || x0 + keep_w > image_w) return DA_ERR_INVALID;
  if (mode < -1 || mode > 2) return DA_ERR_INVALID;
  const bool blend = E > 0 && (up || left);
  if (blend && !weights) return DA_ERR_INVALID;
  TileArgs a;
  a.src = (const uint16_t*)src, a.sB = sB, a.sC = sC, a.sP = sP;
  a.up = up ? (const uint16_t*)up : (const uint16_t*)src;
  a.left = left ? (const uint16_t*)left : (const uint16_t*)src;
  a.wt = (const float*)weights;
  a.fin = (uint16_t*)fin, a.img = image;
  a.C = C, a.h = h, a.w = w, a.hu = up ? hu : 0, a.wl = left ? wl : 0, a.E = E;
  a.ev = up ? (hu < h ? (hu < E ? hu : E) : (h < E ? h : E)) : 0;
  a.eh = left ? (wl < w ? (wl < E ? wl : E) : (w < E ? w : E)) : 0;
  a.keep_h = keep_h, a.keep_w = keep_w, a.IH = image_h, a.IW = image_w, a.y0 = y0, a.x0 = x0;
  // one 8-byte load per pixel: channels-last, every pixel 8-byte aligned, and the 4 channels read lie inside the pixel's own slot
  // (the header's contract: such a source holds whole slots, so channel 3 of the last pixel exists also when C < 4)
  const bool vec = sC == 1 && sP >= 4 && (sP & 3) == 0 && (sB & 3) == 0 && ((uintptr_t)src & 7) == 0;
  const long long nb = ((long long)h * w + 255) / 256;
  const dim3 blocks((unsigned)(nb < 65535 * 16 ? nb : 65535 * 16), (unsigned)B);
  hipStream_t s = (hipStream_t)stream;
  if (mode < 0) launch_mode<-1>(a, blend, vec, blocks, s);
  else if (mode == 0) launch_mode<0>(a, blend, vec, blocks, s);
  else if (mode == 1) launch_mode<1>(a, blend, vec, blocks, s);
  else launch_mode<2>(a, blend, vec, blocks, s);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
