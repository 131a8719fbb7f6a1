// FreeU (models/unets/unet_2d_blocks.py up blocks with resolution_idx 0 and 1, utils/torch_utils.py apply_freeu / fourier_filter), on
// the channels-last pair (hidden, skip) that ResnetBlock2D reads in place of the reference's concat:
//   hidden[..., :Cx/2] <- bf16(float(hidden) * b)                                   one fp32 multiply, one rounding
//   skip_out           <- bf16(ifftn(ifftshift(mask * fftshift(fftn(float(skip))))).real)     mask = s on a 2 x 2 box, 1 elsewhere
// fftshift puts frequency k at position k + H / 2 (even and odd H alike), so the box [H/2 - 1, H/2] x [W/2 - 1, W/2] is the four bins
// {-1, 0} x {-1, 0}: the filter is x plus (s - 1) times the projection of x on those bins.  No FFT runs here.  With t_h = 2 pi h / H,
// p_w = 2 pi w / W, g = s - 1 and real x, per (image, channel) plane:
//   S0 = sum x      Ac = sum x cos t_h      As = sum x sin t_h      Bc = sum x cos p_w      Bs = sum x sin p_w
//   Cc = sum x cos(t_h + p_w)               Cs = sum x sin(t_h + p_w)
//   y[h][w] = bf16(x + g / (H W) (S0 + Ac cos t_h + As sin t_h + Bc cos p_w + Bs sin p_w + Cc cos(t_h + p_w) + Cs sin(t_h + p_w)))
// fp32 throughout, one rounding at the end.  Both halves are separable and computed that way:
//   reduce  per row (segment): r0 = sum_w x, rc = sum_w x cos p_w, rs = sum_w x sin p_w (three FMAs per element), folded into the seven
//           sums with the row's twiddles: Cc += cos t_h rc - sin t_h rs, Cs += sin t_h rc + cos t_h rs
//   apply   per row: P = S0 + Ac cos t_h + As sin t_h, Qc = Bc + Cc cos t_h + Cs sin t_h, Qs = Bs - Cc sin t_h + Cs cos t_h, then
//           y = bf16(x + g / (H W) (P + Qc cos p_w + Qs sin p_w))  (three FMAs per element)
// The twiddles come from the host (evaluated in double, rounded to fp32): [cos t_h (H) | sin t_h (H) | cos p_w (W) | sin p_w (W)].
// H = 2 (frequency -1 is Nyquist there) needs no special case; H == 1 or W == 1 (the two bins coincide) is refused.
//
// Work split.  A workgroup of 256 threads owns (image, slab of `sw` contiguous channels, band of rows).  A lane holds 8 channels (one
// 16-byte access); the 2^lcg >= sw / 8 neighbouring lanes cover the slab's channels of one pixel (sw = 32: one 64-byte run), the other
// thread-index bits number `256 >> lcg` row workers.  A worker walks units (row, segment of the row): rows are cut into nseg segments
// where the band has fewer rows than there are workers, so that no worker idles.  Its per-unit chains are at most one row long; the
// units of a worker, the workers of a wave (xor butterfly over the lanes of one channel group: every lane ends with the same bits),
// the four waves (through LDS, in wave order) and -- two-launch path -- the bands (ascending) combine in that fixed order.  No
// atomics: the result is a function of the inputs and the geometry alone.
//   resident path (one launch): the band is the whole plane and the slab H x W x sw is loaded ONCE into LDS (16-byte accesses, lanes of
//           one pixel side by side: conflict-free); reduce and apply both run out of LDS, one global read and one global write.
//   two-launch path: freeu_reduce_kernel writes per-band partials [B][bands][7][Cs] fp32 to the workspace; freeu_apply_kernel sums
//           a slab's bands in ascending order and applies.  The skip is read twice (the second time out of the memory-side cache).
// The hidden half-scale rides in the first launch on further workgroups of the grid (blockIdx.x >= nskip): a grid-stride loop over
// 16-byte units of the first Cx / 2 channels of every pixel.
#include "common.cuh"

namespace {

constexpr int FREEU_THREADS = 256;
constexpr int FREEU_MAX_BANDS = 32;
constexpr int FREEU_LDS_LIMIT = 144 * 1024;
constexpr int FREEU_FILL = 256;           // the chip's CUs: bands are cut until a launch has this many workgroups

struct FreeuGeom {
  int resident;
  int sw, nslab, lcg;      // slab width in channels, slabs per image, log2 of the lanes that cover one pixel of a slab
  int rpb, bands;          // rows per band, bands per plane (resident: H, 1)
  int nseg, seglen;        // segments per row, their length
  unsigned tw_floats;      // LDS: the twiddles, padded to 16 bytes
  size_t lds;
};

struct FreeuArgs {
  uint16_t* hidden;
  const uint16_t* skip;
  uint16_t* out;
  const float* tw;
  float* ws;
  int B, H, W, Cx, Cs;
  unsigned nskip;          // workgroups of the skip part of the grid
  float b, gn;             // gn = (s - 1) / (H W), evaluated in double
  FreeuGeom g;
};

// 0 = fine, else a DA_ERR_* code.  path: 0 = automatic, 1 = resident, 2 = two launches.
int freeu_geom(int B, int H, int W, int Cs, int path, FreeuGeom* g) {
  if (B <= 0 || H <= 0 || W <= 0 || Cs <= 0 || path < 0 || path > 2) return DA_ERR_INVALID;
  if ((long long)H * W > 0x7fffffffLL) return DA_ERR_INVALID;                // 32-bit pixel index inside a plane
  if ((Cs & 7) || H == 1 || W == 1 || H + W > 4096) return DA_ERR_UNSUPPORTED;   // (H + W: the twiddles live in LDS)
  g->tw_floats = (unsigned)((2 * H + 2 * W + 3) & ~3);
  const long long hw = (long long)H * W;
  auto fixed = [&](int sw) { return (size_t)g->tw_floats * 4 + (size_t)4 * 7 * (sw <= 8 ? 8 : sw <= 16 ? 16 : sw <= 32 ? 32 : 64) * 4; };
  // a slab is at least 32 channels (whole 64-byte runs of a pixel) where the tensor has them; 64 where the plane fits and the slabs
  // alone still fill the chip
  int sw = Cs < 32 ? Cs : 32;
  bool fits = (size_t)hw * sw * 2 + fixed(sw) <= (size_t)FREEU_LDS_LIMIT;
  if (path != 2 && Cs >= 64 && (size_t)hw * 64 * 2 + fixed(64) <= (size_t)FREEU_LDS_LIMIT && (long long)B * ((Cs + 63) / 64) >= FREEU_FILL)
    sw = 64, fits = true;
  if (path == 1 && !fits) return DA_ERR_UNSUPPORTED;
  g->resident = path == 2 ? 0 : fits;
  g->sw = sw, g->nslab = (Cs + sw - 1) / sw;
  g->lcg = sw <= 8 ? 0 : sw <= 16 ? 1 : sw <= 32 ? 2 : 3;
  if (g->resident) {
    g->rpb = H, g->bands = 1;
  } else {
    const long long planes = (long long)B * g->nslab;
    long long want = (FREEU_FILL + planes - 1) / planes;
    const int cap = H < FREEU_MAX_BANDS ? H : FREEU_MAX_BANDS;
    if (want > cap) want = cap;
    g->rpb = (H + (int)want - 1) / (int)want;
    g->bands = (H + g->rpb - 1) / g->rpb;
  }
  const int nrw = FREEU_THREADS >> g->lcg;
  int nseg = 1;
  while ((long long)g->rpb * nseg * 2 <= nrw && W / (nseg * 2) >= 8) nseg *= 2;
  g->nseg = nseg, g->seglen = (W + nseg - 1) / nseg;
  g->lds = fixed(sw) + (g->resident ? (size_t)hw * sw * 2 : 0);
  if ((long long)B * g->nslab * g->bands > 0x3fffffffLL) return DA_ERR_INVALID;
  return 0;
}

// what a thread is in its workgroup
struct FreeuLane {
  int cg, rw, nrw, ncg;    // channel group, row worker, workers, channel groups of THIS slab (the last slab may be narrower)
  bool active;             // cg < ncg
  size_t base;             // element offset of (image, pixel 0, the lane's first channel) in skip / out
  int h0, rows;            // the band
  unsigned plane, band;    // (image, slab) number; band number
  int c;                   // the lane's first channel
};

__device__ __forceinline__ FreeuLane freeu_lane(const FreeuArgs& a) {
  FreeuLane l;
  const FreeuGeom& g = a.g;
  const unsigned wg = blockIdx.x;
  l.band = wg % (unsigned)g.bands;
  const unsigned rest = wg / (unsigned)g.bands;
  const unsigned slab = rest % (unsigned)g.nslab, img = rest / (unsigned)g.nslab;
  l.plane = rest;
  l.cg = (int)(threadIdx.x & ((1u << g.lcg) - 1u));
  l.rw = (int)(threadIdx.x >> g.lcg);
  l.nrw = FREEU_THREADS >> g.lcg;
  const int c0 = (int)slab * g.sw;
  const int left = a.Cs - c0;
  l.ncg = (left < g.sw ? left : g.sw) >> 3;
  l.active = l.cg < l.ncg;
  l.c = c0 + 8 * (l.active ? l.cg : 0);
  l.base = (size_t)img * (size_t)a.H * (size_t)a.W * (size_t)a.Cs + (size_t)l.c;
  l.h0 = (int)l.band * g.rpb;
  l.rows = a.H - l.h0 < g.rpb ? a.H - l.h0 : g.rpb;
  return l;
}

template <bool RES>
__device__ __forceinline__ uint4 freeu_px(const FreeuArgs& a, const FreeuLane& l, const uint4* slab, int p) {
  if (RES) return slab[p * l.ncg + l.cg];
  return *(const uint4*)(a.skip + l.base + (size_t)p * (size_t)a.Cs);
}

// the lane's share of the seven sums of its 8 channels over the band: acc[k][j], k = S0 Ac As Bc Bs Cc Cs
template <bool RES>
__device__ __forceinline__ void freeu_reduce(const FreeuArgs& a, const FreeuLane& l, const uint4* slab, const float* tw, float (&acc)[7][8]) {
  const FreeuGeom& g = a.g;
  const float* thc = tw, *ths = tw + a.H, *pwc = tw + 2 * a.H, *pws = tw + 2 * a.H + a.W;
#pragma unroll
  for (int k = 0; k < 7; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;
  if (!l.active) return;
  const int units = l.rows * g.nseg;
  for (int u = l.rw; u < units; u += l.nrw) {
    const int hr = u / g.nseg, sg = u - hr * g.nseg;
    const int h = l.h0 + hr, w0 = sg * g.seglen, w1 = w0 + g.seglen < a.W ? w0 + g.seglen : a.W;
    float r0[8], rc[8], rs[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r0[j] = rc[j] = rs[j] = 0.f;
#pragma unroll 4
    for (int w = w0; w < w1; ++w) {
      float f[8];
      unpack8(freeu_px<RES>(a, l, slab, h * a.W + w), f);
      const float c = pwc[w], s = pws[w];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        r0[j] += f[j];
        rc[j] = fmaf(f[j], c, rc[j]);
        rs[j] = fmaf(f[j], s, rs[j]);
      }
    }
    const float ch = thc[h], sh = ths[h];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      acc[0][j] += r0[j];
      acc[1][j] = fmaf(ch, r0[j], acc[1][j]);
      acc[2][j] = fmaf(sh, r0[j], acc[2][j]);
      acc[3][j] += rc[j];
      acc[4][j] += rs[j];
      acc[5][j] = fmaf(-sh, rs[j], fmaf(ch, rc[j], acc[5][j]));
      acc[6][j] = fmaf(ch, rs[j], fmaf(sh, rc[j], acc[6][j]));
    }
  }
}

// workers of a wave (butterfly over the lanes of one channel group), then the four waves in wave order through `comb`
// [4][7][8 << lcg]: afterwards every thread holds the workgroup's sums of its 8 channels.  Every thread of the workgroup comes here.
__device__ __forceinline__ void freeu_combine(const FreeuArgs& a, const FreeuLane& l, float* comb, float (&acc)[7][8]) {
  const int ncgp = 1 << a.g.lcg, nc = 8 << a.g.lcg;
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
#pragma unroll
  for (int k = 0; k < 7; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = acc[k][j];
      for (int o = ncgp; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
      acc[k][j] = v;
    }
  if (lane < ncgp) {
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      float4* d = (float4*)(comb + (wave * 7 + k) * nc + 8 * l.cg);
      d[0] = make_float4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
      d[1] = make_float4(acc[k][4], acc[k][5], acc[k][6], acc[k][7]);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 7; ++k) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;
#pragma unroll
    for (int wv = 0; wv < 4; ++wv) {
      const float4* d = (const float4*)(comb + (wv * 7 + k) * nc + 8 * l.cg);
      const float4 lo = d[0], hi = d[1];
      acc[k][0] += lo.x, acc[k][1] += lo.y, acc[k][2] += lo.z, acc[k][3] += lo.w;
      acc[k][4] += hi.x, acc[k][5] += hi.y, acc[k][6] += hi.z, acc[k][7] += hi.w;
    }
  }
}

template <bool RES>
__device__ __forceinline__ void freeu_apply(const FreeuArgs& a, const FreeuLane& l, const uint4* slab, const float* tw,
                                            const float (&sum)[7][8]) {
  const FreeuGeom& g = a.g;
  const float* thc = tw, *ths = tw + a.H, *pwc = tw + 2 * a.H, *pws = tw + 2 * a.H + a.W;
  if (!l.active) return;
  const int units = l.rows * g.nseg;
  for (int u = l.rw; u < units; u += l.nrw) {
    const int hr = u / g.nseg, sg = u - hr * g.nseg;
    const int h = l.h0 + hr, w0 = sg * g.seglen, w1 = w0 + g.seglen < a.W ? w0 + g.seglen : a.W;
    const float ch = thc[h], sh = ths[h];
    float P[8], Qc[8], Qs[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      P[j] = fmaf(sum[2][j], sh, fmaf(sum[1][j], ch, sum[0][j]));
      Qc[j] = fmaf(sum[6][j], sh, fmaf(sum[5][j], ch, sum[3][j]));
      Qs[j] = fmaf(sum[6][j], ch, fmaf(-sum[5][j], sh, sum[4][j]));
    }
#pragma unroll 4
    for (int w = w0; w < w1; ++w) {
      const int p = h * a.W + w;
      float f[8], o[8];
      unpack8(freeu_px<RES>(a, l, slab, p), f);
      const float c = pwc[w], s = pws[w];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = fmaf(a.gn, fmaf(Qs[j], s, fmaf(Qc[j], c, P[j])), f[j]);
      *(uint4*)(a.out + l.base + (size_t)p * (size_t)a.Cs) = pack8(o);
    }
  }
}

// hidden[..., :Cx/2] *= b, in place: 16-byte units, Cx / 16 per pixel
__device__ __forceinline__ void freeu_scale_hidden(const FreeuArgs& a) {
  const unsigned upp = (unsigned)a.Cx >> 4;
  const unsigned long long units = (unsigned long long)a.B * (unsigned)a.H * (unsigned)a.W * upp;
  const unsigned long long step = (unsigned long long)(gridDim.x - a.nskip) * FREEU_THREADS;
  for (unsigned long long u = (unsigned long long)(blockIdx.x - a.nskip) * FREEU_THREADS + threadIdx.x; u < units; u += step) {
    const unsigned long long px = u / upp;
    const unsigned k = (unsigned)(u - px * upp);
    uint4* q = (uint4*)(a.hidden + (size_t)px * (size_t)a.Cx + 8u * k);
    float f[8];
    unpack8(*q, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = __fmul_rn(f[j], a.b);
    *q = pack8(f);
  }
}

__device__ __forceinline__ void freeu_load_twiddles(const FreeuArgs& a, float* tw) {
  for (int i = (int)threadIdx.x; i < 2 * a.H + 2 * a.W; i += FREEU_THREADS) tw[i] = a.tw[i];
}

__global__ __launch_bounds__(FREEU_THREADS) void freeu_resident_kernel(const FreeuArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if (blockIdx.x >= a.nskip) { freeu_scale_hidden(a); return; }
  float* tw = (float*)smem;
  float* comb = tw + a.g.tw_floats;
  uint4* slab = (uint4*)(comb + 4 * 7 * (8 << a.g.lcg));
  const FreeuLane l = freeu_lane(a);
  freeu_load_twiddles(a, tw);
  if (l.active) {
    const int hw = a.H * a.W;
    for (int p = l.rw; p < hw; p += l.nrw) slab[p * l.ncg + l.cg] = *(const uint4*)(a.skip + l.base + (size_t)p * (size_t)a.Cs);
  }
  __syncthreads();
  float acc[7][8];
  freeu_reduce<true>(a, l, slab, tw, acc);
  freeu_combine(a, l, comb, acc);
  freeu_apply<true>(a, l, slab, tw, acc);
}

__global__ __launch_bounds__(FREEU_THREADS) void freeu_reduce_kernel(const FreeuArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if (blockIdx.x >= a.nskip) { freeu_scale_hidden(a); return; }
  float* tw = (float*)smem;
  float* comb = tw + a.g.tw_floats;
  const FreeuLane l = freeu_lane(a);
  freeu_load_twiddles(a, tw);
  __syncthreads();
  float acc[7][8];
  freeu_reduce<false>(a, l, nullptr, tw, acc);
  freeu_combine(a, l, comb, acc);
  if (l.rw == 0 && l.active) {
    // partials [B][bands][7][Cs]; l.plane / nslab = the image
    const size_t img = l.plane / (unsigned)a.g.nslab;
    float* d = a.ws + ((img * (size_t)a.g.bands + l.band) * 7) * (size_t)a.Cs + (size_t)l.c;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      float4* q = (float4*)(d + (size_t)k * (size_t)a.Cs);
      q[0] = make_float4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
      q[1] = make_float4(acc[k][4], acc[k][5], acc[k][6], acc[k][7]);
    }
  }
}

__global__ __launch_bounds__(FREEU_THREADS) void freeu_apply_kernel(const FreeuArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* tw = (float*)smem;
  const FreeuLane l = freeu_lane(a);
  freeu_load_twiddles(a, tw);
  __syncthreads();
  float sum[7][8];
#pragma unroll
  for (int k = 0; k < 7; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) sum[k][j] = 0.f;
  if (l.active) {
    const size_t img = l.plane / (unsigned)a.g.nslab;
    for (int bd = 0; bd < a.g.bands; ++bd) {                                   // ascending: the same order in every workgroup
      const float* d = a.ws + ((img * (size_t)a.g.bands + (size_t)bd) * 7) * (size_t)a.Cs + (size_t)l.c;
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        const float4* q = (const float4*)(d + (size_t)k * (size_t)a.Cs);
        const float4 lo = q[0], hi = q[1];
        sum[k][0] += lo.x, sum[k][1] += lo.y, sum[k][2] += lo.z, sum[k][3] += lo.w;
        sum[k][4] += hi.x, sum[k][5] += hi.y, sum[k][6] += hi.z, sum[k][7] += hi.w;
      }
    }
  }
  freeu_apply<false>(a, l, nullptr, tw, sum);
}

}  // namespace

extern "C" size_t da_freeu_workspace_bytes(int B, int H, int W, int Cs, int path) {
  FreeuGeom g;
  if (freeu_geom(B, H, W, Cs, path, &g) != 0 || g.resident) return 0;
  return (size_t)B * (size_t)g.bands * 7 * (size_t)Cs * sizeof(float);
}

extern "C" int da_freeu_nhwc_bf16(void* hidden, const void* skip, void* skip_out, const void* twiddles, void* workspace,
                                  long long workspace_bytes, int B, int H, int W, int Cx, int Cs, float b, float s, int path,
                                  void* stream) {
  if (!hidden || !skip || !skip_out || !twiddles || Cx <= 0 || workspace_bytes < 0) return DA_ERR_INVALID;
  if (!(b - b == 0.f) || !(s - s == 0.f)) return DA_ERR_INVALID;                                   // finite
  if (((uintptr_t)hidden | (uintptr_t)skip | (uintptr_t)skip_out | (uintptr_t)workspace) & 15 || ((uintptr_t)twiddles & 3))
    return DA_ERR_INVALID;
  FreeuArgs a;
  const int rc = freeu_geom(B, H, W, Cs, path, &a.g);
  if (rc) return rc;
  if (Cx & 15) return DA_ERR_UNSUPPORTED;
  const FreeuGeom& g = a.g;
  const size_t need = g.resident ? 0 : (size_t)B * (size_t)g.bands * 7 * (size_t)Cs * sizeof(float);
  if (need && (!workspace || (size_t)workspace_bytes < need)) return DA_ERR_INVALID;
  a.hidden = (uint16_t*)hidden, a.skip = (const uint16_t*)skip, a.out = (uint16_t*)skip_out;
  a.tw = (const float*)twiddles, a.ws = (float*)workspace;
  a.B = B, a.H = H, a.W = W, a.Cx = Cx, a.Cs = Cs;
  a.b = b, a.gn = (float)(((double)s - 1.0) / ((double)H * (double)W));
  a.nskip = (unsigned)((long long)B * g.nslab * g.bands);
  const unsigned long long hunits = (unsigned long long)B * (unsigned)H * (unsigned)W * ((unsigned)Cx >> 4);
  unsigned long long nh = (hunits + 4 * FREEU_THREADS - 1) / (4 * FREEU_THREADS);
  const unsigned nhid = (unsigned)(nh < 2048 ? nh : 2048);
  hipStream_t st = (hipStream_t)stream;
  if (g.resident) {
    static bool attr_set = false;
    if (!attr_set) {
      if (hipFuncSetAttribute((const void*)freeu_resident_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, FREEU_LDS_LIMIT) !=
          hipSuccess)
        return DA_ERR_LAUNCH;
      attr_set = true;
    }
    DA_LAUNCH(freeu_resident_kernel, dim3(a.nskip + nhid), dim3(FREEU_THREADS), (uint32_t)g.lds, st, a);
    DA_CHECK_LAUNCH();
    return DA_OK;
  }
  DA_LAUNCH(freeu_reduce_kernel, dim3(a.nskip + nhid), dim3(FREEU_THREADS), (uint32_t)g.lds, st, a);
  DA_CHECK_LAUNCH();
  DA_LAUNCH(freeu_apply_kernel, dim3(a.nskip), dim3(FREEU_THREADS), (uint32_t)g.tw_floats * 4, st, a);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
