// Image resizing in front of the VAE / ControlNet input path (image_processor.py VaeImageProcessor.resize).
//
// da_resample_u8: Pillow's 8-bit separable resample (Resample.c ImagingResampleHorizontal_8bpc / Vertical_8bpc) to the bit.  Packed
// uint8 [B][Hin][Win][C] -> [B][Hout][Wout][C], C = 1 or 3.  Per axis the host passes Pillow's own tables (ops.resample_tables):
//   coef   int32 [out][ksize]   weights in 22-bit fixed point
//   bounds int32 [out][2]       (xmin, xcount): the input samples output `o` reads
// and one output sample along an axis is
//   clip8((2^21 + sum_{i < xcount} in[xmin + i] * coef[o][i]) >> 22)          int32 sum, arithmetic shift, clamp to 0 .. 255
// The horizontal pass runs first and rounds to uint8; the vertical pass reads those bytes.  A pass whose input size equals its
// output size is skipped (its tables may be NULL).  Integer sums are order-independent: every split of the work -- either route,
// any tile -- gives the same bytes.
//
// One launch (route 1).  A workgroup of 256 threads owns an output tile of TH x TW pixels of one image:
//   1. ranges   from the vertical bounds of its rows it takes the input rows [r0, r0 + nrows) the tile needs, from the horizontal
//               bounds of its columns the input columns [c0, c0 + ncols).  Both are uniform over the workgroup.
//   2. stage    the nrows row segments (ncols * C bytes each, at any byte alignment) go to LDS as whole 16-byte lines, one line per
//               lane and load: line k of row r is the aligned line at (address of the segment's first byte & ~15) + 16 k, so a
//               segment sits `lead` = address & 15 bytes into its LDS row.  The line index is clamped to the row's last line, the
//               load is unconditional and the lines past it are zeroed by a select.  Every line read holds at least one byte of src.
//   3. H pass   item (row r, column x, channel c) -> intermediate tile [nrows][TW * C] uint8 in LDS (a copy where the pass is skipped)
//   4. V pass   item (row y, column x, channel c) out of the intermediate tile -> ONE byte store to dst; neighbouring lanes write
//               neighbouring bytes.
// The host picks the largest (TH, TW) of {32 x 64, 16 x 32, 8 x 16} whose staged segments plus intermediate tile fit 64 KiB of LDS;
// the tables live in device memory, so the rows / columns a tile can need are bounded from the shape alone:
//   span(T) <= min(in, ceil((T - 1) * in / out) + ksize + 1)                  (ksize >= 2 * support + 1)
// and the kernel clamps what the tables say to that bound and to the image, so no table content can make it read outside src.
// Every upscale and any moderate downscale fits; the coefficients are read through the caches (each is used by a whole tile row or
// column).
//
// Two launches (route 2): no tile fits (a strong downscale).  resample_axis_kernel runs the horizontal pass src -> workspace
// [B][Hin][Wout][C] (Pillow's own temporary image), then the vertical pass workspace -> dst: one thread per output byte, reading
// through the caches.  With one pass skipped it is one launch and needs no workspace.
//
// da_gather_resize: nearest-neighbour resize (F.interpolate's default, the reference's route for tensors and arrays) of fp32 or
// uint8 images, NCHW or NHWC, through one int32 source-index table per axis: dst[.., y, x] = src[.., yidx[y], xidx[x]].  A copy.
#include <math.h>
#include "common.cuh"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_LDS_LIMIT = 64 * 1024;
constexpr int RS_TILES[3][2] = {{32, 64}, {16, 32}, {8, 16}};

struct ResampleGeom {
  int route;               // 1 = one launch, 2 = two launches
  int TH, TW;              // route 1: the output tile
  int maxrows, maxcols;    // route 1: bound of the input rows / columns one tile reads
  int stride;              // route 1: bytes of a staged row in LDS (whole 16-byte lines, room for any lead)
  unsigned lds;
  long long ws;            // workspace bytes (route 2 with both passes)
};

struct ResampleArgs {
  const uint8_t* src;
  uint8_t* dst;
  const int* hcoef;
  const int* hb;           // NULL: the horizontal pass is skipped
  const int* vcoef;
  const int* vb;           // NULL: the vertical pass is skipped
  int ksh, ksv;
  int B, Hin, Win, Hout, Wout;
  int tiles_x, tiles_y;
  ResampleGeom g;
};

// the input samples T neighbouring outputs can read along one axis, from the shape alone
int rs_span(int T, int in, int out, int ks, bool skipped) {
  if (T > out) T = out;
  if (skipped) return T;
  const long long s = (long long)ceil((double)(T - 1) * ((double)in / (double)out)) + ks + 1;
  return (int)(s < in ? s : in);
}

// 0 = fine, else a DA_ERR_* code.  route: 0 = automatic, 1 = one launch or DA_ERR_UNSUPPORTED, 2 = two launches.
int rs_geom(int B, int Hin, int Win, int Hout, int Wout, int C, int ksh, int ksv, int route, ResampleGeom* g) {
  if (B <= 0 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0 || (C != 1 && C != 3)) return DA_ERR_UNSUPPORTED;
  if (route < 0 || route > 2) return DA_ERR_INVALID;
  const bool hskip = Win == Wout, vskip = Hin == Hout;
  if ((!hskip && ksh <= 0) || (!vskip && ksv <= 0)) return DA_ERR_UNSUPPORTED;
  if ((long long)Hin * Win * C > 0x7fffffffLL || (long long)Hout * Wout * C > 0x7fffffffLL || (long long)Hin * Wout * C > 0x7fffffffLL)
    return DA_ERR_UNSUPPORTED;                                                 // 32-bit byte index inside one image
  g->route = 2, g->TH = g->TW = g->maxrows = g->maxcols = g->stride = 0, g->lds = 0;
  g->ws = hskip || vskip ? 0 : (long long)B * Hin * Wout * C;
  if (route == 2) return 0;
  for (const auto& t : RS_TILES) {
    const int rows = rs_span(t[0], Hin, Hout, ksv, vskip), cols = rs_span(t[1], Win, Wout, ksh, hskip);
    const long long stride = ((long long)cols * C + 15 + 15) & ~15LL;
    const long long lds = rows * stride + (((long long)rows * t[1] * C + 15) & ~15LL);
    if (lds > RS_LDS_LIMIT) continue;
    const long long tiles = (long long)((Hout + t[0] - 1) / t[0]) * ((Wout + t[1] - 1) / t[1]) * B;
    if (tiles > 0x7fffffffLL) return DA_ERR_UNSUPPORTED;
    g->route = 1, g->TH = t[0], g->TW = t[1], g->maxrows = rows, g->maxcols = cols, g->stride = (int)stride, g->lds = (unsigned)lds;
    g->ws = 0;
    return 0;
  }
  return route == 1 ? DA_ERR_UNSUPPORTED : 0;
}

__device__ __forceinline__ uint8_t rs_clip8(int acc) {
  const int v = acc >> 22;
  return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// [lo, lo + n) of the input an axis of a tile reads: the union of its outputs' (xmin, xcount), clamped to the image and to `cap`
__device__ __forceinline__ void rs_range(const int* bounds, int o0, int o1, int in, int cap, int& lo, int& n) {
  int a = o0, b = o1;                                                          // a skipped pass reads its own outputs
  if (bounds) {
    a = 0x7fffffff, b = 0;
    for (int o = o0; o < o1; ++o) {
      const int m = bounds[2 * o], e = m + bounds[2 * o + 1];
      a = m < a ? m : a, b = e > b ? e : b;
    }
  }
  a = a < 0 ? 0 : a > in - 1 ? in - 1 : a;
  b = b > in ? in : b;
  n = b - a < 1 ? 1 : b - a;
  n = n > cap ? cap : n;
  lo = a;
}

template <int C>
__global__ __launch_bounds__(RS_THREADS) void resample_tile_kernel(const ResampleArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const ResampleGeom& g = a.g;
  uint8_t* stage = smem;
  uint8_t* inter = smem + (((size_t)g.maxrows * g.stride + 15) & ~(size_t)15);
  const unsigned wg = blockIdx.x;
  const int tx = (int)(wg % (unsigned)a.tiles_x), ty = (int)((wg / (unsigned)a.tiles_x) % (unsigned)a.tiles_y);
  const long long img = wg / ((unsigned)a.tiles_x * (unsigned)a.tiles_y);
  const int y0 = ty * g.TH, y1 = y0 + g.TH < a.Hout ? y0 + g.TH : a.Hout;
  const int x0 = tx * g.TW, x1 = x0 + g.TW < a.Wout ? x0 + g.TW : a.Wout;
  int r0, nrows, c0, ncols;
  rs_range(a.vb, y0, y1, a.Hin, g.maxrows, r0, nrows);
  rs_range(a.hb, x0, x1, a.Win, g.maxcols, c0, ncols);
  const int seg = ncols * C;                                                   // bytes of a staged row segment
  const uint8_t* first = a.src + ((img * a.Hin + r0) * a.Win + c0) * C;       // (row r of the tile: + r * pitch)
  const long long pitch = (long long)a.Win * C;

  // stage: whole aligned 16-byte lines, clamped address, unconditional load, select
  const int lpr = g.stride >> 4;                                               // lines per LDS row
  for (int item = (int)threadIdx.x; item < nrows * lpr; item += RS_THREADS) {
    const int r = item / lpr, k = item - r * lpr;
    const uintptr_t p = (uintptr_t)(first + r * pitch);
    const int lines = (int)(((p & 15) + (uintptr_t)seg + 15) >> 4);
    const uint4 v = *(const uint4*)((p & ~(uintptr_t)15) + 16 * (uintptr_t)(k < lines ? k : lines - 1));
    ((uint4*)stage)[item] = k < lines ? v : make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();

  // horizontal pass: staged rows -> intermediate tile [nrows][TW * C]
  const int wb = (x1 - x0) * C, istride = g.TW * C;
  for (int item = (int)threadIdx.x; item < nrows * wb; item += RS_THREADS) {
    const int r = item / wb, xc = item - r * wb;
    const int x = x0 + xc / C, ch = xc % C;
    const uint8_t* row = stage + r * g.stride + (int)((uintptr_t)(first + r * pitch) & 15) + ch;
    uint8_t v;
    if (a.hb) {
      const int xmin = a.hb[2 * x];
      int lo = xmin, hi = xmin + a.hb[2 * x + 1];
      lo = lo < c0 ? c0 : lo;
      hi = hi > c0 + ncols ? c0 + ncols : hi;
      hi = hi > xmin + a.ksh ? xmin + a.ksh : hi;
      const int* k = a.hcoef + (long long)x * a.ksh - xmin;
      int acc = 1 << 21;
      for (int i = lo; i < hi; ++i) acc += (int)row[(i - c0) * C] * k[i];
      v = rs_clip8(acc);
    } else {
      v = row[(x - c0) * C];
    }
    inter[r * istride + xc] = v;
  }
  __syncthreads();

  // vertical pass: intermediate tile -> dst, every byte once
  for (int item = (int)threadIdx.x; item < (y1 - y0) * wb; item += RS_THREADS) {
    const int yr = item / wb, xc = item - yr * wb;
    const int y = y0 + yr;
    uint8_t v;
    if (a.vb) {
      const int ymin = a.vb[2 * y];
      int lo = ymin, hi = ymin + a.vb[2 * y + 1];
      lo = lo < r0 ? r0 : lo;
      hi = hi > r0 + nrows ? r0 + nrows : hi;
      hi = hi > ymin + a.ksv ? ymin + a.ksv : hi;
      const int* k = a.vcoef + (long long)y * a.ksv - ymin;
      int acc = 1 << 21;
      for (int i = lo; i < hi; ++i) acc += (int)inter[(i - r0) * istride + xc] * k[i];
      v = rs_clip8(acc);
    } else {
      v = inter[(yr < nrows ? yr : nrows - 1) * istride + xc];
    }
    a.dst[((img * a.Hout + y) * a.Wout + x0) * C + xc] = v;
  }
}

// one pass along the middle axis of [outer][Lin][E] -> [outer][Lout][E]: horizontal (outer = B * H, E = C) or vertical
// (outer = B, E = W * C).  One thread per output byte.
__global__ __launch_bounds__(RS_THREADS) void resample_axis_kernel(const uint8_t* in, uint8_t* out, const int* coef, const int* bounds,
                                                                  int ks, long long outer, int Lin, int Lout, int E) {
  const long long n = outer * Lout * E;
  const long long idx = (long long)blockIdx.x * RS_THREADS + threadIdx.x;
  if (idx >= n) return;
  const int e = (int)(idx % E);
  const long long q = idx / E;
  const int o = (int)(q % Lout);
  const long long base = (q / Lout) * Lin * E + e;
  int lo = bounds[2 * o], hi = lo + bounds[2 * o + 1];
  const int* k = coef + (long long)o * ks - lo;
  hi = hi > lo + ks ? lo + ks : hi;
  lo = lo < 0 ? 0 : lo;
  hi = hi > Lin ? Lin : hi;
  int acc = 1 << 21;
  for (int i = lo; i < hi; ++i) acc += (int)in[base + (long long)i * E] * k[i];
  out[idx] = rs_clip8(acc);
}

template <typename T>
__global__ __launch_bounds__(RS_THREADS) void gather_resize_kernel(const T* src, T* dst, const int* yidx, const int* xidx, long long n,
                                                                  int C, int Hin, int Win, int Hout, int Wout, int nchw) {
  const long long idx = (long long)blockIdx.x * RS_THREADS + threadIdx.x;
  if (idx >= n) return;
  int c, x, y;
  long long q;
  if (nchw) {
    x = (int)(idx % Wout), q = idx / Wout;
    y = (int)(q % Hout), q /= Hout;
    c = (int)(q % C), q /= C;
  } else {
    c = (int)(idx % C), q = idx / C;
    x = (int)(q % Wout), q /= Wout;
    y = (int)(q % Hout), q /= Hout;
  }
  int sy = yidx[y], sx = xidx[x];
  sy = sy < 0 ? 0 : sy > Hin - 1 ? Hin - 1 : sy;
  sx = sx < 0 ? 0 : sx > Win - 1 ? Win - 1 : sx;
  dst[idx] = nchw ? src[((q * C + c) * Hin + sy) * Win + sx] : src[((q * Hin + sy) * Win + sx) * C + c];
}

int rs_launch_axis(const uint8_t* in, uint8_t* out, const int* coef, const int* bounds, int ks, long long outer, int Lin, int Lout,
                   int E, hipStream_t st) {
  const long long blocks = (outer * Lout * E + RS_THREADS - 1) / RS_THREADS;
  if (blocks > 0x7fffffffLL) return DA_ERR_UNSUPPORTED;
  DA_LAUNCH(resample_axis_kernel, dim3((unsigned)blocks), dim3(RS_THREADS), 0, st, in, out, coef, bounds, ks, outer, Lin, Lout, E);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

}  // namespace

extern "C" int da_resample_u8_route(int B, int Hin, int Win, int Hout, int Wout, int C, int ksize_h, int ksize_v, int route,
                                    int* tile_h, int* tile_w, long long* workspace_bytes) {
  ResampleGeom g;
  const int rc = rs_geom(B, Hin, Win, Hout, Wout, C, ksize_h, ksize_v, route, &g);
  if (rc) return -rc;
  if (tile_h) *tile_h = g.TH;
  if (tile_w) *tile_w = g.TW;
  if (workspace_bytes) *workspace_bytes = g.ws;
  return g.route;
}

extern "C" int da_resample_u8(const void* src, void* dst, const int* hcoef, const int* hbounds, int ksize_h, const int* vcoef,
                              const int* vbounds, int ksize_v, void* workspace, long long workspace_bytes, int B, int Hin, int Win,
                              int Hout, int Wout, int C, int route, void* stream) {
  if (!src || !dst) return DA_ERR_INVALID;
  ResampleArgs a;
  const int rc = rs_geom(B, Hin, Win, Hout, Wout, C, ksize_h, ksize_v, route, &a.g);
  if (rc) return rc;
  const bool hskip = Win == Wout, vskip = Hin == Hout;
  if ((!hskip && (!hcoef || !hbounds)) || (!vskip && (!vcoef || !vbounds))) return DA_ERR_UNSUPPORTED;
  if (a.g.ws && (!workspace || workspace_bytes < a.g.ws)) return DA_ERR_UNSUPPORTED;
  if (((uintptr_t)hcoef | (uintptr_t)hbounds | (uintptr_t)vcoef | (uintptr_t)vbounds) & 3) return DA_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  if (a.g.route == 1) {
    if ((uintptr_t)src & 15) return DA_ERR_INVALID;                            // whole 16-byte lines: none starts in front of src
    a.src = (const uint8_t*)src, a.dst = (uint8_t*)dst;
    a.hcoef = hskip ? nullptr : hcoef, a.hb = hskip ? nullptr : hbounds, a.ksh = ksize_h;
    a.vcoef = vskip ? nullptr : vcoef, a.vb = vskip ? nullptr : vbounds, a.ksv = ksize_v;
    a.B = B, a.Hin = Hin, a.Win = Win, a.Hout = Hout, a.Wout = Wout;
    a.tiles_x = (Wout + a.g.TW - 1) / a.g.TW, a.tiles_y = (Hout + a.g.TH - 1) / a.g.TH;
    const dim3 grid((unsigned)((long long)a.tiles_x * a.tiles_y * B));
    if (C == 1)
      DA_LAUNCH(resample_tile_kernel<1>, grid, dim3(RS_THREADS), a.g.lds, st, a);
    else
      DA_LAUNCH(resample_tile_kernel<3>, grid, dim3(RS_THREADS), a.g.lds, st, a);
    DA_CHECK_LAUNCH();
    return DA_OK;
  }
  const uint8_t* s = (const uint8_t*)src;
  uint8_t* d = (uint8_t*)dst;
  if (hskip && vskip) {
    if (hipMemcpyAsync(d, s, (size_t)B * Hin * Win * C, hipMemcpyDeviceToDevice, st) != hipSuccess) return DA_ERR_LAUNCH;
    return DA_OK;
  }
  if (vskip) return rs_launch_axis(s, d, hcoef, hbounds, ksize_h, (long long)B * Hin, Win, Wout, C, st);
  if (hskip) return rs_launch_axis(s, d, vcoef, vbounds, ksize_v, B, Hin, Hout, Win * C, st);
  const int r1 = rs_launch_axis(s, (uint8_t*)workspace, hcoef, hbounds, ksize_h, (long long)B * Hin, Win, Wout, C, st);
  if (r1) return r1;
  return rs_launch_axis((const uint8_t*)workspace, d, vcoef, vbounds, ksize_v, B, Hin, Hout, Wout * C, st);
}

extern "C" int da_gather_resize(const void* src, void* dst, const int* yidx, const int* xidx, int B, int C, int Hin, int Win, int Hout,
                                int Wout, int elem_bytes, int nchw, void* stream) {
  if (!src || !dst || !yidx || !xidx) return DA_ERR_INVALID;
  if (B <= 0 || C <= 0 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0 || (elem_bytes != 1 && elem_bytes != 4))
    return DA_ERR_UNSUPPORTED;
  if (elem_bytes == 4 && (((uintptr_t)src | (uintptr_t)dst) & 3)) return DA_ERR_INVALID;
  const long long n = (long long)B * C * Hout * Wout, blocks = (n + RS_THREADS - 1) / RS_THREADS;
  if (blocks > 0x7fffffffLL) return DA_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (elem_bytes == 4)
    DA_LAUNCH(gather_resize_kernel<uint32_t>, dim3((unsigned)blocks), dim3(RS_THREADS), 0, st, (const uint32_t*)src, (uint32_t*)dst, yidx,
              xidx, n, C, Hin, Win, Hout, Wout, nchw);
  else
    DA_LAUNCH(gather_resize_kernel<uint8_t>, dim3((unsigned)blocks), dim3(RS_THREADS), 0, st, (const uint8_t*)src, (uint8_t*)dst, yidx, xidx,
              n, C, Hin, Win, Hout, Wout, nchw);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
