// The tail of the VAE encoder: the encoder's conv_out result (2 L channels per pixel) -> quant_conv -> DiagonalGaussianDistribution
// -> sample / mode -> latent scaling -> scheduler.add_noise, in ONE pass that reads the conv_out result once and writes NCHW latents.
// The head of the encoder (the caller's image -> conv_in) is the image-source loader of the four-pixel thin-input conv (misc.hip).
//
// Reference (diffusers src/diffusers/):
//   AutoencoderKL.encode / _encode             models/autoencoders/autoencoder_kl.py:146-185 (quant_conv 1x1 after the encoder)
//   DiagonalGaussianDistribution               models/autoencoders/vae.py:685-718 (chunk, clamp(-30, 20), exp(0.5 logvar), sample)
//   retrieve_latents + prepare_latents         pipelines/stable_diffusion_xl/pipeline_stable_diffusion_xl_img2img.py
//                                              (scaling_factor * latents, scheduler.add_noise)
//   EulerDiscreteScheduler.add_noise           schedulers/scheduling_euler_discrete.py (x + sigma n)
//   DDIMScheduler / DDPMScheduler.add_noise    schedulers/scheduling_ddim.py, scheduling_ddpm.py (sqrt(a) x + sqrt(1 - a) n)
//
// Operation order per latent element (c < L; the reference runs each line as a bf16 torch op, so each result is rounded to bf16;
// the arithmetic here is fp32 with the same rounding points):
//   p[o]    = bf16(bq[o] + sum_k wq[o][k] x[k])      k ascending, fp32 fma: a product of two bf16 values is exact in fp32, so the
//                                                    fma chain equals the separate multiply-adds of the restatement in the tests
//   mean    = p[c];  logvar = clamp(p[L + c], -30, 20)
//   SAMPLE: std = bf16(expf(bf16(0.5 logvar)));  z = bf16(mean + bf16(std * eps1))       MEAN: z = mean
//   flags & SHIFT: z = bf16(z - shift);   flags & SCALE: z = bf16(z * scale)
//   eps2:   z = bf16(bf16(a z) + bf16(b eps2))        (Euler: a = 1, b = sigma; DDIM / DDPM: a = sqrt(abar), b = sqrt(1 - abar),
//                                                     both computed by the caller in bf16 as the reference does)
// da_flux_prepare_latents (FLUX img2img / inpainting: pipelines/flux/pipeline_flux_img2img.py prepare_latents, _pack_latents;
// FlowMatchEulerDiscreteScheduler.scale_noise, schedulers/scheduling_flow_match_euler_discrete.py) runs the same lines without a
// quant_conv, keeps z, and ends with  x = bf16(bf16(a z) + bf16(b noise))  (a = bf16(1 - bf16(sigma)), b = bf16(sigma)); x, z and
// the noise are written as packed tokens [B][(H/2)(W/2)][4 L], column c * 4 + di * 2 + dj <- latent (c, 2 i + di, 2 j + dj).
// expf is the device library's (what torch.exp of a bf16 tensor evaluates on this GPU too); a host restatement may differ from it in
// the last fp32 bit, which reaches the bf16 std in rare ties only.
#include "common.cuh"

namespace {

__device__ __forceinline__ float rbf(float v) { return bf2f(f2bf(v)); }

// QC: the instantiation may carry a quant_conv (its [2L][2L] weights live in registers: L = 4 only; the 16-channel VAEs have none)
template <int L, int MODE, bool NOISE, bool QC>
__global__ __launch_bounds__(256) void posterior_latents_kernel(const uint16_t* __restrict__ in, long long sB, long long sC, long long sP,
                                                                const uint16_t* __restrict__ wq, const uint16_t* __restrict__ bq,
                                                                const uint16_t* __restrict__ eps1, const uint16_t* __restrict__ eps2,
                                                                uint16_t* __restrict__ out, int B, long long HW, int flags, float shift,
                                                                float scale, float a, float b) {
  constexpr int C2 = 2 * L;
  // quant_conv weights and bias, loaded once per thread before the pixel loop (uniform addresses: scalar loads)
  float wf[QC ? C2 * C2 : 1], bfv[QC ? C2 : 1];
  if (QC && wq) {
#pragma unroll
    for (int j = 0; j < C2 * C2; ++j) wf[j] = bf2f(wq[j]);
#pragma unroll
    for (int o = 0; o < C2; ++o) bfv[o] = bf2f(bq[o]);
  }
  const long long total = (long long)B * HW;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long bi = i / HW, p = i - bi * HW;
    const uint16_t* src = in + bi * sB + p * sP;
    const size_t lat = (size_t)bi * L * (size_t)HW + (size_t)p;     // element (bi, 0, p) of a [B][L][HW] tensor
    // every load of the pixel is issued before the first use: the 2 L inputs and the L noise values of each source
    uint16_t xr[C2], e1r[L], e2r[L];
#pragma unroll
    for (int c = 0; c < C2; ++c) xr[c] = src[c * sC];
    if (MODE == DA_POSTERIOR_SAMPLE) {
#pragma unroll
      for (int c = 0; c < L; ++c) e1r[c] = eps1[lat + (size_t)c * HW];
    }
    if (NOISE) {
#pragma unroll
      for (int c = 0; c < L; ++c) e2r[c] = eps2[lat + (size_t)c * HW];
    }
    float pm[C2];
    if (QC && wq) {
#pragma unroll
      for (int o = 0; o < C2; ++o) {
        float acc = bfv[o];
#pragma unroll
        for (int k = 0; k < C2; ++k) acc = fmaf(wf[o * C2 + k], bf2f(xr[k]), acc);
        pm[o] = rbf(acc);
      }
    } else {
#pragma unroll
      for (int o = 0; o < C2; ++o) pm[o] = bf2f(xr[o]);
    }
    if (MODE == DA_POSTERIOR_MOMENTS) {
#pragma unroll
      for (int o = 0; o < C2; ++o) out[(size_t)bi * C2 * (size_t)HW + (size_t)o * HW + (size_t)p] = f2bf(pm[o]);
      continue;
    }
#pragma unroll
    for (int c = 0; c < L; ++c) {
      float z = pm[c];
      if (MODE == DA_POSTERIOR_SAMPLE) {
        const float lv = fminf(fmaxf(pm[L + c], -30.0f), 20.0f);
        const float sd = rbf(expf(rbf(__fmul_rn(0.5f, lv))));
        z = rbf(__fadd_rn(z, rbf(__fmul_rn(sd, bf2f(e1r[c])))));
      }
      if (flags & DA_LATENTS_SHIFT) z = rbf(__fsub_rn(z, shift));
      if (flags & DA_LATENTS_SCALE) z = rbf(__fmul_rn(z, scale));
      if (NOISE) z = rbf(__fadd_rn(rbf(__fmul_rn(a, z)), rbf(__fmul_rn(b, bf2f(e2r[c])))));
      out[lat + (size_t)c * HW] = f2bf(z);
    }
  }
}

// add_noise alone (latents in, any channel count): out[i] = bf16(bf16(a x) + bf16(b n)), one element per thread, the latents read
// through the same strides as above
__global__ __launch_bounds__(256) void add_noise_kernel(const uint16_t* __restrict__ in, long long sB, long long sC, long long sP,
                                                        const uint16_t* __restrict__ noise, uint16_t* __restrict__ out, int L, long long HW,
                                                        long long total, float a, float b) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long bc = i / HW, p = i - bc * HW;
    const long long bi = bc / L, c = bc - bi * L;
    const float x = bf2f(in[bi * sB + c * sC + p * sP]);
    const float n = bf2f(noise[i]);
    out[i] = f2bf(__fadd_rn(rbf(__fmul_rn(a, x)), rbf(__fmul_rn(b, n))));
  }
}

// FLUX img2img / inpainting latent preparation: the posterior (no quant_conv), the latent shift / scale, scale_noise and
// FluxPipeline._pack_latents in one pass.  One thread per (token, channel): the channel's 2 x 2 patch is 4 consecutive columns of the
// token row (one 8-byte store per output), so the L threads of a token write its 8 L-byte row (128 bytes at L = 16) contiguously
// and a wave writes whole rows back to back.  All loads of the patch are issued before the first use.
template <int MODE>
__global__ __launch_bounds__(256) void flux_prepare_kernel(const uint16_t* __restrict__ in, long long sB, long long sC, long long sP,
                                                           const uint16_t* __restrict__ eps1, const uint16_t* __restrict__ noise,
                                                           uint16_t* __restrict__ out, uint16_t* __restrict__ img_out,
                                                           uint16_t* __restrict__ noise_out, int L, int H, int W, long long total,
                                                           int flags, float shift, float scale, float a, float b) {
  const long long W2 = W / 2, T = (long long)(H / 2) * W2, HW = (long long)H * W;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long tok = i / L, c = i - tok * L;
    const long long bi = tok / T, t = tok - bi * T;
    const long long ti = t / W2, tj = t - ti * W2;
    const long long p0 = 2 * ti * W + 2 * tj;                              // pixel (2 ti, 2 tj); column k = di * 2 + dj
    const long long po[4] = {p0, p0 + 1, p0 + W, p0 + W + 1};
    const uint16_t* src = in + bi * sB + c * sC;
    const size_t lat = ((size_t)bi * L + (size_t)c) * (size_t)HW;          // element (bi, c, 0) of a [B][L][HW] tensor
    uint16_t mr[4], lr[4], e1r[4], nr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) mr[k] = src[po[k] * sP];
    if (MODE == DA_POSTERIOR_SAMPLE) {
#pragma unroll
      for (int k = 0; k < 4; ++k) lr[k] = src[(long long)L * sC + po[k] * sP];
#pragma unroll
      for (int k = 0; k < 4; ++k) e1r[k] = eps1[lat + (size_t)po[k]];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) nr[k] = noise[lat + (size_t)po[k]];
    uint16_t zr[4], xr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float z = bf2f(mr[k]);
      if (MODE == DA_POSTERIOR_SAMPLE) {
        const float lv = fminf(fmaxf(bf2f(lr[k]), -30.0f), 20.0f);
        const float sd = rbf(expf(rbf(__fmul_rn(0.5f, lv))));
        z = rbf(__fadd_rn(z, rbf(__fmul_rn(sd, bf2f(e1r[k])))));
      }
      if (flags & DA_LATENTS_SHIFT) z = rbf(__fsub_rn(z, shift));
      if (flags & DA_LATENTS_SCALE) z = rbf(__fmul_rn(z, scale));
      zr[k] = f2bf(z);
      xr[k] = f2bf(__fadd_rn(rbf(__fmul_rn(a, z)), rbf(__fmul_rn(b, bf2f(nr[k])))));
    }
    const size_t o = (size_t)i * 4;                                        // [B][T][4 L]: row tok, column c * 4
    *(uint2*)(out + o) = make_uint2(xr[0] | ((uint32_t)xr[1] << 16), xr[2] | ((uint32_t)xr[3] << 16));
    if (img_out) *(uint2*)(img_out + o) = make_uint2(zr[0] | ((uint32_t)zr[1] << 16), zr[2] | ((uint32_t)zr[3] << 16));
    if (noise_out) *(uint2*)(noise_out + o) = make_uint2(nr[0] | ((uint32_t)nr[1] << 16), nr[2] | ((uint32_t)nr[3] << 16));
  }
}

}  // namespace

extern "C" int da_vae_posterior_latents(const void* in, long long sB, long long sC, long long sP, const void* wq, const void* bq,
                                        const void* eps1, const void* eps2, void* out, int B, long long HW, int L, int mode, int flags,
                                        float shift, float scale, float a, float b, void* stream) {
  if (!in || !out || B <= 0 || HW <= 0 || L <= 0 || sB < 0 || sC < 0 || sP < 0 || mode < DA_POSTERIOR_MOMENTS ||
      mode > DA_POSTERIOR_NOISE || (flags & ~(DA_LATENTS_SHIFT | DA_LATENTS_SCALE)))
    return DA_ERR_INVALID;
  if (mode == DA_POSTERIOR_SAMPLE && !eps1) return DA_ERR_INVALID;
  if (mode == DA_POSTERIOR_NOISE && (!eps2 || wq || flags)) return DA_ERR_INVALID;
  if (mode == DA_POSTERIOR_MOMENTS && (eps2 || flags)) return DA_ERR_INVALID;
  if (!wq != !bq) return DA_ERR_INVALID;                        // quant_conv: weight and bias, or neither
  hipStream_t s = (hipStream_t)stream;
  if (mode == DA_POSTERIOR_NOISE) {
    const long long total = (long long)B * L * HW;
    long long blocks = (total + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    DA_LAUNCH(add_noise_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const uint16_t*)in, sB, sC, sP, (const uint16_t*)eps2,
              (uint16_t*)out, L, HW, total, a, b);
    DA_CHECK_LAUNCH();
    return DA_OK;
  }
  if (L != 4 && !(L == 16 && !wq)) return DA_ERR_UNSUPPORTED;    // L = 16 with a quant_conv: 32 x 32 weights per thread would spill
  const long long total = (long long)B * HW;
  long long blocks = (total + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  const dim3 grid((unsigned)blocks);
#define DA_POST_L(L_, Q_, M_, N_)                                                                                                      \
  DA_LAUNCH((posterior_latents_kernel<L_, M_, N_, Q_>), grid, dim3(256), 0, s, (const uint16_t*)in, sB, sC, sP, (const uint16_t*)wq, \
            (const uint16_t*)bq, (const uint16_t*)eps1, (const uint16_t*)eps2, (uint16_t*)out, B, HW, flags, shift, scale, a, b)
#define DA_POST(M_, N_)                     \
  do {                                      \
    if (L == 4) DA_POST_L(4, true, M_, N_); \
    else DA_POST_L(16, false, M_, N_);      \
  } while (0)
  if (mode == DA_POSTERIOR_MOMENTS) DA_POST(DA_POSTERIOR_MOMENTS, false);
  else if (mode == DA_POSTERIOR_MEAN && eps2) DA_POST(DA_POSTERIOR_MEAN, true);
  else if (mode == DA_POSTERIOR_MEAN) DA_POST(DA_POSTERIOR_MEAN, false);
  else if (eps2) DA_POST(DA_POSTERIOR_SAMPLE, true);
  else DA_POST(DA_POSTERIOR_SAMPLE, false);
#undef DA_POST
#undef DA_POST_L
  DA_CHECK_LAUNCH();
  return DA_OK;
}

extern "C" int da_flux_prepare_latents(const void* in, long long sB, long long sC, long long sP, const void* eps1, const void* noise,
                                       void* latents_packed, void* image_latents_packed, void* noise_packed, int B, int H, int W, int L,
                                       int mode, int flags, float shift, float scale, float a, float b, void* stream) {
  if (!in || !noise || !latents_packed || B <= 0 || H <= 0 || W <= 0 || L <= 0 || (H & 1) || (W & 1) || sB < 0 || sC < 0 || sP < 0 ||
      (mode != DA_POSTERIOR_MEAN && mode != DA_POSTERIOR_SAMPLE && mode != DA_POSTERIOR_NOISE) ||
      (flags & ~(DA_LATENTS_SHIFT | DA_LATENTS_SCALE)))
    return DA_ERR_INVALID;
  if (mode == DA_POSTERIOR_SAMPLE && !eps1) return DA_ERR_INVALID;
  // the packed rows are written with 8-byte stores (one channel's 2 x 2 patch)
  if (((uintptr_t)latents_packed | (uintptr_t)image_latents_packed | (uintptr_t)noise_packed) & 7) return DA_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  const long long total = (long long)B * (H / 2) * (W / 2) * L;           // (token, channel) pairs
  long long blocks = (total + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  const dim3 grid((unsigned)blocks);
#define DA_PREP(M_)                                                                                                            \
  DA_LAUNCH((flux_prepare_kernel<M_>), grid, dim3(256), 0, s, (const uint16_t*)in, sB, sC, sP, (const uint16_t*)eps1,          \
            (const uint16_t*)noise, (uint16_t*)latents_packed, (uint16_t*)image_latents_packed, (uint16_t*)noise_packed, L, H, W, \
            total, flags, shift, scale, a, b)
  if (mode == DA_POSTERIOR_SAMPLE) DA_PREP(DA_POSTERIOR_SAMPLE);
  else DA_PREP(DA_POSTERIOR_MEAN);                                        // MEAN, and NOISE (the input is the latents): z = in[c]
#undef DA_PREP
  DA_CHECK_LAUNCH();
  return DA_OK;
}
