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
// expf is the device library's (what torch.exp of a bf16 tensor evaluates on this GPU too); a host restatement may differ from it in
// the last fp32 bit, which reaches the bf16 std in rare ties only.
#include "common.cuh"

namespace {

__device__ __forceinline__ float rbf(float v) { return bf2f(f2bf(v)); }

template <int L, int MODE, bool NOISE>
__global__ __launch_bounds__(256) void posterior_latents_kernel(const uint16_t* __restrict__ in, long long sB, long long sC, long long sP,
                                                                const uint16_t* __restrict__ wq, const uint16_t* __restrict__ bq,
                                                                const uint16_t* __restrict__ eps1, const uint16_t* __restrict__ eps2,
                                                                uint16_t* __restrict__ out, int B, long long HW, int flags, float shift,
                                                                float scale, float a, float b) {
  constexpr int C2 = 2 * L;
  // quant_conv weights and bias, loaded once per thread before the pixel loop (uniform addresses: scalar loads)
  float wf[C2 * C2], bfv[C2];
  if (wq) {
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
    if (wq) {
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
  if (L != 4) return DA_ERR_UNSUPPORTED;
  const long long total = (long long)B * HW;
  long long blocks = (total + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  const dim3 grid((unsigned)blocks);
#define DA_POST(M_, N_)                                                                                                         \
  DA_LAUNCH((posterior_latents_kernel<4, M_, N_>), grid, dim3(256), 0, s, (const uint16_t*)in, sB, sC, sP, (const uint16_t*)wq, \
            (const uint16_t*)bq, (const uint16_t*)eps1, (const uint16_t*)eps2, (uint16_t*)out, B, HW, flags, shift, scale, a, b)
  if (mode == DA_POSTERIOR_MOMENTS) DA_POST(DA_POSTERIOR_MOMENTS, false);
  else if (mode == DA_POSTERIOR_MEAN && eps2) DA_POST(DA_POSTERIOR_MEAN, true);
  else if (mode == DA_POSTERIOR_MEAN) DA_POST(DA_POSTERIOR_MEAN, false);
  else if (eps2) DA_POST(DA_POSTERIOR_SAMPLE, true);
  else DA_POST(DA_POSTERIOR_SAMPLE, false);
#undef DA_POST
  DA_CHECK_LAUNCH();
  return DA_OK;
}
