// Fused scheduler.step + classifier-free-guidance kernels for gfx950 (MI355X).
//
// Reference (diffusers src/diffusers/):
//   CFG combine        pipelines/stable_diffusion/pipeline_stable_diffusion.py:1054-1055,
//                      pipelines/stable_diffusion_xl/pipeline_stable_diffusion_xl.py:1223-1225
//   Euler              schedulers/scheduling_euler_discrete.py:326-348 (scale_model_input), :685-800 (step)
//   Euler ancestral    schedulers/scheduling_euler_ancestral_discrete.py (step; per-step noise from a pre-drawn table)
//   Heun, DPM2         schedulers/scheduling_heun_discrete.py, scheduling_k_dpm_2_discrete.py (step; one kernel, the phase in the row)
//   DDIM               schedulers/scheduling_ddim.py:384-514
//   DDPM               schedulers/scheduling_ddpm.py:461-567
//   FlowMatch Euler    schedulers/scheduling_flow_match_euler_discrete.py:423-523
//
// The reference issues ~10 elementwise launches per step, each rounding to the tensor dtype.  These kernels do the
// whole update in one pass but reproduce the reference's rounding points exactly (bf16 tensors round after every
// torch op; 0-d fp32 scalars promote nothing), so results are bit-identical to the reference for identical inputs.
// Per-step scalars live in a device table (8 floats per step) indexed by a device-resident step counter, so a whole
// denoising step can be captured once in a HIP graph and replayed for every step.
//
// Every kernel but the statistics pass is elementwise and is put together from the shared pieces below: its loop from
// EW_EACH / EW_EACH4 + EW_TAIL, its guided model output from load_eps / LOAD_EPS4, its x0 from x0_alpha_beta / x0_sigma, and its
// entry point picks the instantiation with dispatch_dtype / dispatch_step and sizes a 4-wide launch with vec_split.
#include <type_traits>
#include "common.cuh"

namespace {

template <typename T>
struct IO;
template <>
struct IO<uint16_t> {
  static __device__ __forceinline__ float ld(const uint16_t* p, size_t i) { return bf2f(p[i]); }
  static __device__ __forceinline__ void st(uint16_t* p, size_t i, float v) { p[i] = f2bf(v); }
  static __device__ __forceinline__ float rnd(float v) { return bf2f(f2bf(v)); }  // torch rounds each op's result
};
template <>
struct IO<float> {
  static __device__ __forceinline__ float ld(const float* p, size_t i) { return p[i]; }
  static __device__ __forceinline__ void st(float* p, size_t i, float v) { p[i] = v; }
  static __device__ __forceinline__ float rnd(float v) { return v; }
};

template <typename T>
struct Vec4;
template <>
struct Vec4<uint16_t> {
  static __device__ __forceinline__ void ld(const uint16_t* p, size_t i, float (&v)[4]) {
    const uint2 r = *reinterpret_cast<const uint2*>(p + i);
    v[0] = __uint_as_float(r.x << 16), v[1] = __uint_as_float(r.x & 0xffff0000u);
    v[2] = __uint_as_float(r.y << 16), v[3] = __uint_as_float(r.y & 0xffff0000u);
  }
  static __device__ __forceinline__ void st(uint16_t* p, size_t i, const float (&v)[4]) {
    uint2 r;
    r.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
    r.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
    *reinterpret_cast<uint2*>(p + i) = r;
  }
};
template <>
struct Vec4<float> {
  static __device__ __forceinline__ void ld(const float* p, size_t i, float (&v)[4]) {
    const float4 r = *reinterpret_cast<const float4*>(p + i);
    v[0] = r.x, v[1] = r.y, v[2] = r.z, v[3] = r.w;
  }
  static __device__ __forceinline__ void st(float* p, size_t i, const float (&v)[4]) {
    *reinterpret_cast<float4*>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
  }
};

// The grid-stride loop of every elementwise kernel here, as a loop header in front of the kernel's own body: i = lo + W * thread,
// stepping W * (threads of the grid), while i < hi -- W elements per thread per trip.  A macro, not a function that takes the body
// as a lambda, because of the code hipcc generates: blockDim.x read in a device function goes through the partial-last-workgroup
// path that a kernel body is spared, and with the body inlined from a callee the CFG instantiations address their loads with six
// to eight more VGPRs (always_inline, [=] captures and indices passed in do not help).  Expanded in place the header gives the
// code of a loop written out by hand.
#define EW_SPAN(i, W, lo, hi)                                                             \
  for (size_t i = (lo) + ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * (W); i < (hi); \
       i += (size_t)gridDim.x * blockDim.x * (W))
// scalar form: one element per thread per trip over [0, n)
#define EW_EACH(i, n) EW_SPAN(i, 1, 0, n)
// "4-wide body + scalar tail" form: EW_EACH4's body takes elements [i, i + 4) of the leading n_vec (a multiple of 4, see
// vec_split), EW_TAIL's body element i of the rest; both must run the same per-element arithmetic.
#define EW_EACH4(i, n_vec) EW_SPAN(i, 4, 0, n_vec)
#define EW_TAIL(i, n_vec, n) EW_SPAN(i, 1, n_vec, n)

// noise_pred = uncond + g * (text - uncond), every op in the tensor dtype
template <typename T>
__device__ __forceinline__ float cfg_combine(float u, float c, float g) {
  const float d = IO<T>::rnd(__fsub_rn(c, u));
  const float gd = IO<T>::rnd(__fmul_rn(g, d));
  return IO<T>::rnd(__fadd_rn(u, gd));
}

// eps layout with CFG: [2][n] = (uncond, cond); without: [n]
template <typename T, bool CFG>
__device__ __forceinline__ float load_eps(const T* eps, size_t i, size_t n, float g) {
  if (CFG) return cfg_combine<T>(IO<T>::ld(eps, i), IO<T>::ld(eps, n + i), g);
  return IO<T>::ld(eps, i);
}
// the same for elements [i, i + 4) through 4-wide loads, into `float e[4]`.  A macro for the reason EW_SPAN is one: as a
// function it changes the vector loops of the CFG instantiations of both kernels that use it (up to 8 more VGPRs).
#define LOAD_EPS4(T, CFG, eps, i, n, g, e)                                                \
  {                                                                                       \
    if (CFG) {                                                                            \
      float u[4], c[4];                                                                   \
      Vec4<T>::ld(eps, i, u), Vec4<T>::ld(eps, (n) + (i), c);                             \
      _Pragma("unroll") for (int j = 0; j < 4; ++j) e[j] = cfg_combine<T>(u[j], c[j], g); \
    } else {                                                                              \
      Vec4<T>::ld(eps, i, e);                                                             \
    }                                                                                     \
  }

// element i of an n-element tensor, stored `rep` times along the batch (torch.cat([x] * rep) fused)
template <typename T>
__device__ __forceinline__ void store_rep(T* out, size_t i, size_t n, int rep, float v) {
  for (int r = 0; r < rep; ++r) IO<T>::st(out, (size_t)r * n + i, v);
}

// pred_original_sample of the alpha / beta schedulers (DDIM, DDPM, LCM) from cb = sqrt(beta_t), ca = sqrt(alpha_t), the model
// output e and the sample s, every op rounded in the tensor dtype.  PRED: 0 epsilon, 1 v_prediction, 2 sample
//   PRED 0   x0 = (s - cb * e) / ca        PRED 1   x0 = ca * s - cb * e        PRED 2   x0 = e
// (scheduling_ddim.py:455-468, scheduling_ddpm.py:505-517, scheduling_lcm.py step())
template <typename T, int PRED>
__device__ __forceinline__ float x0_alpha_beta(float cb, float ca, float e, float s) {
  if (PRED == 0) {
    float x0 = IO<T>::rnd(__fmul_rn(cb, e));
    x0 = IO<T>::rnd(__fsub_rn(s, x0));
    return IO<T>::rnd(__fdiv_rn(x0, ca));
  }
  if (PRED == 1) return IO<T>::rnd(__fsub_rn(IO<T>::rnd(__fmul_rn(ca, s)), IO<T>::rnd(__fmul_rn(cb, e))));
  return e;
}

// pred_original_sample (fp32) of the sigma schedulers (Euler, Euler ancestral); PRED as above
// (scheduling_euler_discrete.py:760-775)
struct EulerCoef {
  float sigma, dt, c_out, s2p1;
};

template <typename T, int PRED>
__device__ __forceinline__ float x0_sigma(const EulerCoef& k, float e, float s) {
  if (PRED == 0) return __fsub_rn(s, IO<T>::rnd(__fmul_rn(k.sigma, e)));  // sample - sigma_hat * model_output  (model dtype)
  // model_output * (-sigma / sqrt(sigma^2+1)) (model dtype) + sample / (sigma^2+1) (fp32)
  if (PRED == 1) return __fadd_rn(IO<T>::rnd(__fmul_rn(e, k.c_out)), __fdiv_rn(s, k.s2p1));
  return e;
}

// rescale_noise_cfg (pipelines/stable_diffusion/pipeline_stable_diffusion.py:69-92), used when guidance_rescale > 0:
//   std_text = noise_pred_text.std(dims 1..)   std_cfg = noise_cfg.std(dims 1..)         (unbiased, per sample)
//   noise_cfg = guidance_rescale * (noise_cfg * (std_text / std_cfg)) + (1 - guidance_rescale) * noise_cfg
// Pass 1: one workgroup per sample sums x and x^2 of the text prediction and of the CFG combination (fp64 accumulators:
// torch reduces a bf16 tensor in fp32 and rounds the RESULT to the tensor dtype, so what has to match is the rounded std)
// and stores ratio = rnd(rnd(std_text) / rnd(std_cfg)).  Pass 2: the combination again (same roundings as cfg_combine), then
// every product / sum of the formula rounded in the tensor dtype.  eps layout [2][B][n_per] = (uncond, cond).
template <typename T>
__global__ __launch_bounds__(1024) void cfg_rescale_stats_kernel(const T* __restrict__ eps, float* __restrict__ ratio, float g,
                                                                 size_t n_per, int B) {
  const int b = blockIdx.x;
  const T* u = eps + (size_t)b * n_per;
  const T* c = eps + ((size_t)B + b) * n_per;
  double st = 0, st2 = 0, sc = 0, sc2 = 0;
  for (size_t i = threadIdx.x; i < n_per; i += blockDim.x) {
    const float tv = IO<T>::ld(c, i);
    const float cv = cfg_combine<T>(IO<T>::ld(u, i), tv, g);
    st += tv; st2 += (double)tv * tv;
    sc += cv; sc2 += (double)cv * cv;
  }
  __shared__ double red[4][16];
  double v[4] = {st, st2, sc, sc2};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) { red[0][wave] = v[0]; red[1][wave] = v[1]; red[2][wave] = v[2]; red[3][wave] = v[3]; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t[4] = {0, 0, 0, 0};
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { t[0] += red[0][w]; t[1] += red[1][w]; t[2] += red[2][w]; t[3] += red[3][w]; }
    const double n = (double)n_per;
    const double var_t = fmax((t[1] - t[0] * t[0] / n) / (n - 1.0), 0.0), var_c = fmax((t[3] - t[2] * t[2] / n) / (n - 1.0), 0.0);
    const float std_t = IO<T>::rnd((float)sqrt(var_t)), std_c = IO<T>::rnd((float)sqrt(var_c));
    ratio[b] = IO<T>::rnd(__fdiv_rn(std_t, std_c));
  }
}

template <typename T>
__global__ void cfg_rescale_apply_kernel(const T* __restrict__ eps, T* __restrict__ out, const float* __restrict__ ratio,
                                         float g, float gr, float one_minus_gr, size_t n_per, size_t n) {
  EW_EACH(i, n) {
    const float cv = cfg_combine<T>(IO<T>::ld(eps, i), IO<T>::ld(eps, n + i), g);
    const float resc = IO<T>::rnd(__fmul_rn(cv, ratio[i / n_per]));
    const float a = IO<T>::rnd(__fmul_rn(gr, resc));
    const float b = IO<T>::rnd(__fmul_rn(one_minus_gr, cv));
    IO<T>::st(out, i, __fadd_rn(a, b));
  }
}

// InstructPix2Pix's three-way guidance (pipeline_stable_diffusion_instruct_pix2pix.py, the `do_classifier_free_guidance` branch of
// the denoising loop; the SDXL pipeline has the same expression):
//   noise_pred = noise_pred_uncond + guidance_scale * (noise_pred_text - noise_pred_image)
//                                  + image_guidance_scale * (noise_pred_image - noise_pred_uncond)
// eps layout [3][n] = (text, image, uncond).  Python evaluates it left to right, every op rounded in the tensor dtype:
//   rnd(rnd(u + rnd(g * rnd(t - i))) + rnd(ig * rnd(i - u)))
// -- five torch launches in the reference, one here; the step kernel that follows runs with cfg = 0.
template <typename T>
__global__ void cfg_combine3_kernel(const T* __restrict__ eps, T* __restrict__ out, float g, float ig, size_t n) {
  EW_EACH(i, n) {
    const float t = IO<T>::ld(eps, i), im = IO<T>::ld(eps, n + i), u = IO<T>::ld(eps, 2 * n + i);
    const float d_ti = IO<T>::rnd(__fsub_rn(t, im));
    const float left = IO<T>::rnd(__fadd_rn(u, IO<T>::rnd(__fmul_rn(g, d_ti))));
    const float d_iu = IO<T>::rnd(__fsub_rn(im, u));
    const float right = IO<T>::rnd(__fmul_rn(ig, d_iu));
    IO<T>::st(out, i, __fadd_rn(left, right));
  }
}

// Euler (gamma = 0): table row = [sigma, sigma_next, dt, sqrt(sigma^2+1), c_out, sigma^2+1, -, timestep]
// PRED: 0 epsilon, 1 v_prediction, 2 sample (scheduling_euler_discrete.py:760-775)
template <typename T, int PRED>
__device__ __forceinline__ float euler_one(const EulerCoef& k, float e, float s) {
  const float x0 = x0_sigma<T, PRED>(k, e, s);               // pred_original_sample (fp32); s = sample.to(float32)
  const float der = __fdiv_rn(__fsub_rn(s, x0), k.sigma);    // derivative
  return __fadd_rn(s, __fmul_rn(der, k.dt));
}

template <typename T, bool CFG, int PRED>
__global__ void euler_step_kernel(const T* __restrict__ eps, const T* __restrict__ x, T* __restrict__ out,
                                  const float* __restrict__ table, const int* __restrict__ step_idx, float g,
                                  size_t n) {
  const float* row = table + (size_t)(*step_idx) * 8;
  const EulerCoef k = {row[0], row[2], row[4], row[5]};
  EW_EACH(i, n) {
    const float e = load_eps<T, CFG>(eps, i, n, g);
    IO<T>::st(out, i, euler_one<T, PRED>(k, e, IO<T>::ld(x, i)));
  }
}

// scale_model_input for Euler, replicated `rep` times along batch (torch.cat([latents] * 2))
template <typename T>
__global__ void euler_scale_input_kernel(const T* __restrict__ x, T* __restrict__ out, const float* __restrict__ table,
                                         const int* __restrict__ step_idx, int rep, size_t n) {
  const float den = table[(size_t)(*step_idx) * 8 + 3];
  EW_EACH(i, n) store_rep<T>(out, i, n, rep, __fdiv_rn(IO<T>::ld(x, i), den));
}

// DDIM / DDPM: row = [sqrt(beta_t), sqrt(alpha_t), k0, ke, kx, kn, clip_range(0=off), timestep]
//   PRED 0 (epsilon)       x0 = (x - sqrt(beta_t) * out) / sqrt(alpha_t)                 pred_eps = out
//   PRED 1 (v_prediction)  x0 = sqrt(alpha_t) * x - sqrt(beta_t) * out                   pred_eps = sqrt(alpha_t) * out + sqrt(beta_t) * x
//   PRED 2 (sample)        x0 = out                                                      pred_eps = (x - sqrt(alpha_t) * x0) / sqrt(beta_t)
//   (scheduling_ddim.py:455-468, scheduling_ddpm.py:505-517; pred_eps is formed from the UNCLIPPED x0, as the reference
//   does unless use_clipped_model_output)
//   prev = k0*x0 [clamped] (+ ke*pred_eps) (+ kx*x) (+ kn*noise)     each product / sum rounded in the tensor dtype
template <typename T, bool CFG, int PRED>
__global__ void x0_linear_step_kernel(const T* __restrict__ eps, const T* __restrict__ x, const T* __restrict__ noise,
                                      T* __restrict__ out, const float* __restrict__ table,
                                      const int* __restrict__ step_idx, float g, size_t n, size_t noise_step_stride) {
  const float* row = table + (size_t)(*step_idx) * 8;
  if (noise) noise += (size_t)(*step_idx) * noise_step_stride;  // pre-drawn per-step noise: graph-replay safe
  const float cb = row[0], ca = row[1], k0 = row[2], ke = row[3], kx = row[4], kn = row[5], clip = row[6];
  EW_EACH(i, n) {
    const float e = load_eps<T, CFG>(eps, i, n, g);
    const float s = IO<T>::ld(x, i);
    float x0 = x0_alpha_beta<T, PRED>(cb, ca, e, s), pe;
    if (PRED == 0)
      pe = e;
    else if (PRED == 1)
      pe = IO<T>::rnd(__fadd_rn(IO<T>::rnd(__fmul_rn(ca, e)), IO<T>::rnd(__fmul_rn(cb, s))));
    else
      pe = IO<T>::rnd(__fdiv_rn(IO<T>::rnd(__fsub_rn(s, IO<T>::rnd(__fmul_rn(ca, x0)))), cb));
    if (clip > 0.f) x0 = fminf(fmaxf(x0, -clip), clip);
    float acc = IO<T>::rnd(__fmul_rn(k0, x0));
    if (ke != 0.f) acc = IO<T>::rnd(__fadd_rn(acc, IO<T>::rnd(__fmul_rn(ke, pe))));
    if (kx != 0.f) acc = IO<T>::rnd(__fadd_rn(acc, IO<T>::rnd(__fmul_rn(kx, s))));
    if (kn != 0.f && noise) acc = IO<T>::rnd(__fadd_rn(acc, IO<T>::rnd(__fmul_rn(kn, IO<T>::ld(noise, i)))));
    IO<T>::st(out, i, acc);
  }
}

// Latent-consistency (LCM) step, schedulers/scheduling_lcm.py step():
//   row = [sqrt(1 - abar_t), sqrt(abar_t), c_out, c_skip, sqrt(abar_prev), sqrt(1 - abar_prev), clip_range(0=off), timestep]
//   x0       as x0_linear_step_kernel (epsilon / v_prediction / sample), clamped when clip > 0
//   denoised = c_out * x0 + c_skip * x
//   prev     = sqrt(abar_prev) * denoised + sqrt(1 - abar_prev) * noise       each product / sum rounded in the tensor dtype
// The last step of a schedule has slots 4, 5 = 1, 0: prev = denoised, and the noise row is not read.
template <typename T, bool CFG, int PRED>
__global__ void lcm_step_kernel(const T* __restrict__ eps, const T* __restrict__ x, const T* __restrict__ noise,
                                T* __restrict__ out, const float* __restrict__ table, const int* __restrict__ step_idx,
                                float g, size_t n, size_t noise_step_stride) {
  const float* row = table + (size_t)(*step_idx) * 8;
  noise += (size_t)(*step_idx) * noise_step_stride;
  const float cb = row[0], ca = row[1], c_out = row[2], c_skip = row[3], pa = row[4], pb = row[5], clip = row[6];
  EW_EACH(i, n) {
    const float e = load_eps<T, CFG>(eps, i, n, g);
    const float s = IO<T>::ld(x, i);
    float x0 = x0_alpha_beta<T, PRED>(cb, ca, e, s);
    if (clip > 0.f) x0 = fminf(fmaxf(x0, -clip), clip);
    float acc = IO<T>::rnd(__fadd_rn(IO<T>::rnd(__fmul_rn(c_out, x0)), IO<T>::rnd(__fmul_rn(c_skip, s))));
    if (pb != 0.f)
      acc = IO<T>::rnd(__fadd_rn(IO<T>::rnd(__fmul_rn(pa, acc)), IO<T>::rnd(__fmul_rn(pb, IO<T>::ld(noise, i)))));
    IO<T>::st(out, i, acc);
  }
}

// FlowMatch Euler: row = [sigma, sigma_next, dt, -, -, -, -, timestep]; prev = float(x) + (dt * v in model dtype), stored in
// the MODEL OUTPUT's dtype (scheduling_flow_match_euler_discrete.py:484,:517: sample.to(float32) ... .to(model_output.dtype)).
// TX = dtype of the sample, TV = dtype of the model output and of `out` (TX = float, TV = bf16 is what the reference's
// Wan loop hands over on its first step).
template <typename TX, typename TV, bool CFG>
__global__ void flowmatch_step_kernel(const TV* __restrict__ v, const TX* __restrict__ x, TV* __restrict__ out,
                                      const float* __restrict__ table, const int* __restrict__ step_idx, float g,
                                      size_t n) {
  const float dt = table[(size_t)(*step_idx) * 8 + 2];
  EW_EACH(i, n) {
    const float e = load_eps<TV, CFG>(v, i, n, g);
    const float s = IO<TX>::ld(x, i);
    const float de = IO<TV>::rnd(__fmul_rn(dt, e));
    IO<TV>::st(out, i, __fadd_rn(s, de));
  }
}

// UniPC (B(h), predict-x0, flow prediction) step, orders 1 / 2 -- schedulers/scheduling_unipc_multistep.py:760-1300.
// One pass does convert_model_output, the corrector (multistep_uni_c_bh_update) and the predictor
// (multistep_uni_p_bh_update) and rolls the history IN PLACE: x <- next sample, last <- corrected sample,
// m2 <- m1, m1 <- this step's x0 prediction.  Every tensor op of the reference is reproduced with its rounding point
// (TX = dtype of the sample / history, TV = dtype of the model output; 0-d fp32 scalars never promote a tensor).
// coef row (16 floats): [sigma, use_corr, order_c, c1c, c2c, c3c, rk_c, rho0_c, rho_last_c, order_p, c1p, c2p, c3p, rk_p, -, -]
//   c1 = sigma_t / sigma_s0, c2 = alpha_t * h_phi_1, c3 = alpha_t * B_h   (corrector: t = i, s0 = i-1; predictor: t = i+1, s0 = i)
template <typename TX, typename TV, bool CFG>
__global__ void unipc_flow_step_kernel(const TV* __restrict__ v, TX* __restrict__ x, TX* __restrict__ last,
                                       TX* __restrict__ m1, TX* __restrict__ m2, const float* __restrict__ coef,
                                       const int* __restrict__ step_idx, float g, size_t n) {
  const float* r = coef + (size_t)(*step_idx) * 16;
  const float sigma = r[0];
  const bool use_corr = r[1] != 0.f;
  const int order_c = (int)r[2], order_p = (int)r[9];
  const float c1c = r[3], c2c = r[4], c3c = r[5], rk_c = r[6];
  const float rho0 = IO<TX>::rnd(r[7]), rhol = IO<TX>::rnd(r[8]);   // rhos_c is a tensor of the sample dtype
  const float c1p = r[10], c2p = r[11], c3p = r[12], rk_p = r[13];
  EW_EACH(i, n) {
    const float e = load_eps<TV, CFG>(v, i, n, g);
    const float xs = IO<TX>::ld(x, i);
    const float m1o = IO<TX>::ld(m1, i);
    const float se = IO<TV>::rnd(__fmul_rn(sigma, e));
    const float mn = IO<TX>::rnd(__fsub_rn(xs, se));                        // x0_pred = sample - sigma * model_output
    float xc = xs;
    if (use_corr) {
      const float t1 = IO<TX>::rnd(__fmul_rn(c1c, IO<TX>::ld(last, i)));
      const float t2 = IO<TX>::rnd(__fmul_rn(c2c, m1o));
      const float xt = IO<TX>::rnd(__fsub_rn(t1, t2));
      const float d1t = IO<TX>::rnd(__fsub_rn(mn, m1o));
      float inner = IO<TX>::rnd(__fmul_rn(rhol, d1t));
      if (order_c == 2) {
        float d = IO<TX>::rnd(__fsub_rn(IO<TX>::ld(m2, i), m1o));
        d = IO<TX>::rnd(__fdiv_rn(d, rk_c));
        const float corr = IO<TX>::rnd(__fmul_rn(rho0, d));
        inner = IO<TX>::rnd(__fadd_rn(corr, inner));
      }
      xc = IO<TX>::rnd(__fsub_rn(xt, IO<TX>::rnd(__fmul_rn(c3c, inner))));
    }
    const float p1 = IO<TX>::rnd(__fmul_rn(c1p, xc));
    const float p2 = IO<TX>::rnd(__fmul_rn(c2p, mn));
    float xn = IO<TX>::rnd(__fsub_rn(p1, p2));
    if (order_p == 2) {
      float d = IO<TX>::rnd(__fsub_rn(m1o, mn));
      d = IO<TX>::rnd(__fdiv_rn(d, rk_p));
      const float pred = IO<TX>::rnd(__fmul_rn(0.5f, d));
      xn = IO<TX>::rnd(__fsub_rn(xn, IO<TX>::rnd(__fmul_rn(c3p, pred))));
    }
    IO<TX>::st(m2, i, m1o);
    IO<TX>::st(m1, i, mn);
    IO<TX>::st(last, i, xc);
    IO<TX>::st(x, i, xn);
  }
}

// DPM-Solver++ (2M) step, orders 1 / 2 -- data-prediction multistep solver of Lu et al., "DPM-Solver++", Alg. 2; the
// scheduler (schedulers.py DPMSolverMultistepScheduler) evaluates every scalar on the host in fp64 and stores fp32 rows:
//   row = [alpha_s0, sigma_s0, cx, c0, cd, -, second_order_allowed, timestep]
//   x0  = (x - sigma_s0 e) / alpha_s0 (epsilon) | alpha_s0 x - sigma_s0 e (v_prediction) | e (sample)
//   x'  = cx x + c0 x0 [+ cd (x0 - m1)]        cx = sigma_t / sigma_s0, c0 = -alpha_t (exp(-h) - 1), cd = D1 coefficient / r0
// The second-order term is added only when the row allows it AND this is not the first step of the loop (step != begin: img2img
// and the refiner hand-off start past row 0 and replay the same graph), so stale history is never read.  fp32 arithmetic with
// one rounding at the store of x; the history m1 <- x0 stays fp32 (D1 is a difference of two nearby tensors).  TX = dtype of the
// sample, TV = dtype of the model output.
struct DpmCoef {
  float a0, b0, cx, c0, cd;
  bool second;
};

template <int PRED>
__device__ __forceinline__ float dpm_x0(const DpmCoef& k, float e, float xs) {
  if (PRED == 0) return __fdiv_rn(__fsub_rn(xs, __fmul_rn(k.b0, e)), k.a0);
  if (PRED == 1) return __fsub_rn(__fmul_rn(k.a0, xs), __fmul_rn(k.b0, e));
  return e;
}

__device__ __forceinline__ float dpm_update(const DpmCoef& k, float xs, float x0, float m1o) {
  float xn = __fadd_rn(__fmul_rn(k.cx, xs), __fmul_rn(k.c0, x0));
  if (k.second) xn = __fadd_rn(xn, __fmul_rn(k.cd, __fsub_rn(x0, m1o)));
  return xn;
}

// n_vec (a multiple of 4, 0 when a pointer is not 16-byte aligned or, with CFG, the cond half is not) elements go through
// 4-wide loads / stores, the rest through the scalar tail; both run the same per-element arithmetic.
template <typename TX, typename TV, bool CFG, int PRED>
__global__ void dpmpp_2m_step_kernel(const TV* __restrict__ eps, TX* __restrict__ x, float* __restrict__ m1,
                                     const float* __restrict__ table, const int* __restrict__ step_idx,
                                     const int* __restrict__ begin_idx, float g, size_t n, size_t n_vec) {
  const int step = *step_idx;
  const float* row = table + (size_t)step * 8;
  DpmCoef k;
  k.a0 = row[0], k.b0 = row[1], k.cx = row[2], k.c0 = row[3], k.cd = row[4];
  k.second = row[6] != 0.f && step != *begin_idx;
  EW_EACH4(i, n_vec) {
    float e[4], xs[4], mo[4], x0[4], xn[4];
    LOAD_EPS4(TV, CFG, eps, i, n, g, e);
    Vec4<TX>::ld(x, i, xs);
    if (k.second) Vec4<float>::ld(m1, i, mo);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x0[j] = dpm_x0<PRED>(k, e[j], xs[j]);
      xn[j] = dpm_update(k, xs[j], x0[j], k.second ? mo[j] : 0.f);
    }
    Vec4<float>::st(m1, i, x0);
    Vec4<TX>::st(x, i, xn);
  }
  EW_TAIL(i, n_vec, n) {
    const float e = load_eps<TV, CFG>(eps, i, n, g);
    const float xs = IO<TX>::ld(x, i);
    const float x0 = dpm_x0<PRED>(k, e, xs);
    const float xn = dpm_update(k, xs, x0, k.second ? m1[i] : 0.f);
    m1[i] = x0;
    IO<TX>::st(x, i, xn);
  }
}

// Second-order single-step samplers -- Heun (Karras et al. 2022, Alg. 1 without churn; HeunDiscreteScheduler) and DPM2 (k-diffusion
// sample_dpm_2; KDPM2DiscreteScheduler) -- as the reference models them: 2n - 1 schedule entries, predictor and corrector alternating,
// one model call per entry.  ONE kernel serves every entry; what an entry is stands in its row:
//   row = [sigma_eval, c_hist, dt_x, sqrt(sigma_eval^2+1), c_out, sigma_eval^2+1, phase, timestep]
// slots 0, 3, 4, 5, 7 are the Euler row (euler_scale_input_kernel and the U-Net's sinusoid read the same table).  With x0 = x0_sigma at
// sigma_eval and d = (x - x0) / sigma_eval:
//   phase 0 (Euler entry)   x <- x + dt_x d
//   phase 1 (predictor)     m1 <- x + c_hist d,  x <- x + dt_x d
//   phase 2 (corrector)     x <- m1 + dt_x d                                   (m1 is left as it is)
// Both samplers get by with the one fp32 buffer m1: Heun's x + dt (d + d') / 2 = (x + (dt/2) d) + (dt/2) d' (c_hist = dt/2, the
// corrector's dt_x = dt/2), DPM2's x + dt d_mid keeps m1 = x (c_hist = 0).  fp32 arithmetic, one rounding at the store of x, as
// dpmpp_2m_step_kernel; the phase is uniform over the launch.  TX = dtype of the sample, TV = dtype of the model output.
template <typename TV, int PRED>
__device__ __forceinline__ float sigma_slope(const EulerCoef& k, float e, float s) {
  return __fdiv_rn(__fsub_rn(s, x0_sigma<TV, PRED>(k, e, s)), k.sigma);
}

// n_vec as in dpmpp_2m_step_kernel.
template <typename TX, typename TV, bool CFG, int PRED>
__global__ void second_order_step_kernel(const TV* __restrict__ eps, TX* __restrict__ x, float* __restrict__ m1,
                                         const float* __restrict__ table, const int* __restrict__ step_idx, float g, size_t n,
                                         size_t n_vec) {
  const float* row = table + (size_t)(*step_idx) * 8;
  const EulerCoef k = {row[0], row[2], row[4], row[5]};
  const float c_hist = row[1];
  const int phase = (int)row[6];
  const bool predictor = phase == 1, corrector = phase == 2;
  EW_EACH4(i, n_vec) {
    float e[4], xs[4], base[4], h[4], xn[4];
    LOAD_EPS4(TV, CFG, eps, i, n, g, e);
    Vec4<TX>::ld(x, i, xs);
    if (corrector) Vec4<float>::ld(m1, i, base);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = sigma_slope<TV, PRED>(k, e[j], xs[j]);
      h[j] = __fadd_rn(xs[j], __fmul_rn(c_hist, d));
      xn[j] = __fadd_rn(corrector ? base[j] : xs[j], __fmul_rn(k.dt, d));
    }
    if (predictor) Vec4<float>::st(m1, i, h);
    Vec4<TX>::st(x, i, xn);
  }
  EW_TAIL(i, n_vec, n) {
    const float e = load_eps<TV, CFG>(eps, i, n, g);
    const float xs = IO<TX>::ld(x, i);
    const float d = sigma_slope<TV, PRED>(k, e, xs);
    const float base = corrector ? m1[i] : xs;
    if (predictor) m1[i] = __fadd_rn(xs, __fmul_rn(c_hist, d));
    IO<TX>::st(x, i, __fadd_rn(base, __fmul_rn(k.dt, d)));
  }
}

// Euler ancestral ("Euler a", schedulers/scheduling_euler_ancestral_discrete.py step):
//   row = [sigma, sigma_to, dt = sigma_down - sigma, sqrt(sigma^2+1), c_out, sigma^2+1, sigma_up, timestep]
// slots 0, 1, 3, 4, 5, 7 are the Euler row (euler_scale_input_kernel reads slot 3 of the same table); dt and sigma_up are evaluated
// by the scheduler with fp32 torch scalar ops.  PRED: 0 epsilon, 1 v_prediction.  Rounding points of the reference's op chain:
//   x0   = float(x) - T(sigma e)                      | T(e c_out) + float(x) / (sigma^2+1)        (products in the model dtype T)
//   prev = float(x) + ((float(x) - x0) / sigma) dt                                                  (fp32, each op rounded)
//   prev = prev + T(noise sigma_up)                                                                 (product in T, sum in fp32)
//   out  = T(prev)
// noise + *step_idx * noise_step_stride is this step's pre-drawn randn (stride 0: one buffer the host refills per step), so the
// step stays graph-replayable.  A row with sigma_up == 0 (the last one) skips the noise read: x + T(n * 0) == x.
template <typename T>
__device__ __forceinline__ float euler_a_noise(float sigma_up, float prev, float nz) {
  return __fadd_rn(prev, IO<T>::rnd(__fmul_rn(nz, sigma_up)));
}

// n_vec as in dpmpp_2m_step_kernel: the leading multiple of 4 elements when every base (the cond half and every noise row
// included) is 16-byte aligned, else 0; the rest runs the scalar tail.  `out` may alias `x`: a thread reads its elements first.
template <typename T, bool CFG, int PRED>
__global__ void euler_ancestral_step_kernel(const T* __restrict__ eps, const T* x, const T* __restrict__ noise, T* out,
                                            const float* __restrict__ table, const int* __restrict__ step_idx, float g,
                                            size_t n, size_t n_vec, size_t noise_step_stride) {
  const int step = *step_idx;
  const float* row = table + (size_t)step * 8;
  const EulerCoef k = {row[0], row[2], row[4], row[5]};
  const float sigma_up = row[6];
  noise += (size_t)step * noise_step_stride;
  const bool add = sigma_up != 0.f;   // uniform over the launch
  EW_EACH4(i, n_vec) {
    float e[4], xs[4], nz[4], o[4];
    LOAD_EPS4(T, CFG, eps, i, n, g, e);
    Vec4<T>::ld(x, i, xs);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = euler_one<T, PRED>(k, e[j], xs[j]);
    if (add) {
      Vec4<T>::ld(noise, i, nz);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = euler_a_noise<T>(sigma_up, o[j], nz[j]);
    }
    Vec4<T>::st(out, i, o);
  }
  EW_TAIL(i, n_vec, n) {
    const float e = load_eps<T, CFG>(eps, i, n, g);
    float o = euler_one<T, PRED>(k, e, IO<T>::ld(x, i));
    if (add) o = euler_a_noise<T>(sigma_up, o, IO<T>::ld(noise, i));
    IO<T>::st(out, i, o);
  }
}

// Inpainting with a 4-channel U-Net re-imposes the known region after every scheduler step
// (pipelines/stable_diffusion/pipeline_stable_diffusion_inpaint.py, the `num_channels_unet == 4` branch of the loop):
//   init_latents_proper = scheduler.add_noise(image_latents, noise, timesteps[i + 1])     (the clean latents after the last step)
//   latents = (1 - mask) * init_latents_proper + mask * latents
// One pass, in place over the latents, every bf16 rounding of the reference's op chain kept:
//   p = bf16(bf16(a x0) + bf16(b n))      out = bf16(bf16(bf16(1 - m) p) + bf16(m l))
// (a, b) = row *step_idx of `coef` ([rows][2] fp32, bf16-rounded values; last row (1, 0)).  The launch follows the scheduler step,
// which has advanced the counter: during step i the row read is i + 1.  The row index is clamped to the table.
// Layout: l / x0 / n [B][C][HW], mask [Bm][1][HW] with Bm in {1, B}.  VEC: eight elements per thread through 16-byte accesses
// (HW % 8 == 0, 16-byte aligned bases: a group of eight never straddles a (b, c) plane); otherwise one element per thread.
struct BlendCoef {
  float a, b;
};

__device__ __forceinline__ float inpaint_blend_one(const BlendCoef& k, float l, float x0, float n, float m) {
  const float p = bf2f(f2bf(__fadd_rn(bf2f(f2bf(__fmul_rn(k.a, x0))), bf2f(f2bf(__fmul_rn(k.b, n))))));
  const float om = bf2f(f2bf(__fsub_rn(1.0f, m)));
  return __fadd_rn(bf2f(f2bf(__fmul_rn(om, p))), bf2f(f2bf(__fmul_rn(m, l))));
}

template <bool VEC>
__global__ __launch_bounds__(256) void inpaint_blend_kernel(uint16_t* __restrict__ lat, const uint16_t* __restrict__ x0,
                                                            const uint16_t* __restrict__ noise, const uint16_t* __restrict__ mask,
                                                            const float* __restrict__ coef, const int* __restrict__ step_idx,
                                                            int n_rows, size_t chw, size_t hw, int mask_per_sample, size_t n) {
  const int row = min(max(*step_idx, 0), n_rows - 1);
  BlendCoef k;
  k.a = coef[2 * row], k.b = coef[2 * row + 1];
  if (VEC) {
    EW_SPAN(i, 8, 0, n) {
      const size_t b = i / chw, p = i % hw;
      const uint4 lq = *(const uint4*)(lat + i), xq = *(const uint4*)(x0 + i), nq = *(const uint4*)(noise + i);
      const uint4 mq = *(const uint4*)(mask + (mask_per_sample ? b * hw : 0) + p);
      float l[8], x[8], e[8], m[8], o[8];
      unpack8(lq, l), unpack8(xq, x), unpack8(nq, e), unpack8(mq, m);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = inpaint_blend_one(k, l[j], x[j], e[j], m[j]);
      *(uint4*)(lat + i) = pack8(o);
    }
  } else {
    EW_EACH(i, n) {
      const size_t b = i / chw, p = i % hw;
      const float m = bf2f(mask[(mask_per_sample ? b * hw : 0) + p]);
      lat[i] = f2bf(inpaint_blend_one(k, bf2f(lat[i]), bf2f(x0[i]), bf2f(noise[i]), m));
    }
  }
}

__global__ void advance_step_kernel(int* step_idx) { *step_idx += 1; }

// out = x * s in the tensor dtype (latents * init_noise_sigma, pipeline_stable_diffusion.py:713)
template <typename T>
__global__ void mul_scalar_kernel(const T* __restrict__ x, T* __restrict__ out, float sc, int rep, size_t n) {
  EW_EACH(i, n) store_rep<T>(out, i, n, rep, __fmul_rn(IO<T>::ld(x, i), sc));
}

// latents.to(transformer_dtype) (pipeline_wan.py:600) fused with the CFG batch doubling: fp32 -> bf16, `rep` copies
__global__ void cast_f32_bf16_kernel(const float* __restrict__ x, uint16_t* __restrict__ out, int rep, size_t n) {
  EW_EACH(i, n) store_rep<uint16_t>(out, i, n, rep, x[i]);
}

inline dim3 ew_grid(size_t n) {
  size_t b = (n + 255) / 256;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return dim3((unsigned)b);
}

// How a launch of the "4-wide body + scalar tail" form splits its n elements.  4-wide accesses need every base in `bases` (the
// OR of the operand pointers) 16-byte aligned, and so every offset the kernel adds to a base: the cond half of the model output,
// n elements of `esz` bytes in, when `cfg`, and a noise row, a multiple of `row_bytes` in.  n_vec = the leading multiple of 4
// when all are, else 0; work = what ew_grid has to cover, the longer of the two loops.
struct VecSplit {
  size_t n_vec, work;
};
inline VecSplit vec_split(uintptr_t bases, size_t esz, size_t n, bool cfg, size_t row_bytes = 0) {
  const bool aligned = bases % 16 == 0 && row_bytes % 16 == 0 && (!cfg || (n * esz) % 16 == 0);
  const size_t n_vec = aligned ? n - n % 4 : 0;
  return {n_vec, n_vec / 4 > n - n_vec ? n_vec / 4 : n - n_vec};
}

// Runtime (dtype, cfg, pred_type) -> template arguments.  Each level calls f with a tag value whose TYPE carries the choice and
// returns what f returns, so the innermost f launches, checks the launch and returns the status.
template <typename T>
struct Type {
  using type = T;
};
template <typename F>
int dispatch_dtype(int dtype, F f) {  // f(Type<uint16_t>) / f(Type<float>); any other dtype: DA_ERR_UNSUPPORTED, f not called
  if (dtype == DA_DTYPE_BF16) return f(Type<uint16_t>{});
  if (dtype == DA_DTYPE_F32) return f(Type<float>{});
  return DA_ERR_UNSUPPORTED;
}
template <typename F>
int dispatch_bool(bool b, F f) {  // f(std::true_type) / f(std::false_type)
  return b ? f(std::true_type{}) : f(std::false_type{});
}
template <int N, typename F>
int dispatch_int(int v, F f) {  // f(std::integral_constant<int, v>) for v in [0, N), which the caller has checked
  if constexpr (N > 1) {
    if (v != N - 1) return dispatch_int<N - 1>(v, f);
  }
  return f(std::integral_constant<int, N - 1>{});
}
// all three at once, for the step kernels templated on <T, CFG, PRED>: f(Type<T>, bool constant, int constant in [0, NPRED))
template <int NPRED, typename F>
int dispatch_step(int dtype, bool cfg, int pred, F f) {
  return dispatch_dtype(dtype, [&](auto t) {
    return dispatch_bool(cfg, [&](auto c) { return dispatch_int<NPRED>(pred, [&](auto p) { return f(t, c, p); }); });
  });
}
// the (sample TX, model output TV) pairs of the flow schedulers: bf16 / bf16, f32 / f32 and f32 / bf16; f(Type<TX>, Type<TV>)
template <typename F>
int dispatch_flow_dtypes(int x_dtype, int v_dtype, F f) {
  return dispatch_dtype(x_dtype, [&](auto tx) {
    return dispatch_dtype(v_dtype, [&](auto tv) {
      if constexpr (std::is_same_v<decltype(tx), Type<uint16_t>> && std::is_same_v<decltype(tv), Type<float>>)
        return DA_ERR_UNSUPPORTED;
      else
        return f(tx, tv);
    });
  });
}
template <typename Tag>
using type_of = typename Tag::type;

}  // namespace

extern "C" int da_euler_step(const void* eps, const void* x, void* out, const float* table, const int* step_idx,
                             int cfg, float guidance, long long n_, int dtype, int pred_type, void* stream) {
  if (!eps || !x || !out || !table || !step_idx || n_ <= 0) return DA_ERR_INVALID;
  if (pred_type < 0 || pred_type > 2) return DA_ERR_INVALID;
  const size_t n = (size_t)n_;
  hipStream_t s = (hipStream_t)stream;
  return dispatch_step<3>(dtype, cfg, pred_type, [&](auto t, auto c, auto p) {
    using T = type_of<decltype(t)>;
    DA_LAUNCH((euler_step_kernel<T, c.value, p.value>), ew_grid(n), dim3(256), 0, s, (const T*)eps, (const T*)x, (T*)out, table,
              step_idx, guidance, n);
    DA_CHECK_LAUNCH();
    return DA_OK;
  });
}

extern "C" int da_euler_scale_model_input(const void* x, void* out, const float* table, const int* step_idx, int rep,
                                          long long n_, int dtype, void* stream) {
  if (!x || !out || !table || !step_idx || n_ <= 0 || rep <= 0) return DA_ERR_INVALID;
  const size_t n = (size_t)n_;
  hipStream_t s = (hipStream_t)stream;
  return dispatch_dtype(dtype, [&](auto t) {
    using T = type_of<decltype(t)>;
    DA_LAUNCH((euler_scale_input_kernel<T>), ew_grid(n), dim3(256), 0, s, (const T*)x, (T*)out, table, step_idx, rep, n);
    DA_CHECK_LAUNCH();
    return DA_OK;
  });
}

extern "C" int da_x0_linear_step(const void* eps, const void* x, const void* noise, long long noise_step_stride,
                                 void* out, const float* table, const int* step_idx, int cfg, float guidance,
                                 long long n_, int dtype, int pred_type, void* stream) {
  if (!eps || !x || !out || !table || !step_idx || n_ <= 0 || noise_step_stride < 0) return DA_ERR_INVALID;
  // bit 2 (DA_PRED_LCM) selects the consistency update; the low bits stay the prediction type
  const bool lcm = (pred_type & 4) != 0;
  const int pred = pred_type & 3;
  if (pred_type < 0 || pred_type > 6 || pred > 2) return DA_ERR_INVALID;
  if (lcm && !noise) return DA_ERR_INVALID;
  const size_t n = (size_t)n_;
  hipStream_t s = (hipStream_t)stream;
  return dispatch_step<3>(dtype, cfg, pred, [&](auto t, auto c, auto p) {
    using T = type_of<decltype(t)>;
    const auto kernel = lcm ? lcm_step_kernel<T, c.value, p.value> : x0_linear_step_kernel<T, c.value, p.value>;
    DA_LAUNCH(kernel, ew_grid(n), dim3(256), 0, s, (const T*)eps, (const T*)x, (const T*)noise, (T*)out, table, step_idx,
              guidance, n, (size_t)noise_step_stride);
    DA_CHECK_LAUNCH();
    return DA_OK;
  });
}

extern "C" int da_flowmatch_step(const void* v, const void* x, void* out, const float* table, const int* step_idx,
                                 int cfg, float guidance, long long n_, int dtype, int x_dtype, void* stream) {
  if (!v || !x || !out || !table || !step_idx || n_ <= 0) return DA_ERR_INVALID;
  const size_t n = (size_t)n_;
  hipStream_t s = (hipStream_t)stream;
  return dispatch_flow_dtypes(x_dtype, dtype, [&](auto tx, auto tv) {
    return dispatch_bool(cfg, [&](auto c) {
      using TX = type_of<decltype(tx)>;
      using TV = type_of<decltype(tv)>;
      DA_LAUNCH((flowmatch_step_kernel<TX, TV, c.value>), ew_grid(n), dim3(256), 0, s, (const TV*)v, (const TX*)x, (TV*)out, table,
                step_idx, guidance, n);
      DA_CHECK_LAUNCH();
      return DA_OK;
    });
  });
}

extern "C" int da_cfg_rescale(const void* eps, void* out, float* ratio_ws, int B, long long n_per_, float guidance,
                              float guidance_rescale, int dtype, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (dtype & DA_CFG_IMAGE_GUIDANCE) {
    // three-way (text, image, uncond) guidance: `guidance_rescale` carries image_guidance_scale, no statistics, ratio_ws unused
    if (!eps || !out || B <= 0 || n_per_ <= 0) return DA_ERR_INVALID;
    const size_t n3 = (size_t)n_per_ * (size_t)B;
    return dispatch_dtype(dtype & ~DA_CFG_IMAGE_GUIDANCE, [&](auto t) {
      using T = type_of<decltype(t)>;
      DA_LAUNCH((cfg_combine3_kernel<T>), ew_grid(n3), dim3(256), 0, s, (const T*)eps, (T*)out, guidance, guidance_rescale, n3);
      DA_CHECK_LAUNCH();
      return DA_OK;
    });
  }
  if (!eps || !out || !ratio_ws || B <= 0 || n_per_ <= 1) return DA_ERR_INVALID;
  const size_t n_per = (size_t)n_per_, n = n_per * (size_t)B;
  const float omg = (float)(1.0 - (double)guidance_rescale);   // the reference forms (1 - guidance_rescale) in Python doubles
  return dispatch_dtype(dtype, [&](auto t) {
    using T = type_of<decltype(t)>;
    DA_LAUNCH((cfg_rescale_stats_kernel<T>), dim3(B), dim3(1024), 0, s, (const T*)eps, ratio_ws, guidance, n_per, B);
    DA_CHECK_LAUNCH();
    DA_LAUNCH((cfg_rescale_apply_kernel<T>), ew_grid(n), dim3(256), 0, s, (const T*)eps, (T*)out, ratio_ws, guidance,
              guidance_rescale, omg, n_per, n);
    DA_CHECK_LAUNCH();
    return DA_OK;
  });
}

extern "C" int da_advance_step(int* step_idx, void* stream) {
  if (!step_idx) return DA_ERR_INVALID;
  DA_LAUNCH(advance_step_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step_idx);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

extern "C" int da_mul_scalar(const void* x, void* out, float sc, int rep, long long n_, int dtype, void* stream) {
  if (!x || !out || n_ <= 0 || rep <= 0) return DA_ERR_INVALID;
  const size_t n = (size_t)n_;
  hipStream_t s = (hipStream_t)stream;
  return dispatch_dtype(dtype, [&](auto t) {
    using T = type_of<decltype(t)>;
    DA_LAUNCH((mul_scalar_kernel<T>), ew_grid(n), dim3(256), 0, s, (const T*)x, (T*)out, sc, rep, n);
    DA_CHECK_LAUNCH();
    return DA_OK;
  });
}

extern "C" int da_unipc_flow_step(const void* v, void* x, void* last, void* m1, void* m2, const float* coef,
                                  const int* step_idx, int cfg, float guidance, long long n_, int x_dtype, int v_dtype,
                                  void* stream) {
  if (!v || !x || !last || !m1 || !m2 || !coef || !step_idx || n_ <= 0) return DA_ERR_INVALID;
  const size_t n = (size_t)n_;
  hipStream_t s = (hipStream_t)stream;
  return dispatch_flow_dtypes(x_dtype, v_dtype, [&](auto tx, auto tv) {
    return dispatch_bool(cfg, [&](auto c) {
      using TX = type_of<decltype(tx)>;
      using TV = type_of<decltype(tv)>;
      DA_LAUNCH((unipc_flow_step_kernel<TX, TV, c.value>), ew_grid(n), dim3(256), 0, s, (const TV*)v, (TX*)x, (TX*)last, (TX*)m1,
                (TX*)m2, coef, step_idx, guidance, n);
      DA_CHECK_LAUNCH();
      return DA_OK;
    });
  });
}

extern "C" int da_dpmpp_2m_step(const void* eps, void* x, float* m1, const float* table, const int* step_idx,
                                const int* begin_idx, int cfg, float guidance, long long n_, int x_dtype, int e_dtype,
                                int pred_type, void* stream) {
  if (!eps || !x || !m1 || !table || !step_idx || !begin_idx || n_ <= 0) return DA_ERR_INVALID;
  // bit 3 (DA_PRED_SECOND_ORDER) selects the predictor / corrector step of Heun and DPM2; the low bits stay the prediction type
  const bool second_order = (pred_type & DA_PRED_SECOND_ORDER) != 0;
  const int pred = pred_type & ~DA_PRED_SECOND_ORDER;
  if (pred_type < 0 || pred < 0 || pred > 2) return DA_ERR_INVALID;
  if ((x_dtype != DA_DTYPE_BF16 && x_dtype != DA_DTYPE_F32) || (e_dtype != DA_DTYPE_BF16 && e_dtype != DA_DTYPE_F32))
    return DA_ERR_UNSUPPORTED;
  const size_t n = (size_t)n_;
  hipStream_t s = (hipStream_t)stream;
  // with CFG the cond half starts n elements in and n must be a multiple of 4, whatever the model output's dtype: the condition of
  // 4-byte elements (a bf16 model output is read 8 bytes at a time and would need no more)
  const VecSplit vs = vec_split((uintptr_t)eps | (uintptr_t)x | (uintptr_t)m1, sizeof(float), n, cfg);
  return dispatch_dtype(x_dtype, [&](auto tx) {
    return dispatch_step<3>(e_dtype, cfg, pred, [&](auto tv, auto c, auto p) {
      using TX = type_of<decltype(tx)>;
      using TV = type_of<decltype(tv)>;
      if (second_order) {
        DA_LAUNCH((second_order_step_kernel<TX, TV, c.value, p.value>), ew_grid(vs.work), dim3(256), 0, s, (const TV*)eps, (TX*)x,
                  m1, table, step_idx, guidance, n, vs.n_vec);
        DA_CHECK_LAUNCH();
        return DA_OK;
      }
      DA_LAUNCH((dpmpp_2m_step_kernel<TX, TV, c.value, p.value>), ew_grid(vs.work), dim3(256), 0, s, (const TV*)eps, (TX*)x, m1,
                table, step_idx, begin_idx, guidance, n, vs.n_vec);
      DA_CHECK_LAUNCH();
      return DA_OK;
    });
  });
}

extern "C" int da_euler_ancestral_step(const void* eps, const void* x, const void* noise, long long noise_step_stride,
                                       void* out, const float* table, const int* step_idx, int cfg, float guidance,
                                       long long n_, int dtype, int pred_type, void* stream) {
  if (!eps || !x || !noise || !out || !table || !step_idx || n_ <= 0 || noise_step_stride < 0) return DA_ERR_INVALID;
  if (pred_type < 0 || pred_type > 1) return DA_ERR_INVALID;
  if (dtype != DA_DTYPE_BF16 && dtype != DA_DTYPE_F32) return DA_ERR_UNSUPPORTED;
  const size_t n = (size_t)n_, esz = dtype == DA_DTYPE_BF16 ? 2 : 4;
  hipStream_t s = (hipStream_t)stream;
  // every base 16-byte aligned -- with CFG the cond half n elements in, and the noise row of any step
  const VecSplit vs = vec_split((uintptr_t)eps | (uintptr_t)x | (uintptr_t)noise | (uintptr_t)out, esz, n, cfg,
                                (size_t)noise_step_stride * esz);
  return dispatch_step<2>(dtype, cfg, pred_type, [&](auto t, auto c, auto p) {
    using T = type_of<decltype(t)>;
    DA_LAUNCH((euler_ancestral_step_kernel<T, c.value, p.value>), ew_grid(vs.work), dim3(256), 0, s, (const T*)eps, (const T*)x,
              (const T*)noise, (T*)out, table, step_idx, guidance, n, vs.n_vec, (size_t)noise_step_stride);
    DA_CHECK_LAUNCH();
    return DA_OK;
  });
}

extern "C" int da_cast_f32_bf16(const float* x, void* out, int rep, long long n_, void* stream) {
  if (!x || !out || n_ <= 0 || rep <= 0) return DA_ERR_INVALID;
  const size_t n = (size_t)n_;
  DA_LAUNCH(cast_f32_bf16_kernel, ew_grid(n), dim3(256), 0, (hipStream_t)stream, x, (uint16_t*)out, rep, n);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

extern "C" int da_inpaint_blend(void* latents, const void* image_latents, const void* noise, const void* mask, const float* coef,
                                const int* step_idx, int n_rows, int B, int C, long long HW, int Bm, void* stream) {
  if (!latents || !image_latents || !noise || !mask || !coef || !step_idx || n_rows <= 0 || B <= 0 || C <= 0 || HW <= 0)
    return DA_ERR_INVALID;
  if (Bm != 1 && Bm != B) return DA_ERR_INVALID;
  const size_t hw = (size_t)HW, chw = (size_t)C * hw, n = (size_t)B * chw;
  hipStream_t s = (hipStream_t)stream;
  const bool vec = hw % 8 == 0 && ((uintptr_t)latents | (uintptr_t)image_latents | (uintptr_t)noise | (uintptr_t)mask) % 16 == 0;
  return dispatch_bool(vec, [&](auto v) {
    DA_LAUNCH(inpaint_blend_kernel<v.value>, ew_grid(vec ? n / 8 : n), dim3(256), 0, s, (uint16_t*)latents,
              (const uint16_t*)image_latents, (const uint16_t*)noise, (const uint16_t*)mask, coef, step_idx, n_rows, chw, hw,
              Bm == B && B > 1 ? 1 : 0, n);
    DA_CHECK_LAUNCH();
    return DA_OK;
  });
}
