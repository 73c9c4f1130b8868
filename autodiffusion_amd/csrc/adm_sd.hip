// Token-wise kernels of the Stable-Diffusion SpatialTransformer (gfx950): LayerNorm and GEGLU over bf16
// [rows][C] token tensors (rows = images x pixels; in NHWC a token IS a pixel, so the Linear layers around them
// are adm_conv 1x1 launches).  Both are single-pass HBM streams: 16-byte lanes, fp32 math.
// Reference: "Stable Diffusion"/ldm/modules/attention.py:196-215 (BasicTransformerBlock), 36-44 (GEGLU).
#include "adm_common.h"

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__device__ __forceinline__ void unpack8(const uint4 v, float* f) {
  const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = adm_lo_f32(u[j]);
    f[2 * j + 1] = adm_hi_f32(u[j]);
  }
}

__device__ __forceinline__ uint4 pack8(const float* f) {
  uint4 pk;
  pk.x = adm_pack2(f[0], f[1]);
  pk.y = adm_pack2(f[2], f[3]);
  pk.z = adm_pack2(f[4], f[5]);
  pk.w = adm_pack2(f[6], f[7]);
  return pk;
}

// One wave per token row; the row stays in registers between the mean, the variance (two-pass, as
// torch.nn.LayerNorm computes it) and the normalised store.  SEGS = 16-byte segments per lane (C <= 512 * SEGS).
template <int SEGS>
__global__ void __launch_bounds__(256)
layernorm_kernel(const uint16_t* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                 uint16_t* __restrict__ out, long long rows, int c, float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nseg = c / 8;
  const float inv_c = 1.0f / (float)c;
  for (long long row = (long long)blockIdx.x * 4 + wave; row < rows; row += (long long)gridDim.x * 4) {
    float v[SEGS][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < SEGS; ++i) {
      const int sg = lane + i * 64;
      if (sg < nseg) {
        unpack8(*reinterpret_cast<const uint4*>(x + row * c + sg * 8), v[i]);
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[i][j];
      }
    }
    const float mean = wave_sum(s) * inv_c;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < SEGS; ++i)
      if (lane + i * 64 < nseg) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float d = v[i][j] - mean;
          ss += d * d;
        }
      }
    const float rstd = rsqrtf(wave_sum(ss) * inv_c + eps);
#pragma unroll
    for (int i = 0; i < SEGS; ++i) {
      const int sg = lane + i * 64;
      if (sg < nseg) {
        float g8[8], b8[8], y[8];
        *reinterpret_cast<float4*>(g8) = *reinterpret_cast<const float4*>(gamma + sg * 8);
        *reinterpret_cast<float4*>(g8 + 4) = *reinterpret_cast<const float4*>(gamma + sg * 8 + 4);
        *reinterpret_cast<float4*>(b8) = *reinterpret_cast<const float4*>(beta + sg * 8);
        *reinterpret_cast<float4*>(b8 + 4) = *reinterpret_cast<const float4*>(beta + sg * 8 + 4);
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] = (v[i][j] - mean) * rstd * g8[j] + b8[j];
        *reinterpret_cast<uint4*>(out + row * c + sg * 8) = pack8(y);
      }
    }
  }
}

// out[r][i] = u[r][i] * gelu(u[r][inner + i]), exact (erf) GELU as F.gelu's default
__global__ void __launch_bounds__(256)
geglu_kernel(const uint16_t* __restrict__ u, uint16_t* __restrict__ out, long long rows, int inner) {
  const int sg = inner / 8;
  const long long items = rows * sg;
  for (long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (long long)gridDim.x * blockDim.x) {
    const long long r = it / sg;
    const int i = (int)(it % sg);
    float a[8], g[8], y[8];
    unpack8(*reinterpret_cast<const uint4*>(u + r * 2 * inner + i * 8), a);
    unpack8(*reinterpret_cast<const uint4*>(u + r * 2 * inner + inner + i * 8), g);
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = a[j] * (0.5f * g[j] * (1.0f + erff(g[j] * 0.70710678118654752f)));
    *reinterpret_cast<uint4*>(out + r * inner + i * 8) = pack8(y);
  }
}

}  // namespace

extern "C" int adm_layernorm(const adm_bf16* x, const float* gamma, const float* beta, adm_bf16* out, int64_t rows,
                             int c, float eps, void* stream) {
  ADM_REQUIRE(x && gamma && beta && out, ADM_E_ARG, "adm_layernorm: null pointer");
  ADM_REQUIRE(rows > 0 && c > 0 && c % 8 == 0 && c <= 2048, ADM_E_SHAPE, "adm_layernorm: rows=%lld c=%d unsupported (c %% 8 == 0, c <= 2048)",
              (long long)rows, c);
  ADM_REQUIRE(adm_aligned16(x) && adm_aligned16(out) && adm_aligned16(gamma) && adm_aligned16(beta), ADM_E_ALIGN,
              "adm_layernorm: unaligned pointer");
  long long blocks = (rows + 3) / 4;
  if (blocks > 16384) blocks = 16384;
  hipStream_t s = (hipStream_t)stream;
  const int segs = (c / 8 + 63) / 64;
  if (segs <= 1) hipLaunchKernelGGL((layernorm_kernel<1>), dim3((unsigned)blocks), dim3(256), 0, s, x, gamma, beta, out, (long long)rows, c, eps);
  else if (segs == 2) hipLaunchKernelGGL((layernorm_kernel<2>), dim3((unsigned)blocks), dim3(256), 0, s, x, gamma, beta, out, (long long)rows, c, eps);
  else hipLaunchKernelGGL((layernorm_kernel<4>), dim3((unsigned)blocks), dim3(256), 0, s, x, gamma, beta, out, (long long)rows, c, eps);
  return adm_check_launch("adm_layernorm");
}

extern "C" int adm_geglu(const adm_bf16* u, adm_bf16* out, int64_t rows, int inner, void* stream) {
  ADM_REQUIRE(u && out, ADM_E_ARG, "adm_geglu: null pointer");
  ADM_REQUIRE(rows > 0 && inner > 0 && inner % 8 == 0, ADM_E_SHAPE, "adm_geglu: rows=%lld inner=%d unsupported", (long long)rows, inner);
  ADM_REQUIRE(adm_aligned16(u) && adm_aligned16(out), ADM_E_ALIGN, "adm_geglu: unaligned pointer");
  const long long items = (long long)rows * (inner / 8);
  long long blocks = (items + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(geglu_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, u, out, (long long)rows, inner);
  return adm_check_launch("adm_geglu");
}

// ------------------------------------------------------------------------------------------------
// One latent sampler update ("Stable Diffusion"/ldm/models/diffusion/ddim.py:165-203 p_sample_ddim,
// plms.py:195-258 p_sample_plms): classifier-free guidance combine, multistep eps blend, pred_x0 and x_prev in one
// pass over the latents (fp32, 5-7 streams instead of ~12 separate elementwise launches).
//
// Parameterisations (adm_sd_step_p; PARAM is a template argument, so the eps instantiation is the kernel adm_sd_step always
// launched).  o = the guided RAW model output, combined by the expression above; then, each line one fp32 operation, left to
// right, compiled with fp contract(off):
//   ADM_PARAM_V    t1 = sqrt_at * o;  t2 = sqrt_one_minus_at * x;  e = t1 + t2
//                  pred_x0 without history and with w0 == 1 (DDIM):  s1 = sqrt_at * x;  s2 = sqrt_one_minus_at * o;  x0 = s1 - s2
//   ADM_PARAM_X0   t1 = sqrt_at * o;  t2 = x - t1;  e = t2 / sqrt_one_minus_at
//                  pred_x0 without history and with w0 == 1 (DDIM):  x0 = o
// e_out holds e (the PLMS history is eps); e', x_prev and pred_x0 with a history come from e by the eps expressions.
namespace {
struct SdStep {
  const float* x; const float* eu; const float* ec; const float* h1; const float* h2; const float* h3; const float* noise;
  float* x_prev; float* pred_x0; float* e_out;
  long long numel;
  float cfg, w0, w1, w2, w3, sqrt_one_minus_at, sqrt_at, sqrt_a_prev, dir_coef, sigma;
};

// e from the raw output o under V / X0, every operation rounded on its own
template <int PARAM>
__device__ __forceinline__ float sd_eps_of(float o, float x, float sqrt_at, float sqrt_one_minus_at) {
#pragma clang fp contract(off)
  if constexpr (PARAM == ADM_PARAM_V) {
    const float t1 = sqrt_at * o;
    const float t2 = sqrt_one_minus_at * x;
    return t1 + t2;
  } else {
    const float t1 = sqrt_at * o;
    const float t2 = x - t1;
    return t2 / sqrt_one_minus_at;
  }
}

__device__ __forceinline__ float sd_x0_of_v(float o, float x, float sqrt_at, float sqrt_one_minus_at) {
#pragma clang fp contract(off)
  const float s1 = sqrt_at * x;
  const float s2 = sqrt_one_minus_at * o;
  return s1 - s2;
}

template <int PARAM>
__global__ void __launch_bounds__(256)
sd_step_kernel(const SdStep p) {
  const bool direct_x0 = PARAM != ADM_PARAM_EPS && !p.h1 && !p.h2 && !p.h3 && p.w0 == 1.0f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < p.numel; i += (long long)gridDim.x * blockDim.x) {
    float e = p.ec[i];
    if (p.eu) {
      const float u = p.eu[i];
      e = u + p.cfg * (e - u);
    }
    const float o = e;
    if constexpr (PARAM != ADM_PARAM_EPS) e = sd_eps_of<PARAM>(o, p.x[i], p.sqrt_at, p.sqrt_one_minus_at);
    if (p.e_out) p.e_out[i] = e;
    float ep = p.w0 * e;
    if (p.h1) ep += p.w1 * p.h1[i];
    if (p.h2) ep += p.w2 * p.h2[i];
    if (p.h3) ep += p.w3 * p.h3[i];
    const float x0 = (p.x[i] - p.sqrt_one_minus_at * ep) / p.sqrt_at;
    float xp = p.sqrt_a_prev * x0 + p.dir_coef * ep;
    if (p.noise) xp += p.sigma * p.noise[i];
    p.x_prev[i] = xp;
    if (p.pred_x0) {
      float px0 = x0;
      if constexpr (PARAM == ADM_PARAM_V) {
        if (direct_x0) px0 = sd_x0_of_v(o, p.x[i], p.sqrt_at, p.sqrt_one_minus_at);
      } else if constexpr (PARAM == ADM_PARAM_X0) {
        if (direct_x0) px0 = o;
      }
      p.pred_x0[i] = px0;
    }
  }
}

int sd_step_launch(const char* who, const float* x, const float* eps_uncond, const float* eps_cond, const float* h1, const float* h2,
                   const float* h3, const float* noise, float* x_prev, float* pred_x0, float* e_out, int64_t numel,
                   const adm_sd_step_coefs* c, int param, void* stream) {
  ADM_REQUIRE(param == ADM_PARAM_EPS || param == ADM_PARAM_X0 || param == ADM_PARAM_V, ADM_E_ARG,
              "%s: param=%d (0 eps, 1 x0, 2 v)", who, param);
  ADM_REQUIRE(x && eps_cond && x_prev && c, ADM_E_ARG, "%s: null pointer", who);
  ADM_REQUIRE(numel > 0, ADM_E_ARG, "%s: empty tensor", who);
  ADM_REQUIRE(c->sqrt_at > 0.f, ADM_E_ARG, "%s: sqrt(alpha_t) must be positive", who);
  ADM_REQUIRE(param != ADM_PARAM_X0 || c->sqrt_one_minus_at > 0.f, ADM_E_ARG,
              "%s: sqrt(1 - alpha_t) must be positive under the x0 parameterisation", who);
  SdStep p{x, eps_uncond, eps_cond, h1, h2, h3, noise, x_prev, pred_x0, e_out, (long long)numel,
           c->cfg_scale, c->w[0], c->w[1], c->w[2], c->w[3], c->sqrt_one_minus_at, c->sqrt_at, c->sqrt_a_prev, c->dir_coef, c->sigma};
  long long blocks = (numel + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  const dim3 grid((unsigned)blocks);
  hipStream_t s = (hipStream_t)stream;
  if (param == ADM_PARAM_V) hipLaunchKernelGGL((sd_step_kernel<ADM_PARAM_V>), grid, dim3(256), 0, s, p);
  else if (param == ADM_PARAM_X0) hipLaunchKernelGGL((sd_step_kernel<ADM_PARAM_X0>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((sd_step_kernel<ADM_PARAM_EPS>), grid, dim3(256), 0, s, p);
  return adm_check_launch(who);
}
}  // namespace

extern "C" int adm_sd_step(const float* x, const float* eps_uncond, const float* eps_cond, const float* h1, const float* h2,
                           const float* h3, const float* noise, float* x_prev, float* pred_x0, float* e_out, int64_t numel,
                           const adm_sd_step_coefs* c, void* stream) {
  return sd_step_launch("adm_sd_step", x, eps_uncond, eps_cond, h1, h2, h3, noise, x_prev, pred_x0, e_out, numel, c, ADM_PARAM_EPS, stream);
}

extern "C" int adm_sd_step_p(const float* x, const float* out_uncond, const float* out_cond, const float* h1, const float* h2,
                             const float* h3, const float* noise, float* x_prev, float* pred_x0, float* e_out, int64_t numel,
                             const adm_sd_step_coefs* c, void* stream, int param) {
  return sd_step_launch("adm_sd_step_p", x, out_uncond, out_cond, h1, h2, h3, noise, x_prev, pred_x0, e_out, numel, c, param, stream);
}

// ------------------------------------------------------------------------------------------------
// One multistep DPM-Solver++ update in data-prediction form (dpm_solver.py:755-810 second order, 700-735 first order;
// model_wrapper's classifier-free guidance + data_prediction_fn :289-330, 380-400):
//   e = eu ? eu + cfg*(ec - eu) : ec;   m = (x - sigma_s*e) / alpha_s          (kept: the next step's model_prev)
//   x_next = a*x + b0*m + b1*m_prev
// Parameterisations (adm_dpm_step_p, model_wrapper's noise_pred_fn :297-306 folded into the data prediction); o = the guided raw
// output by the expression of e, then with fp contract(off), one fp32 operation each:
//   ADM_PARAM_V    t1 = alpha_s * x;  t2 = sigma_s * o;  m = t1 - t2
//   ADM_PARAM_X0   m = o
namespace {
struct DpmStep {
  const float* x; const float* eu; const float* ec; const float* m_prev;
  float* x_next; float* m_out;
  long long numel;
  float cfg, sigma_s, alpha_s, a, b0, b1;
};

// the data prediction of a guided raw output o under V / X0 (adm_dpm_step_p, adm_unipc_step_p)
template <int PARAM>
__device__ __forceinline__ float dpm_m_of(float o, float x, float alpha_s, float sigma_s) {
#pragma clang fp contract(off)
  if constexpr (PARAM == ADM_PARAM_V) {
    const float t1 = alpha_s * x;
    const float t2 = sigma_s * o;
    return t1 - t2;
  } else {
    return o;
  }
}

template <int PARAM>
__global__ void __launch_bounds__(256)
dpm_step_kernel(const DpmStep p) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < p.numel; i += (long long)gridDim.x * blockDim.x) {
    float e = p.ec[i];
    if (p.eu) {
      const float u = p.eu[i];
      e = u + p.cfg * (e - u);
    }
    const float x = p.x[i];
    float m;
    if constexpr (PARAM == ADM_PARAM_EPS) m = (x - p.sigma_s * e) / p.alpha_s;
    else m = dpm_m_of<PARAM>(e, x, p.alpha_s, p.sigma_s);
    float xn = p.a * x + p.b0 * m;
    if (p.m_prev) xn += p.b1 * p.m_prev[i];
    p.x_next[i] = xn;
    if (p.m_out) p.m_out[i] = m;
  }
}

int dpm_step_launch(const char* who, const float* x, const float* eps_uncond, const float* eps_cond, const float* m_prev, float* x_next,
                    float* m_out, int64_t numel, float cfg_scale, float sigma_s, float alpha_s, float a, float b0, float b1, int param,
                    void* stream) {
  ADM_REQUIRE(param == ADM_PARAM_EPS || param == ADM_PARAM_X0 || param == ADM_PARAM_V, ADM_E_ARG,
              "%s: param=%d (0 eps, 1 x0, 2 v)", who, param);
  ADM_REQUIRE(x && eps_cond && x_next, ADM_E_ARG, "%s: null pointer", who);
  ADM_REQUIRE(numel > 0 && alpha_s > 0.f, ADM_E_ARG, "%s: empty tensor or alpha_s <= 0", who);
  DpmStep p{x, eps_uncond, eps_cond, m_prev, x_next, m_out, (long long)numel, cfg_scale, sigma_s, alpha_s, a, b0, b1};
  long long blocks = (numel + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  const dim3 grid((unsigned)blocks);
  hipStream_t s = (hipStream_t)stream;
  if (param == ADM_PARAM_V) hipLaunchKernelGGL((dpm_step_kernel<ADM_PARAM_V>), grid, dim3(256), 0, s, p);
  else if (param == ADM_PARAM_X0) hipLaunchKernelGGL((dpm_step_kernel<ADM_PARAM_X0>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((dpm_step_kernel<ADM_PARAM_EPS>), grid, dim3(256), 0, s, p);
  return adm_check_launch(who);
}
}  // namespace

extern "C" int adm_dpm_step(const float* x, const float* eps_uncond, const float* eps_cond, const float* m_prev, float* x_next,
                            float* m_out, int64_t numel, float cfg_scale, float sigma_s, float alpha_s, float a, float b0,
                            float b1, void* stream) {
  return dpm_step_launch("adm_dpm_step", x, eps_uncond, eps_cond, m_prev, x_next, m_out, numel, cfg_scale, sigma_s, alpha_s, a, b0, b1,
                         ADM_PARAM_EPS, stream);
}

extern "C" int adm_dpm_step_p(const float* x, const float* out_uncond, const float* out_cond, const float* m_prev, float* x_next,
                              float* m_out, int64_t numel, float cfg_scale, float sigma_s, float alpha_s, float a, float b0,
                              float b1, void* stream, int param) {
  return dpm_step_launch("adm_dpm_step_p", x, out_uncond, out_cond, m_prev, x_next, m_out, numel, cfg_scale, sigma_s, alpha_s, a, b0, b1,
                         param, stream);
}

// ------------------------------------------------------------------------------------------------
// One model evaluation of UniPC (Zhao et al. 2023; autodiffusion_amd/unipc.py) in data-prediction form on the
// latents: adm_dpm_step's guided model value, then two states from host float64 coefficients,
//   e = eu ? eu + cfg*(ec - eu) : ec;   m = (x_eval - sigma_s*e) / alpha_s
//   x_c    = x_corr ? ac*x_base + c0*m + c1*h1 + c2*h2 + c3*h3 : x_eval     (the corrector of the update that arrived at x_eval)
//   x_pred = ap*x_c + p0*m + p1*h1 + p2*h2                                  (the predictor of the next update)
// fp32, left to right, no contraction: tests/unipc_ref.py restates exactly this sequence.  8-11 streams in one pass; two
// adm_dpm_step launches for the same two states would read x_eval, eps and the history twice.
// adm_unipc_step_p: m from the guided raw output as adm_dpm_step_p's (dpm_m_of above: V  t1 = alpha_s * x_eval; t2 = sigma_s * o;
// m = t1 - t2.  X0  m = o); everything after m, both VEC routes, is the same code.
namespace {
struct UniStep {
  const float* x; const float* eu; const float* ec; const float* xb; const float* h1; const float* h2; const float* h3;
  float* m_out; float* x_corr; float* x_pred;
  long long numel;
  float cfg, sigma_s, alpha_s, ac, c0, c1, c2, c3, ap, p0, p1, p2;
};

template <int VEC, int PARAM>
__global__ void __launch_bounds__(256)
unipc_step_kernel(const UniStep p) {
#pragma clang fp contract(off)
  const long long groups = p.numel / VEC;
  const bool states = p.x_corr || p.x_pred;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long long)gridDim.x * blockDim.x) {
    const long long i = g * VEC;
    float xv[VEC], cv[VEC], uv[VEC], bv[VEC], h1v[VEC], h2v[VEC], h3v[VEC], mv[VEC], xcv[VEC], xpv[VEC];
    if constexpr (VEC == 4) {
      *reinterpret_cast<float4*>(xv) = *reinterpret_cast<const float4*>(p.x + i);
      *reinterpret_cast<float4*>(cv) = *reinterpret_cast<const float4*>(p.ec + i);
      if (p.eu) *reinterpret_cast<float4*>(uv) = *reinterpret_cast<const float4*>(p.eu + i);
      if (p.x_corr) *reinterpret_cast<float4*>(bv) = *reinterpret_cast<const float4*>(p.xb + i);
      if (states) {
        if (p.h1) *reinterpret_cast<float4*>(h1v) = *reinterpret_cast<const float4*>(p.h1 + i);
        if (p.h2) *reinterpret_cast<float4*>(h2v) = *reinterpret_cast<const float4*>(p.h2 + i);
        if (p.h3 && p.x_corr) *reinterpret_cast<float4*>(h3v) = *reinterpret_cast<const float4*>(p.h3 + i);
      }
    } else {
      xv[0] = p.x[i];
      cv[0] = p.ec[i];
      if (p.eu) uv[0] = p.eu[i];
      if (p.x_corr) bv[0] = p.xb[i];
      if (states) {
        if (p.h1) h1v[0] = p.h1[i];
        if (p.h2) h2v[0] = p.h2[i];
        if (p.h3 && p.x_corr) h3v[0] = p.h3[i];
      }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float e = cv[j];
      if (p.eu) e = uv[j] + p.cfg * (e - uv[j]);
      float m;
      if constexpr (PARAM == ADM_PARAM_EPS) m = (xv[j] - p.sigma_s * e) / p.alpha_s;
      else m = dpm_m_of<PARAM>(e, xv[j], p.alpha_s, p.sigma_s);
      mv[j] = m;
      float xc = xv[j];
      if (p.x_corr) {
        xc = p.ac * bv[j] + p.c0 * m;
        if (p.h1) xc = xc + p.c1 * h1v[j];
        if (p.h2) xc = xc + p.c2 * h2v[j];
        if (p.h3) xc = xc + p.c3 * h3v[j];
      }
      xcv[j] = xc;
      float xp = p.ap * xc + p.p0 * m;
      if (p.h1) xp = xp + p.p1 * h1v[j];
      if (p.h2) xp = xp + p.p2 * h2v[j];
      xpv[j] = xp;
    }
    if constexpr (VEC == 4) {
      *reinterpret_cast<float4*>(p.m_out + i) = *reinterpret_cast<float4*>(mv);
      if (p.x_corr) *reinterpret_cast<float4*>(p.x_corr + i) = *reinterpret_cast<float4*>(xcv);
      if (p.x_pred) *reinterpret_cast<float4*>(p.x_pred + i) = *reinterpret_cast<float4*>(xpv);
    } else {
      p.m_out[i] = mv[0];
      if (p.x_corr) p.x_corr[i] = xcv[0];
      if (p.x_pred) p.x_pred[i] = xpv[0];
    }
  }
}
}  // namespace

namespace {
template <int PARAM>
void unipc_launch(bool vec4, unsigned blocks, hipStream_t s, const UniStep& p) {
  if (vec4) hipLaunchKernelGGL((unipc_step_kernel<4, PARAM>), dim3(blocks), dim3(256), 0, s, p);
  else hipLaunchKernelGGL((unipc_step_kernel<1, PARAM>), dim3(blocks), dim3(256), 0, s, p);
}

int unipc_step_launch(const char* who, const adm_unipc_args* a, int param, void* stream) {
  ADM_REQUIRE(param == ADM_PARAM_EPS || param == ADM_PARAM_X0 || param == ADM_PARAM_V, ADM_E_ARG,
              "%s: param=%d (0 eps, 1 x0, 2 v)", who, param);
  ADM_REQUIRE(a, ADM_E_ARG, "%s: null argument block", who);
  ADM_REQUIRE(a->x_eval && a->eps_cond && a->m_out, ADM_E_ARG, "%s: null x_eval / eps_cond / m_out", who);
  ADM_REQUIRE(!a->x_corr || a->x_base, ADM_E_ARG, "%s: x_corr without x_base", who);
  ADM_REQUIRE(a->numel > 0 && a->numel <= (1LL << 60) && a->alpha_s > 0.f, ADM_E_ARG, "%s: numel=%lld or alpha_s <= 0", who,
              (long long)a->numel);
  UniStep p{a->x_eval, a->eps_uncond, a->eps_cond, a->x_base, a->h1, a->h2, a->h3, a->m_out, a->x_corr, a->x_pred,
            (long long)a->numel, a->cfg_scale, a->sigma_s, a->alpha_s, a->ac, a->c0, a->c1, a->c2, a->c3, a->ap, a->p0, a->p1, a->p2};
  const bool states = a->x_corr || a->x_pred;
  const bool vec4 = (a->numel % 4 == 0) && adm_aligned16(a->x_eval) && adm_aligned16(a->eps_cond) && adm_aligned16(a->m_out) &&
                    (!a->eps_uncond || adm_aligned16(a->eps_uncond)) &&
                    (!a->x_corr || (adm_aligned16(a->x_corr) && adm_aligned16(a->x_base))) && (!a->x_pred || adm_aligned16(a->x_pred)) &&
                    (!states || ((!a->h1 || adm_aligned16(a->h1)) && (!a->h2 || adm_aligned16(a->h2)) &&
                                 (!a->h3 || adm_aligned16(a->h3))));
  const long long groups = vec4 ? a->numel / 4 : a->numel;
  long long blocks = (groups + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipStream_t s = (hipStream_t)stream;
  if (param == ADM_PARAM_V) unipc_launch<ADM_PARAM_V>(vec4, (unsigned)blocks, s, p);
  else if (param == ADM_PARAM_X0) unipc_launch<ADM_PARAM_X0>(vec4, (unsigned)blocks, s, p);
  else unipc_launch<ADM_PARAM_EPS>(vec4, (unsigned)blocks, s, p);
  return adm_check_launch(who);
}
}  // namespace

extern "C" int adm_unipc_step(const adm_unipc_args* a, void* stream, int flags) {
  ADM_REQUIRE(flags == 0, ADM_E_ARG, "adm_unipc_step: flags=%d (must be 0)", flags);
  return unipc_step_launch("adm_unipc_step", a, ADM_PARAM_EPS, stream);
}

extern "C" int adm_unipc_step_p(const adm_unipc_args* a, void* stream, int param) {
  return unipc_step_launch("adm_unipc_step_p", a, param, stream);
}
