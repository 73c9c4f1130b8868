// K15: the kernels of the Stable-Diffusion cond stage, the CLIP text transformer behind FrozenCLIPEmbedder (reference
// "Stable Diffusion"/ldm/modules/encoders/modules.py:137-162; transformers' CLIPTextModel), beside the LayerNorm and 1x1-conv
// kernels it shares with the latent UNet:
//   adm_clip_embed         token_embedding[ids] + position_embedding[:T] -> 16-bit rows [N][pitch][C], pad rows zero
//   adm_attention_causal   softmax(q k^T / 8 + causal mask) v over 64-wide heads of a fused q | k | v projection
//   adm_quick_gelu         u * sigmoid(1.702 u)
//   adm_gelu               0.5 u (1 + erf(u / sqrt 2)): the exact GELU of the OpenCLIP text tower (Stable Diffusion 2.x)
//   adm_layernorm_f32out   the final LayerNorm, written as compact fp32 rows [N][T][C]
//
// Causal attention: one block of 4 waves per (prompt, head).  The head's K and V rows [0, T) are staged once, row-major, in LDS
// (rows T .. round-up-32(T) are written as zeros and never read from memory); wave w then owns the 16-query tiles w, w + 4, ...
// and walks the 32-key tiles 0 .. (q0 + 15) / 32 of each: a key tile that lies entirely above the diagonal of a query tile is
// never touched.  Per tile (all MFMAs v_mfma_f32_16x16x32 of the element type, as adm_attention_1h512):
//   S^T = K . Q^T    two 16-key halves x two 32-deep k-steps; lane (query lc, quarter lq) gets keys 16 h + 4 lq + r
//   softmax          fp32, running maximum and sum; in the diagonal tile (the only one that can hold keys above the diagonal or
//                    beyond T) a masked score is replaced BY VALUE: it does not enter the maximum and its weight is exactly 0
//   O^T += V^T . P^T V^T fragments through the transposing LDS read, which needs every lane active: the ragged last query tile
//                    runs with all 64 lanes (its queries >= T are zeros) and is masked at the store only.
// LDS row pitch 80 elements = 40 dwords = 8 (mod 16): the pitch adm_attention.hip uses for D = 64, conflict-free for the b128
// fragment reads (K) and the transposing reads (V).  2 x round-up-32(T) x 160 B: 30720 B at T = 77, 81920 B at T = 256.
#include "adm_attn_common.h"

namespace {

constexpr int CD = 64;          // head width
constexpr int CKT = 32;         // keys per tile
constexpr int CROW = CD + 16;   // LDS row pitch in elements
constexpr int CMAX_T = 256;
constexpr int CSMEM_MAX = 2 * CMAX_T * CROW * 2;

struct CausalK {
  const uint16_t* qkv; uint16_t* out;
  int T, pitch, heads;
  float scale_log2;   // log2(e) / 8: an fp32 multiply on the logits in front of the exponent (never folded into Q)
};

__global__ void __launch_bounds__(256)
attn_causal_kernel(const CausalK p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tpad = (p.T + CKT - 1) / CKT * CKT;
  uint16_t* Ks = reinterpret_cast<uint16_t*>(smem);
  uint16_t* Vs = Ks + tpad * CROW;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lc = lane & 15, lq = lane >> 4;
  const int h = blockIdx.x, n = blockIdx.y;
  const int C = p.heads * CD;
  const long long C3 = 3ll * C;
  const uint16_t* base = p.qkv + (long long)n * p.pitch * C3 + h * CD;

  // K and V rows of this head: 8 sixteen-byte units per row; rows >= T are zeros and are not read
  for (int u = tid; u < tpad * 8; u += 256) {
    const int r = u >> 3, sg = u & 7;
    uint4 kx = make_uint4(0, 0, 0, 0), vx = make_uint4(0, 0, 0, 0);
    if (r < p.T) {
      const uint16_t* row = base + r * C3 + sg * 8;
      kx = *reinterpret_cast<const uint4*>(row + C);
      vx = *reinterpret_cast<const uint4*>(row + 2 * C);
    }
    *reinterpret_cast<uint4*>(&Ks[r * CROW + sg * 8]) = kx;
    *reinterpret_cast<uint4*>(&Vs[r * CROW + sg * 8]) = vx;
  }
  __syncthreads();

  const int nqt = (p.T + 15) / 16;
  for (int qt = wave; qt < nqt; qt += 4) {   // wave-uniform: every lane stays active inside
    const int q0 = qt * 16, q = q0 + lc;
    // Q^T fragments: lane (query lc, quarter lq) holds Q[query][ks*32 + 8*lq .. +8]; queries >= T are zeros, not read
    adm_h8 qf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (q < p.T) v = *reinterpret_cast<const uint4*>(base + q * C3 + ks * 32 + lq * 8);
      qf[ks] = __builtin_bit_cast(adm_h8, v);
    }
    f32x4 oacc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -1e30f, l_run = 0.f;
    const int nkt = (q0 + 15) / CKT + 1;   // tiles with a key <= the tile's last query; the last one starts at k0 <= q0 < T
    for (int kt = 0; kt < nkt; ++kt) {
      const int k0 = kt * CKT;
      f32x4 s0 = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = f32x4{0.f, 0.f, 0.f, 0.f};
      const uint16_t* krow = &Ks[(k0 + lc) * CROW + lq * 8];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const adm_h8 ka = *reinterpret_cast<const adm_h8*>(krow + ks * 32);
        const adm_h8 kb = *reinterpret_cast<const adm_h8*>(krow + 16 * CROW + ks * 32);
        s0 = adm_mfma_16x16x32(ka, qf[ks], s0, 0, 0, 0);
        s1 = adm_mfma_16x16x32(kb, qf[ks], s1, 0, 0, 0);
      }
      // contraction slot 8*lq + e  <->  key k0 + 16*(e>>2) + 4*lq + (e&3): the order adm_tr_frag delivers V^T in.
      // Keys above the diagonal (key > query; for a query < T that covers every key >= T) exist in the diagonal tile only.
      const bool diag = k0 + CKT - 1 > q0;
      float sv[8];
      bool dead[8];
      float mx = -1e30f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        dead[e] = diag && (k0 + 16 * (e >> 2) + 4 * lq + (e & 3) > q);
        sv[e] = dead[e] ? -1e30f : (e < 4 ? s0[e & 3] : s1[e & 3]);
        mx = fmaxf(mx, sv[e]);
      }
      mx = adm_quarter_max(mx);
      const float m_new = fmaxf(m_run, mx);
      const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * p.scale_log2);
      m_run = m_new;
      float psum = 0.f;
      adm_h8 pf;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float pe = dead[e] ? 0.f : __builtin_amdgcn_exp2f((sv[e] - m_new) * p.scale_log2);
        psum += pe;
        pf[e] = (adm_elem_t)pe;
      }
      l_run = l_run * alpha + psum;
      // the rescale runs only where some query's maximum moved (wave-uniform branch; alpha is exactly 1 otherwise)
      if (__any(alpha != 1.0f)) {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) oacc[dt] *= alpha;
      }
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const adm_h8 vf = adm_tr_frag(Vs, CROW, k0, dt * 16, lc, lq);
        oacc[dt] = adm_mfma_16x16x32(vf, pf, oacc[dt], 0, 0, 0);
      }
    }
    // normalise and store: lane holds columns dt*16 + 4*lq .. +3 of query lc; rows >= T are not written
    const float inv = 1.0f / adm_quarter_sum(l_run);
    if (q < p.T) {
      uint16_t* orow = p.out + ((long long)n * p.pitch + q) * C + h * CD + lq * 4;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const f32x4 o = oacc[dt] * inv;
        uint2 pk;
        pk.x = adm_pack2(o[0], o[1]);
        pk.y = adm_pack2(o[2], o[3]);
        *reinterpret_cast<uint2*>(orow + dt * 16) = pk;
      }
    }
  }
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
  return make_uint4(adm_pack2(f[0], f[1]), adm_pack2(f[2], f[3]), adm_pack2(f[4], f[5]), adm_pack2(f[6], f[7]));
}

__device__ __forceinline__ void load8(const float* p, float* f) {
  *reinterpret_cast<float4*>(f) = *reinterpret_cast<const float4*>(p);
  *reinterpret_cast<float4*>(f + 4) = *reinterpret_cast<const float4*>(p + 4);
}

// one thread per 8 channels of an output row; the id is clamped into the table (ops checks the range on the host)
__global__ void __launch_bounds__(256)
clip_embed_kernel(const long long* __restrict__ ids, const float* __restrict__ tok, const float* __restrict__ pos,
                  uint16_t* __restrict__ out, long long items, int t, int pitch, int c, int vocab) {
  const int sg = c / 8;
  for (long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (long long)gridDim.x * blockDim.x) {
    const long long row = it / sg;
    const int i = (int)(it % sg);
    const long long n = row / pitch;
    const int r = (int)(row % pitch);
    uint4 pk = make_uint4(0, 0, 0, 0);
    if (r < t) {
      long long id = ids[n * t + r];
      id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
      float a[8], b[8], y[8];
      load8(tok + id * c + i * 8, a);
      load8(pos + (long long)r * c + i * 8, b);
#pragma unroll
      for (int j = 0; j < 8; ++j) y[j] = a[j] + b[j];
      pk = pack8(y);
    }
    *reinterpret_cast<uint4*>(out + row * c + i * 8) = pk;
  }
}

// u * sigmoid(1.702 u) = u * rcp(1 + 2^(-1.702 log2(e) u)) in fp32 (as adm_silu: v_exp_f32 + v_rcp_f32)
__global__ void __launch_bounds__(256)
quick_gelu_kernel(const uint16_t* __restrict__ u, uint16_t* __restrict__ out, long long items) {
  for (long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (long long)gridDim.x * blockDim.x) {
    float a[8], y[8];
    unpack8(*reinterpret_cast<const uint4*>(u + it * 8), a);
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = a[j] * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(a[j] * (-1.702f * 1.4426950408889634f)));
    *reinterpret_cast<uint4*>(out + it * 8) = pack8(y);
  }
}

// the exact GELU 0.5 u (1 + erf(u / sqrt 2)) in fp32, adm_geglu's gate factor (adm_sd.hip), rounded once to the element type
__global__ void __launch_bounds__(256)
gelu_kernel(const uint16_t* __restrict__ u, uint16_t* __restrict__ out, long long items) {
  for (long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (long long)gridDim.x * blockDim.x) {
    float a[8], y[8];
    unpack8(*reinterpret_cast<const uint4*>(u + it * 8), a);
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = 0.5f * a[j] * (1.0f + erff(a[j] * 0.70710678118654752f));
    *reinterpret_cast<uint4*>(out + it * 8) = pack8(y);
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// adm_sd.hip's layernorm_kernel (one wave per row, two-pass statistics) reading row t of prompt n at [n][pitch][C] and writing
// fp32 row n * T + t: the pad rows are dropped here
template <int SEGS>
__global__ void __launch_bounds__(256)
layernorm_f32out_kernel(const uint16_t* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                        float* __restrict__ out, long long rows, int t, int pitch, int c, float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nseg = c / 8;
  const float inv_c = 1.0f / (float)c;
  for (long long row = (long long)blockIdx.x * 4 + wave; row < rows; row += (long long)gridDim.x * 4) {
    const uint16_t* src = x + ((row / t) * pitch + row % t) * c;
    float v[SEGS][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < SEGS; ++i) {
      const int sg = lane + i * 64;
      if (sg < nseg) {
        unpack8(*reinterpret_cast<const uint4*>(src + sg * 8), v[i]);
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
    const float rstd = 1.0f / sqrtf(wave_sum(ss) * inv_c + eps);
#pragma unroll
    for (int i = 0; i < SEGS; ++i) {
      const int sg = lane + i * 64;
      if (sg < nseg) {
        float g8[8], b8[8], y[8];
        load8(gamma + sg * 8, g8);
        load8(beta + sg * 8, b8);
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] = (v[i][j] - mean) * rstd * g8[j] + b8[j];
        float* o = out + row * c + sg * 8;
        *reinterpret_cast<float4*>(o) = *reinterpret_cast<const float4*>(y);
        *reinterpret_cast<float4*>(o + 4) = *reinterpret_cast<const float4*>(y + 4);
      }
    }
  }
}

unsigned grid_for(long long items, int per_block) {
  long long blocks = (items + per_block - 1) / per_block;
  return (unsigned)(blocks > 16384 ? 16384 : blocks);
}

}  // namespace

extern "C" int adm_clip_embed(const int64_t* ids, const float* tok, const float* pos, adm_bf16* out, int n, int t, int pitch,
                              int c, int vocab, int positions, void* stream) {
  ADM_REQUIRE(ids && tok && pos && out, ADM_E_ARG, "adm_clip_embed: null pointer");
  ADM_REQUIRE(n > 0 && t > 0 && pitch >= t && vocab > 0 && t <= positions, ADM_E_ARG,
              "adm_clip_embed: bad shape n=%d t=%d pitch=%d vocab=%d positions=%d", n, t, pitch, vocab, positions);
  ADM_REQUIRE(c > 0 && c % 8 == 0, ADM_E_SHAPE, "adm_clip_embed: c=%d unsupported (c %% 8 == 0)", c);
  ADM_REQUIRE(adm_aligned16(tok) && adm_aligned16(pos) && adm_aligned16(out), ADM_E_ALIGN, "adm_clip_embed: unaligned pointer");
  const long long items = (long long)n * pitch * (c / 8);
  hipLaunchKernelGGL(clip_embed_kernel, dim3(grid_for(items, 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(ids), tok, pos, out, items, t, pitch, c, vocab);
  return adm_check_launch("adm_clip_embed");
}

extern "C" int adm_attention_causal(const adm_bf16* qkv, adm_bf16* out, int n, int t, int pitch, int heads, int d, void* stream) {
  ADM_REQUIRE(qkv && out, ADM_E_ARG, "adm_attention_causal: null pointer");
  ADM_REQUIRE(d == CD, ADM_E_SHAPE, "adm_attention_causal: head width %d unsupported (64 only)", d);
  ADM_REQUIRE(n > 0 && heads > 0 && t >= 1 && t <= CMAX_T && pitch >= t, ADM_E_SHAPE,
              "adm_attention_causal: bad shape n=%d t=%d (1..%d) pitch=%d heads=%d", n, t, CMAX_T, pitch, heads);
  ADM_REQUIRE(n < 65536 && heads <= 1024, ADM_E_SHAPE, "adm_attention_causal: n exceeds grid.y or more than 1024 heads");
  ADM_REQUIRE(adm_aligned16(qkv) && adm_aligned16(out), ADM_E_ALIGN, "adm_attention_causal: unaligned pointer");
  static thread_local int sized_for = -1;   // per device: the dynamic LDS at T > 192 exceeds the 64 KB default
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) ADM_FAIL((int)e, "adm_attention_causal: hipGetDevice: %s", hipGetErrorString(e));
  if (sized_for != dev) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_causal_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, CSMEM_MAX);
    if (e != hipSuccess) ADM_FAIL((int)e, "adm_attention_causal: hipFuncSetAttribute: %s", hipGetErrorString(e));
    sized_for = dev;
  }
  CausalK k{};
  k.qkv = qkv; k.out = out; k.T = t; k.pitch = pitch; k.heads = heads;
  k.scale_log2 = 1.4426950408889634f * 0.125f;
  const int tpad = (t + CKT - 1) / CKT * CKT;
  hipLaunchKernelGGL(attn_causal_kernel, dim3(heads, n), dim3(256), 2 * tpad * CROW * 2, (hipStream_t)stream, k);
  return adm_check_launch("adm_attention_causal");
}

extern "C" int adm_quick_gelu(const adm_bf16* u, adm_bf16* out, int64_t rows, int inner, void* stream) {
  ADM_REQUIRE(u && out, ADM_E_ARG, "adm_quick_gelu: null pointer");
  ADM_REQUIRE(rows > 0 && inner > 0 && inner % 8 == 0, ADM_E_SHAPE, "adm_quick_gelu: rows=%lld inner=%d unsupported", (long long)rows, inner);
  ADM_REQUIRE(adm_aligned16(u) && adm_aligned16(out), ADM_E_ALIGN, "adm_quick_gelu: unaligned pointer");
  const long long items = (long long)rows * (inner / 8);
  hipLaunchKernelGGL(quick_gelu_kernel, dim3(grid_for(items, 256)), dim3(256), 0, (hipStream_t)stream, u, out, items);
  return adm_check_launch("adm_quick_gelu");
}

extern "C" int adm_gelu(const adm_bf16* u, adm_bf16* out, int64_t rows, int inner, void* stream, int flags) {
  ADM_REQUIRE(flags == 0, ADM_E_ARG, "adm_gelu: flags=%d (must be 0)", flags);
  ADM_REQUIRE(u && out, ADM_E_ARG, "adm_gelu: null pointer");
  ADM_REQUIRE(rows > 0 && inner > 0 && inner % 8 == 0, ADM_E_SHAPE, "adm_gelu: rows=%lld inner=%d unsupported", (long long)rows, inner);
  ADM_REQUIRE(adm_aligned16(u) && adm_aligned16(out), ADM_E_ALIGN, "adm_gelu: unaligned pointer");
  const long long items = (long long)rows * (inner / 8);
  hipLaunchKernelGGL(gelu_kernel, dim3(grid_for(items, 256)), dim3(256), 0, (hipStream_t)stream, u, out, items);
  return adm_check_launch("adm_gelu");
}

extern "C" int adm_layernorm_f32out(const adm_bf16* x, const float* gamma, const float* beta, float* out, int n, int t, int pitch,
                                    int c, float eps, void* stream) {
  ADM_REQUIRE(x && gamma && beta && out, ADM_E_ARG, "adm_layernorm_f32out: null pointer");
  ADM_REQUIRE(n > 0 && t > 0 && pitch >= t, ADM_E_ARG, "adm_layernorm_f32out: bad shape n=%d t=%d pitch=%d", n, t, pitch);
  ADM_REQUIRE(c > 0 && c % 8 == 0 && c <= 2048, ADM_E_SHAPE, "adm_layernorm_f32out: c=%d unsupported (c %% 8 == 0, c <= 2048)", c);
  ADM_REQUIRE(adm_aligned16(x) && adm_aligned16(out) && adm_aligned16(gamma) && adm_aligned16(beta), ADM_E_ALIGN,
              "adm_layernorm_f32out: unaligned pointer");
  const long long rows = (long long)n * t;
  const dim3 grid(grid_for(rows, 4));
  hipStream_t s = (hipStream_t)stream;
  const int segs = (c / 8 + 63) / 64;
  if (segs <= 1) hipLaunchKernelGGL((layernorm_f32out_kernel<1>), grid, dim3(256), 0, s, x, gamma, beta, out, rows, t, pitch, c, eps);
  else if (segs == 2) hipLaunchKernelGGL((layernorm_f32out_kernel<2>), grid, dim3(256), 0, s, x, gamma, beta, out, rows, t, pitch, c, eps);
  else hipLaunchKernelGGL((layernorm_f32out_kernel<4>), grid, dim3(256), 0, s, x, gamma, beta, out, rows, t, pitch, c, eps);
  return adm_check_launch("adm_layernorm_f32out");
}
