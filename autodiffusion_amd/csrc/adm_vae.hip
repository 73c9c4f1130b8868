// K14: the three kernels the KL-f8 VAE decoder needs beside the conv / GroupNorm / attention kernels it shares with the UNets
// (reference "Stable Diffusion"/ldm/modules/diffusionmodules/model.py:462-568, ldm/models/autoencoder.py:303, 330-331):
//   adm_attention_1h512   the mid block's single-head attention of width 512 (model.py:186-198)
//   adm_vae_latent_in     z / scale_factor -> post_quant_conv (1x1) -> 16-bit NHWC padded to 32 channels (conv_in's operand)
//   adm_vae_image_out     clamp((x + 1) / 2, 0, 1) as fp32 NCHW and / or uint8 NHWC (scripts/search_ea.py:540, txt2img.py:337-339)
//
// Attention formulation (all MFMAs v_mfma_f32_16x16x32 of the element type) -- block-cooperative, 4 waves x 32 queries, 32-key
// tiles of K and V staged row-major in LDS:
//   S phase   wave w owns ONE 16 x 16 piece of the 32-query x 32-key score tile: query tile w & 1 (its Q^T fragments, 16 k-steps =
//             64 registers, are loaded once) against key half w >> 1 (K rows from LDS); two accumulation chains of 8 MFMAs.  The
//             raw fp32 scores go to a [32][32] LDS tile.
//   softmax   every wave reads the WHOLE score tile back (8 scores per lane and query tile) and runs the same fp32 online
//             softmax for all 32 queries: the four waves compute bit-identical maxima, sums and rescale factors, so nothing but S
//             is exchanged.  P is rounded to 16 bits straight into the B fragments of the second product.
//   PV phase  wave w owns the 128-column slab w of O for all 32 queries (2 x 8 accumulators = 64 registers): V^T fragments of its
//             slab come from the row-major LDS tile through the transposing read (adm_tr_frag), each used for both query tiles.
// Against one wave per 16 queries with all 512 columns (attn_wide_kernel's shape: 128 accumulator + 64 Q registers, every wave
// reading the whole K and V tiles) this holds 64 + 64 and reads K twice and V once per block and tile: 96 KB of LDS reads per
// 32 x 32 tile instead of 128 KB, at under 256 registers with the next tile's global loads in flight (64 staging registers).
#include <stdlib.h>

#include "adm_attn_common.h"

namespace {

constexpr int VD = 512;          // head width
constexpr int VKT = 32;          // keys per tile
constexpr int VQB = 32;          // queries per block
constexpr int VKROW = VD + 16;   // LDS row pitch in elements: 264 dwords = 8 (mod 16), conflict-free for the b128 fragment
                                 // reads and the transposing reads (as adm_attention.hip's PADE)
constexpr int VSROW = VKT + 4;   // fp32 score row pitch (16-byte aligned rows)
constexpr int VSMEM = 2 * VKT * VKROW * 2 + VQB * VSROW * 4;   // K | V | S = 72192 bytes: dynamic (static LDS stops at 64 KB)

struct Attn512K {
  const uint16_t* qkv; uint16_t* out;
  int T;
  float scale_log2;   // log2(e) / sqrt(512): an fp32 multiply in front of the exponent (adm_attention.hip: never folded into Q)
};

// launch bounds: 2 blocks per CU = 2 waves per SIMD caps the kernel at 256 registers, so the accumulators stay in VGPRs
// (adm_attention.hip: with no bound hipcc parks them in AGPRs); 2 x 70.5 KB of LDS fit the CU's 160 KB
__global__ void __launch_bounds__(256, 2)
attn_1h512_kernel(const Attn512K p) {
  constexpr int KS = VD / 32;   // 16 k-steps of QK^T
  constexpr int DT = 8;         // 16-column output tiles of a wave's 128-column slab
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint16_t* Ks = reinterpret_cast<uint16_t*>(smem);
  uint16_t* Vs = Ks + VKT * VKROW;
  float* Ss = reinterpret_cast<float*>(Vs + VKT * VKROW);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lc = lane & 15, lq = lane >> 4;
  int bx, by;
  adm_xcd_block(bx, by);
  const int n = by, qbase = bx * VQB;
  const int C3 = 3 * VD;
  const uint16_t* base = p.qkv + (long long)n * p.T * C3;
  // one descriptor over this image's T rows: queries / keys beyond T read as zeros (no bounds branches)
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, p.T * C3 * 2, 0x00020000);

  const int sqt = wave & 1, skh = wave >> 1;   // S phase: this wave's query tile and key half
  // Q^T fragments: lane (query lc, quarter lq) holds Q[query][ks*32 + 8*lq .. +8]
  adm_h8 qf[KS];
  {
    const int q = qbase + sqt * 16 + lc;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const adm_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, (q * C3 + ks * 32 + lq * 8) * 2, 0, 0);
      qf[ks] = __builtin_bit_cast(adm_h8, v);
    }
  }
  f32x4 oacc[DT][2];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) oacc[dt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run[2] = {-1e30f, -1e30f}, l_run[2] = {0.f, 0.f};

  AdmTileRegs<VKT, VD, 256> kr, vr;
  const int ntiles = (p.T + VKT - 1) / VKT;
  kr.load_buf(rs, C3, VD, 0, tid);
  vr.load_buf(rs, C3, 2 * VD, 0, tid);
  for (int kt0 = 0; kt0 < ntiles; ++kt0) {
    const int k0 = kt0 * VKT;
    __syncthreads();   // the previous tile's readers (V, S) are done
    kr.store(Ks, VKROW, tid);
    vr.store(Vs, VKROW, tid);
    if (kt0 + 1 < ntiles) {   // the next tile's loads fly during this tile's MFMAs
      kr.load_buf(rs, C3, VD, k0 + VKT, tid);
      vr.load_buf(rs, C3, 2 * VD, k0 + VKT, tid);
    }
    __syncthreads();
    // ---- S^T piece = K . Q^T: lane (query lc, quarter lq) gets keys skh*16 + 4*lq + r
    {
      f32x4 s0 = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = f32x4{0.f, 0.f, 0.f, 0.f};
      const uint16_t* krow = &Ks[(skh * 16 + lc) * VKROW + lq * 8];
#pragma unroll
      for (int ks = 0; ks < KS; ks += 2) {
        const adm_h8 k0f = *reinterpret_cast<const adm_h8*>(krow + ks * 32);
        const adm_h8 k1f = *reinterpret_cast<const adm_h8*>(krow + ks * 32 + 32);
        s0 = adm_mfma_16x16x32(k0f, qf[ks], s0, 0, 0, 0);
        s1 = adm_mfma_16x16x32(k1f, qf[ks + 1], s1, 0, 0, 0);
      }
      f32x4 s = s0 + s1;
      if (k0 + VKT > p.T) {   // keys beyond T (their K rows read as zeros): weight 0
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (k0 + skh * 16 + lq * 4 + r >= p.T) s[r] = -1e30f;
      }
      *reinterpret_cast<f32x4*>(&Ss[(sqt * 16 + lc) * VSROW + skh * 16 + lq * 4]) = s;
    }
    __syncthreads();
    // ---- online softmax of all 32 queries (identical in the four waves); contraction slot k = 8*lq + e  <->
    //      key 16*(e>>2) + 4*lq + (e&3), the order adm_tr_frag delivers V^T in
    adm_h8 pf[2];
    float alpha[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const float* srow = &Ss[(qt * 16 + lc) * VSROW + lq * 4];
      const f32x4 a = *reinterpret_cast<const f32x4*>(srow);
      const f32x4 b = *reinterpret_cast<const f32x4*>(srow + 16);
      float mx = fmaxf(fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3])), fmaxf(fmaxf(b[0], b[1]), fmaxf(b[2], b[3])));
      mx = adm_quarter_max(mx);
      const float m_new = fmaxf(m_run[qt], mx);
      alpha[qt] = __builtin_amdgcn_exp2f((m_run[qt] - m_new) * p.scale_log2);
      m_run[qt] = m_new;
      float psum = 0.f;
      adm_h8 f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float sv = e < 4 ? a[e & 3] : b[e & 3];
        const float pe = __builtin_amdgcn_exp2f((sv - m_new) * p.scale_log2);
        psum += pe;
        f[e] = (adm_elem_t)pe;
      }
      pf[qt] = f;
      l_run[qt] = l_run[qt] * alpha[qt] + psum;
    }
    // ---- O^T slab += V^T . P^T; the rescale runs only in tiles where some query's maximum moved (wave-uniform branch;
    //      alpha is exactly 1 otherwise, so skipping the multiplies changes no bit)
    if (__any(alpha[0] != 1.0f || alpha[1] != 1.0f)) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) oacc[dt][qt] *= alpha[qt];
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const adm_h8 vf = adm_tr_frag(Vs, VKROW, 0, wave * 128 + dt * 16, lc, lq);
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) oacc[dt][qt] = adm_mfma_16x16x32(vf, pf[qt], oacc[dt][qt], 0, 0, 0);
    }
  }
  // ---- normalise and store: lane holds columns wave*128 + dt*16 + 4*lq .. +3 of query lc
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const float l = adm_quarter_sum(l_run[qt]);
    const float inv = 1.0f / l;
    const int q = qbase + qt * 16 + lc;
    if (q >= p.T) continue;
    uint16_t* orow = p.out + ((long long)n * p.T + q) * VD + wave * 128;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const f32x4 o = oacc[dt][qt] * inv;
      uint2 pk;
      pk.x = adm_pack2(o[0], o[1]);
      pk.y = adm_pack2(o[2], o[3]);
      *reinterpret_cast<uint2*>(orow + dt * 16 + lq * 4) = pk;
    }
  }
}

// ---- latent entry: one thread per pixel; the 1x1 weights ride in LDS
constexpr int LAT_MAX_E = 16, LAT_CPAD = 32;

__global__ void __launch_bounds__(256)
latent_in_kernel(const float* __restrict__ z, const float* __restrict__ w, const float* __restrict__ b, float inv_scale,
                 uint16_t* __restrict__ out, long long pixels, int hw, int zc, int e) {
  __shared__ float ws[LAT_CPAD * LAT_MAX_E + LAT_CPAD];
  for (int i = threadIdx.x; i < zc * e; i += blockDim.x) ws[i] = w[i];
  for (int i = threadIdx.x; i < zc; i += blockDim.x) ws[LAT_CPAD * LAT_MAX_E + i] = b[i];
  __syncthreads();
  for (long long px = (long long)blockIdx.x * blockDim.x + threadIdx.x; px < pixels; px += (long long)gridDim.x * blockDim.x) {
    const long long img = px / hw;
    const int p = (int)(px % hw);
    float zs[LAT_MAX_E];
#pragma unroll
    for (int j = 0; j < LAT_MAX_E; ++j) zs[j] = j < e ? inv_scale * z[(img * e + j) * hw + p] : 0.f;
    uint32_t pk[LAT_CPAD / 2];
#pragma unroll
    for (int c2 = 0; c2 < LAT_CPAD / 2; ++c2) {
      float v[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int c = 2 * c2 + h;
        float acc = 0.f;
        if (c < zc) {
#pragma unroll
          for (int j = 0; j < LAT_MAX_E; ++j)
            if (j < e) acc = fmaf(ws[c * e + j], zs[j], acc);
          acc += ws[LAT_CPAD * LAT_MAX_E + c];
        }
        v[h] = acc;
      }
      pk[c2] = adm_pack2(v[0], v[1]);
    }
    uint4* o = reinterpret_cast<uint4*>(out + px * LAT_CPAD);
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = make_uint4(pk[4 * i], pk[4 * i + 1], pk[4 * i + 2], pk[4 * i + 3]);
  }
}

// ---- image exit: unit = min(max((x + 1) / 2, 0), 1) in exactly that order, no FMA contraction (as adm_sampler.hip)
__global__ void __launch_bounds__(256)
image_out_kernel(const float* __restrict__ x, float* __restrict__ unit, uint8_t* __restrict__ u8, long long pixels, int hw) {
#pragma clang fp contract(off)
  for (long long px = (long long)blockIdx.x * blockDim.x + threadIdx.x; px < pixels; px += (long long)gridDim.x * blockDim.x) {
    const long long img = px / hw;
    const int p = (int)(px % hw);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const long long xi = (img * 3 + ch) * hw + p;
      float v = (x[xi] + 1.0f) / 2.0f;
      v = fminf(fmaxf(v, 0.0f), 1.0f);
      if (unit) unit[xi] = v;
      if (u8) u8[px * 3 + ch] = (uint8_t)(255.0f * v);   // truncation, as .astype(np.uint8)
    }
  }
}

int grid_for(long long items) {
  long long blocks = (items + 255) / 256;
  return (int)(blocks > 8192 ? 8192 : blocks);
}

}  // namespace

extern "C" int adm_attention_1h512(const adm_bf16* qkv, adm_bf16* out, int n, int t, void* stream) {
  ADM_REQUIRE(qkv && out, ADM_E_ARG, "adm_attention_1h512: null pointer");
  ADM_REQUIRE(n > 0 && t > 0, ADM_E_ARG, "adm_attention_1h512: bad shape n=%d t=%d", n, t);
  ADM_REQUIRE(n < 65536, ADM_E_SHAPE, "adm_attention_1h512: n exceeds grid.y");
  ADM_REQUIRE((long long)t * 3 * VD * 2 < (1ll << 31), ADM_E_SHAPE,
              "adm_attention_1h512: an image's rows exceed the 32-bit byte offsets of a buffer descriptor");
  ADM_REQUIRE(adm_aligned16(qkv) && adm_aligned16(out), ADM_E_ALIGN, "adm_attention_1h512: unaligned pointer");
  static thread_local int sized_for = -1;   // per device: the kernel's dynamic LDS exceeds the 64 KB default
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) ADM_FAIL((int)e, "adm_attention_1h512: hipGetDevice: %s", hipGetErrorString(e));
  if (sized_for != dev) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_1h512_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, VSMEM);
    if (e != hipSuccess) ADM_FAIL((int)e, "adm_attention_1h512: hipFuncSetAttribute: %s", hipGetErrorString(e));
    sized_for = dev;
  }
  Attn512K k{};
  k.qkv = qkv; k.out = out; k.T = t;
  k.scale_log2 = 1.4426950408889634f / sqrtf((float)VD);
  hipLaunchKernelGGL(attn_1h512_kernel, dim3((t + VQB - 1) / VQB, n), dim3(256), VSMEM, (hipStream_t)stream, k);
  return adm_check_launch("adm_attention_1h512");
}

extern "C" int adm_vae_latent_in(const float* z, const float* w, const float* b, float inv_scale, adm_bf16* out, int n, int zc,
                                 int e, int h, int w_, void* stream) {
  ADM_REQUIRE(z && w && b && out, ADM_E_ARG, "adm_vae_latent_in: null pointer");
  ADM_REQUIRE(n > 0 && h > 0 && w_ > 0, ADM_E_ARG, "adm_vae_latent_in: bad shape n=%d h=%d w=%d", n, h, w_);
  ADM_REQUIRE(zc >= 1 && zc <= LAT_CPAD && e >= 1 && e <= LAT_MAX_E, ADM_E_SHAPE,
              "adm_vae_latent_in: z_channels %d (1..%d) / embed_dim %d (1..%d) unsupported", zc, LAT_CPAD, e, LAT_MAX_E);
  ADM_REQUIRE(adm_aligned16(out), ADM_E_ALIGN, "adm_vae_latent_in: unaligned output");
  const long long pixels = (long long)n * h * w_;
  hipLaunchKernelGGL(latent_in_kernel, dim3(grid_for(pixels)), dim3(256), 0, (hipStream_t)stream, z, w, b, inv_scale, out, pixels,
                     h * w_, zc, e);
  return adm_check_launch("adm_vae_latent_in");
}

extern "C" int adm_vae_image_out(const float* x, float* unit, uint8_t* u8, int n, int h, int w, void* stream) {
  ADM_REQUIRE(x, ADM_E_ARG, "adm_vae_image_out: null pointer");
  ADM_REQUIRE(unit || u8, ADM_E_ARG, "adm_vae_image_out: null outputs (at least one of unit / u8 is needed)");
  ADM_REQUIRE(n > 0 && h > 0 && w > 0, ADM_E_ARG, "adm_vae_image_out: bad shape n=%d h=%d w=%d", n, h, w);
  const long long pixels = (long long)n * h * w;
  hipLaunchKernelGGL(image_out_kernel, dim3(grid_for(pixels)), dim3(256), 0, (hipStream_t)stream, x, unit, u8, pixels, h * w);
  return adm_check_launch("adm_vae_image_out");
}
