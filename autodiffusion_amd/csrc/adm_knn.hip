// K13: k-nearest-neighbour radii and manifold membership of the ADM precision / recall (evaluations/evaluator.py
// ManifoldEstimator.manifold_radii :319-352, evaluate_pr :396-430, DistanceBlock :458-500).
//
// Both entry points are one fp16 GEMM  G[r][c] = x_r . p_c  (fp32 accumulation on v_mfma_f32_32x32x16_f16) with the
// reduction in its epilogue; the distance is  max(|p_c|^2 + |x_r|^2 - 2 G[r][c], 0)  as in _batch_pairwise_distances, and no
// distance matrix leaves the registers.  The "column" set p rides on the accumulator's lane (col = lane & 31), the "row" set
// x on its 16 registers, so every lane owns one column and sees 16 row distances per 32x32 tile:
//   * adm_knn_smallest: columns = queries; each lane keeps a register-sorted list of the KK smallest distances of its query,
//     the 4 lists of a query inside a block (2 lane halves x 2 row waves) are merged through LDS at the end, the row set is
//     split over `splits` blocks per query tile and a second kernel merges their partial lists;
//   * adm_knn_cover: columns = a, rows = b; a lane ORs (d <= rb[j][k]) over its rows into its column's flags, a ballot ORs
//     (d <= ra[i][k]) over the lanes into each row's flags; every writer stores the same 1, so no atomics.
// Every distance is computed by the same fixed K-loop wherever it lands (tile origins are multiples of 128 whatever the
// split), and the k smallest values of a multiset do not depend on insertion order: the outputs are bitwise independent of
// `splits` and of scheduling.
// Operands are _Float16 in both builds of the library (the reference casts the features to tf.float16, :447-450).
// Algorithmic work: 2 * n_rows * n_cols * d FLOP (+ the epilogue's 2..3 VALU ops per distance).
#include "adm_common.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int BT = 128;            // block tile: 128 rows x 128 columns, 4 waves of 64 x 64 (2 x 2 MFMA tiles each)
constexpr int KC = 64;             // d-chunk staged per step
constexpr int LROW = KC + 8;       // LDS row pitch in halves (144 B: breaks the 128-B bank period)
constexpr int KMAX = 8;            // longest list / most neighbourhood sizes

// global -> registers of one 128 x 64 half tile of each operand: 256 threads x 4 x 16 B each
struct Stage {
  uint4 r[4], p[4];
};

__device__ __forceinline__ void load_stage(Stage& s, const _Float16* __restrict__ x, int nx, int r0, const _Float16* __restrict__ p,
                                           int np, int c0, int d, int k0, int tid) {
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int e = tid + 256 * v, row = e >> 3, seg = (e & 7) * 8;
    s.r[v] = make_uint4(0, 0, 0, 0);
    s.p[v] = make_uint4(0, 0, 0, 0);
    if (r0 + row < nx) s.r[v] = *reinterpret_cast<const uint4*>(x + (long long)(r0 + row) * d + k0 + seg);
    if (c0 + row < np) s.p[v] = *reinterpret_cast<const uint4*>(p + (long long)(c0 + row) * d + k0 + seg);
  }
}

__device__ __forceinline__ void store_stage(const Stage& s, _Float16* Rs, _Float16* Ps, int tid) {
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int e = tid + 256 * v, row = e >> 3, seg = (e & 7) * 8;
    *reinterpret_cast<uint4*>(Rs + row * LROW + seg) = s.r[v];
    *reinterpret_cast<uint4*>(Ps + row * LROW + seg) = s.p[v];
  }
}

// acc[rt][ct] += R[wr*64 + rt*32 + ..][chunk] . P[wc*64 + ct*32 + ..][chunk]
__device__ __forceinline__ void mma_chunk(adm_f32x16 (&acc)[2][2], const _Float16* Rs, const _Float16* Ps, int wr, int wc, int lane) {
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int s = 0; s < KC / 16; ++s) {
    f16x8 a[2], b[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      a[t] = *reinterpret_cast<const f16x8*>(Rs + (wr * 64 + t * 32 + r) * LROW + s * 16 + 8 * h);
      b[t] = *reinterpret_cast<const f16x8*>(Ps + (wc * 64 + t * 32 + r) * LROW + s * 16 + 8 * h);
    }
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[rt], b[ct], acc[rt][ct], 0, 0, 0);
  }
}

// ascending register list: insert v (caller has checked v < L[KK - 1])
template <int KK>
__device__ __forceinline__ void list_insert(float (&L)[KK], float v) {
#pragma unroll
  for (int i = KK - 1; i > 0; --i) L[i] = v < L[i - 1] ? L[i - 1] : (v < L[i] ? v : L[i]);
  L[0] = v < L[0] ? v : L[0];
}

// row index of accumulator register q of lane half h inside a 32 x 32 tile
__device__ __forceinline__ int acc_row(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

template <int KK>
__global__ void __launch_bounds__(256)
knn_partial_kernel(const _Float16* __restrict__ q, const float* __restrict__ qn, int nq, const _Float16* __restrict__ x,
                   const float* __restrict__ xn, int nx, int d, int kk, float* __restrict__ out, int splits) {
  __shared__ __attribute__((aligned(16))) _Float16 smem[2 * BT * LROW];
  _Float16* Rs = smem;
  _Float16* Ps = smem + BT * LROW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1, h = lane >> 5;
  const int c0 = blockIdx.x * BT, split = blockIdx.y;
  const int rtiles = (nx + BT - 1) / BT;
  const int t_lo = (int)((long long)rtiles * split / splits), t_hi = (int)((long long)rtiles * (split + 1) / splits);
  const int nch = d / KC, iters = (t_hi - t_lo) * nch;

  float L[2][KK];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int i = 0; i < KK; ++i) L[ct][i] = __builtin_inff();
  float qnorm[2];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int c = c0 + wc * 64 + ct * 32 + (lane & 31);
    qnorm[ct] = c < nq ? qn[c] : 0.f;
  }

  adm_f32x16 acc[2][2];
  Stage st;
  if (iters > 0) load_stage(st, x, nx, t_lo * BT, q, nq, c0, d, 0, tid);
  for (int it = 0; it < iters; ++it) {
    const int tile = t_lo + it / nch, ch = it % nch, r0 = tile * BT;
    if (ch == 0) {
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = adm_f32x16{};
    }
    store_stage(st, Rs, Ps, tid);
    __syncthreads();
    if (it + 1 < iters) {
      const int nt = t_lo + (it + 1) / nch;
      load_stage(st, x, nx, nt * BT, q, nq, c0, d, ((it + 1) % nch) * KC, tid);
    }
    mma_chunk(acc, Rs, Ps, wr, wc, lane);
    __syncthreads();
    if (ch == nch - 1) {
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int qq = 0; qq < 16; ++qq) {
          const int j = r0 + wr * 64 + rt * 32 + acc_row(qq, h);
          const float jn = j < nx ? xn[j] : __builtin_inff();   // out-of-range rows: +inf never enters a list
#pragma unroll
          for (int ct = 0; ct < 2; ++ct) {
            const float dist = fmaxf((qnorm[ct] + jn) - 2.0f * acc[rt][ct][qq], 0.0f);
            if (dist < L[ct][KK - 1]) list_insert<KK>(L[ct], dist);
          }
        }
    }
  }

  // merge the 4 lists of every column (2 row waves x 2 lane halves) through LDS: [128 columns][4][KK]
  float* M = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int col = wc * 64 + ct * 32 + (lane & 31), src = wr * 2 + h;
#pragma unroll
    for (int i = 0; i < KK; ++i) M[(col * 4 + src) * KK + i] = L[ct][i];
  }
  __syncthreads();
  if (tid < BT && c0 + tid < nq) {
    float R[KK];
#pragma unroll
    for (int i = 0; i < KK; ++i) R[i] = __builtin_inff();
    for (int e = 0; e < 4 * KK; ++e) {
      const float v = M[tid * 4 * KK + e];
      if (v < R[KK - 1]) list_insert<KK>(R, v);
    }
    float* o = out + ((long long)split * nq + c0 + tid) * kk;
#pragma unroll
    for (int i = 0; i < KK; ++i)
      if (i < kk) o[i] = R[i];
  }
}

// out[c][0..kk) = the kk smallest of the splits partial lists ws[s][c][0..kk)
template <int KK>
__global__ void __launch_bounds__(256)
knn_merge_kernel(const float* __restrict__ ws, int nq, int kk, int splits, float* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= nq) return;
  float R[KK];
#pragma unroll
  for (int i = 0; i < KK; ++i) R[i] = __builtin_inff();
  for (int s = 0; s < splits; ++s)
    for (int i = 0; i < kk; ++i) {
      const float v = ws[((long long)s * nq + c) * kk + i];
      if (v < R[KK - 1]) list_insert<KK>(R, v);
    }
#pragma unroll
  for (int i = 0; i < KK; ++i)
    if (i < kk) out[(long long)c * kk + i] = R[i];
}

// columns = a (ra, a_in), rows = b (rb, b_in); one 128 x 128 tile per block
__global__ void __launch_bounds__(256)
knn_cover_kernel(const _Float16* __restrict__ a, const float* __restrict__ an, const float* __restrict__ ra, int na,
                 const _Float16* __restrict__ b, const float* __restrict__ bn, const float* __restrict__ rb, int nb, int d, int K,
                 uint8_t* __restrict__ a_in, uint8_t* __restrict__ b_in) {
  __shared__ __attribute__((aligned(16))) _Float16 smem[2 * BT * LROW];
  _Float16* Rs = smem;
  _Float16* Ps = smem + BT * LROW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1, h = lane >> 5;
  const int c0 = blockIdx.x * BT, r0 = blockIdx.y * BT, nch = d / KC;

  adm_f32x16 acc[2][2];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = adm_f32x16{};
  Stage st;
  load_stage(st, b, nb, r0, a, na, c0, d, 0, tid);
  for (int ch = 0; ch < nch; ++ch) {
    store_stage(st, Rs, Ps, tid);
    __syncthreads();
    if (ch + 1 < nch) load_stage(st, b, nb, r0, a, na, c0, d, (ch + 1) * KC, tid);
    mma_chunk(acc, Rs, Ps, wr, wc, lane);
    __syncthreads();
  }

  int ci[2];
  float cn[2];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    ci[ct] = c0 + wc * 64 + ct * 32 + (lane & 31);
    cn[ct] = ci[ct] < na ? an[ci[ct]] : 0.f;
  }
  for (int k = 0; k < K; ++k) {
    float rc[2];                          // out-of-range columns / rows: radius -inf never covers
    bool ahit[2] = {false, false};
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) rc[ct] = ci[ct] < na ? ra[(long long)ci[ct] * K + k] : -__builtin_inff();
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int qq = 0; qq < 16; ++qq) {
        const int j = r0 + wr * 64 + rt * 32 + acc_row(qq, h);
        const bool jv = j < nb;
        const float jn = jv ? bn[j] : 0.f;
        const float rj = jv ? rb[(long long)j * K + k] : -__builtin_inff();
        bool bh = false;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          const float dist = fmaxf((cn[ct] + jn) - 2.0f * acc[rt][ct][qq], 0.0f);
          ahit[ct] |= dist <= rj;
          bh |= jv && dist <= rc[ct];
        }
        const unsigned long long m = __ballot(bh);
        const unsigned half = h ? (unsigned)(m >> 32) : (unsigned)m;
        if (half && (lane & 31) == 0) b_in[(long long)j * K + k] = 1;
      }
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
      if (ahit[ct] && ci[ct] < na) a_in[(long long)ci[ct] * K + k] = 1;
  }
}

template <int KK>
int launch_smallest(const void* q, int nq, const float* qn, const void* x, int nx, const float* xn, int d, int kk, float* out,
                    float* ws, int splits, hipStream_t s) {
  float* part = splits == 1 ? out : ws;
  hipLaunchKernelGGL(knn_partial_kernel<KK>, dim3((nq + BT - 1) / BT, splits), dim3(256), 0, s, (const _Float16*)q, qn, nq,
                     (const _Float16*)x, xn, nx, d, kk, part, splits);
  if (splits > 1) hipLaunchKernelGGL(knn_merge_kernel<KK>, dim3((nq + 255) / 256), dim3(256), 0, s, ws, nq, kk, splits, out);
  return adm_check_launch("adm_knn_smallest");
}

}  // namespace

extern "C" int adm_knn_smallest(const void* q, int nq, const float* qnorm, const void* x, int nx, const float* xnorm, int d, int kk,
                                float* out, float* ws, int splits, void* stream) {
  ADM_REQUIRE(q && qnorm && x && xnorm && out, ADM_E_ARG, "adm_knn_smallest: null pointer");
  ADM_REQUIRE(kk >= 1 && kk <= KMAX, ADM_E_ARG, "adm_knn_smallest: kk=%d outside [1, %d]", kk, KMAX);
  ADM_REQUIRE(nq > 0 && nx >= kk, ADM_E_ARG, "adm_knn_smallest: need nq > 0 and nx >= kk (nq=%d nx=%d kk=%d)", nq, nx, kk);
  ADM_REQUIRE(d > 0 && d % KC == 0, ADM_E_SHAPE, "adm_knn_smallest: d=%d must be a positive multiple of %d", d, KC);
  const int rtiles = (nx + BT - 1) / BT;
  ADM_REQUIRE(splits >= 1 && splits <= rtiles, ADM_E_ARG, "adm_knn_smallest: splits=%d outside [1, %d]", splits, rtiles);
  ADM_REQUIRE(splits == 1 || ws, ADM_E_ARG, "adm_knn_smallest: splits > 1 needs the workspace [splits][nq][kk]");
  ADM_REQUIRE(adm_aligned16(q) && adm_aligned16(x), ADM_E_ALIGN, "adm_knn_smallest: 16-byte aligned features required");
  hipStream_t s = (hipStream_t)stream;
  return kk <= 4 ? launch_smallest<4>(q, nq, qnorm, x, nx, xnorm, d, kk, out, ws, splits, s)
                 : launch_smallest<8>(q, nq, qnorm, x, nx, xnorm, d, kk, out, ws, splits, s);
}

extern "C" int adm_knn_cover(const void* a, int na, const float* anorm, const float* ra, const void* b, int nb, const float* bnorm,
                             const float* rb, int d, int K, uint8_t* a_in, uint8_t* b_in, void* stream) {
  ADM_REQUIRE(a && anorm && ra && b && bnorm && rb && a_in && b_in, ADM_E_ARG, "adm_knn_cover: null pointer");
  ADM_REQUIRE(K >= 1 && K <= KMAX, ADM_E_ARG, "adm_knn_cover: K=%d outside [1, %d]", K, KMAX);
  ADM_REQUIRE(na > 0 && nb > 0, ADM_E_ARG, "adm_knn_cover: need na > 0 and nb > 0 (na=%d nb=%d)", na, nb);
  ADM_REQUIRE(d > 0 && d % KC == 0, ADM_E_SHAPE, "adm_knn_cover: d=%d must be a positive multiple of %d", d, KC);
  ADM_REQUIRE(adm_aligned16(a) && adm_aligned16(b), ADM_E_ALIGN, "adm_knn_cover: 16-byte aligned features required");
  ADM_REQUIRE((nb + BT - 1) / BT <= 65535, ADM_E_SHAPE, "adm_knn_cover: nb=%d too large for the grid", nb);
  hipLaunchKernelGGL(knn_cover_kernel, dim3((na + BT - 1) / BT, (nb + BT - 1) / BT), dim3(256), 0, (hipStream_t)stream,
                     (const _Float16*)a, anorm, ra, na, (const _Float16*)b, bnorm, rb, nb, d, K, a_in, b_in);
  return adm_check_launch("adm_knn_cover");
}
