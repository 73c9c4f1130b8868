// K18: the Gaussian RBF kernel sums of CMMD (Jayasumana et al., "Rethinking FID", CVPR 2024; project-defined: the reference has no
// CMMD) on CLIP image embeddings, normalised in f64 inside the kernel.
//
//   r_i = |x_i|^2   s_j = |y_j|^2   G_ij = x_i . y_j   c_ij = G_ij / sqrt(r_i s_j)   D_ij = max(2 - 2 c_ij, 0)
//   kappa_ij = expm1(-gamma D_ij) = k_ij - 1 <= 0        S_xy = sum_i sum_j kappa_ij        S_xx = sum_{i != j} kappa_ij
//
// On unit vectors with gamma = 1 / 200 every k lies in [exp(-0.02), 1] and MMD^2 is 1e-4 .. 1e-3: the sums are of k - 1, so the
// ones of the three means cancel algebraically (cmmd.py) and not in the last digits of a sum of n m values near 1.
//   * pass 0, norm_kernel: one wave per row of x, then of y; a lane adds the squares (fp32 widened: exact) of its float4s at
//     features 256 t + 4 lane in order, then 6 xor shuffles.  r and s go to work[blocks ..] as f64.
//   * pass 1, rbf_tile_kernel: the 64 x 64 tile loop of poly3_tile_kernel (adm_kid.hip; same staging, same operand and C/D maps
//     of v_mfma_f64_16x16x4_f64) with the epilogue above: a true f64 sqrt and division, then expm1.  Masked BY INDEX: a
//     zero-filled row past n or m has norm 0 and gives 0 / 0 = NaN, not 0.  Lane, wave, block sums and the doubling of a tile above
//     the diagonal as in K16; one partial per block into work[block].
//   * pass 2, rbf_final_kernel: thread t adds work[t], work[t + 256], ... in index order, then a fixed 8-level tree.
// No floating-point atomics: two calls on the same inputs are bitwise equal.  Longest chain of additions behind out[0]:
// 16 + 6 + 3 + ceil(blocks / 256) + 8 (cmmd.reduction_chain); behind a norm: 4 ceil(d / 256) + 6 (cmmd.norm_chain).
// A row of norm 0 (or one whose r_i s_j overflows f64) makes out[0] NaN; cmmd.py refuses such rows from the norms in work.
#include "adm_common.h"

namespace {

constexpr int PT = 64;         // tile edge (rows of x and rows of y per block)
constexpr int PK = 64;         // features staged per step
constexpr int PP = PK + 4;     // LDS row pitch in floats
typedef double f64x4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256)
norm_kernel(const float* __restrict__ x, long long n, const float* __restrict__ y, long long m, int d, double* __restrict__ norms) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);     // wave-uniform
  if (row >= n + m) return;
  const float* __restrict__ p = row < n ? x + row * d : y + (row - n) * d;
  double s = 0.0;
  for (int k = 4 * lane; k < d; k += 256) {
    const float4 v = *reinterpret_cast<const float4*>(p + k);
    const double a = (double)v.x, b = (double)v.y, c = (double)v.z, e = (double)v.w;
    s += a * a;
    s += b * b;
    s += c * c;
    s += e * e;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) norms[row] = s;
}

// global -> registers of the 64 x 64 chunk of each operand: 256 threads x 4 x 16 B each; rows past the set and features past d
// (d % 4 == 0: a float4 is inside or outside as a whole) read as zero
struct Stage {
  float4 x[4], y[4];
};

__device__ __forceinline__ void load_stage(Stage& s, const float* __restrict__ x, long long n, long long r0,
                                           const float* __restrict__ y, long long m, long long c0, int d, int k0, int tid) {
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int e = tid + 256 * v, row = e >> 4, seg = (e & 15) * 4;
    s.x[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    s.y[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k0 + seg < d) {
      if (r0 + row < n) s.x[v] = *reinterpret_cast<const float4*>(x + (r0 + row) * d + k0 + seg);
      if (c0 + row < m) s.y[v] = *reinterpret_cast<const float4*>(y + (c0 + row) * d + k0 + seg);
    }
  }
}

__device__ __forceinline__ void store_stage(const Stage& s, float* Xs, float* Ys, int tid) {
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int e = tid + 256 * v, row = e >> 4, seg = (e & 15) * 4;
    *reinterpret_cast<float4*>(Xs + row * PP + seg) = s.x[v];
    *reinterpret_cast<float4*>(Ys + row * PP + seg) = s.y[v];
  }
}

__global__ void __launch_bounds__(256)
rbf_tile_kernel(const float* __restrict__ x, long long n, const float* __restrict__ y, long long m, int d, double gamma,
                double* __restrict__ work, const double* __restrict__ rn, const double* __restrict__ sn, int tiles_j, int self_pairs) {
  __shared__ __attribute__((aligned(16))) float Xs[PT * PP];
  __shared__ __attribute__((aligned(16))) float Ys[PT * PP];
  __shared__ double wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1, kq = lane >> 4, c = lane & 15;
  // block -> tile: row-major over the rectangle, or over the rows of the upper triangle (row bi holds tiles_j - bi tiles)
  int bi, bj;
  if (self_pairs) {
    int rem = (int)blockIdx.x;
    bi = 0;
    while (rem >= tiles_j - bi) {
      rem -= tiles_j - bi;
      ++bi;
    }
    bj = bi + rem;
  } else {
    bi = (int)(blockIdx.x / (unsigned)tiles_j);
    bj = (int)(blockIdx.x % (unsigned)tiles_j);
  }
  const long long i0 = (long long)bi * PT, j0 = (long long)bj * PT;

  f64x4 acc[2][2];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) acc[ti][tj] = f64x4{0.0, 0.0, 0.0, 0.0};

  const int nch = (d + PK - 1) / PK;
  Stage st;
  load_stage(st, x, n, i0, y, m, j0, d, 0, tid);
  for (int ch = 0; ch < nch; ++ch) {
    store_stage(st, Xs, Ys, tid);
    __syncthreads();
    if (ch + 1 < nch) load_stage(st, x, n, i0, y, m, j0, d, (ch + 1) * PK, tid);
    const int left = d - ch * PK;                                   // features left from this chunk on
    const int groups = left >= PK ? PK / 16 : (left + 15) / 16;     // 16-feature groups with anything in them (block-uniform)
#pragma unroll
    for (int g = 0; g < PK / 16; ++g) {
      if (g < groups) {
        float4 a[2], b[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          a[t] = *reinterpret_cast<const float4*>(Xs + ((2 * wi + t) * 16 + c) * PP + g * 16 + 4 * kq);
          b[t] = *reinterpret_cast<const float4*>(Ys + ((2 * wj + t) * 16 + c) * PP + g * 16 + 4 * kq);
        }
        const float ae[2][4] = {{a[0].x, a[0].y, a[0].z, a[0].w}, {a[1].x, a[1].y, a[1].z, a[1].w}};
        const float be[2][4] = {{b[0].x, b[0].y, b[0].z, b[0].w}, {b[1].x, b[1].y, b[1].z, b[1].w}};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const double af[2] = {(double)ae[0][e], (double)ae[1][e]}, bf[2] = {(double)be[0][e], (double)be[1][e]};
#pragma unroll
          for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
              acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[ti], bf[tj], acc[ti][tj], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  // epilogue: a lane's 4 results of an MFMA tile are rows kq + 4 q, column c (the f64 C/D map).  A row or column past the set
  // takes norm 1 (its Gram entries are 0, so its value is finite) and is masked below by index.
  const bool diag = self_pairs && bi == bj;
  double sj[2];
#pragma unroll
  for (int tj = 0; tj < 2; ++tj) {
    const long long j = j0 + (2 * wj + tj) * 16 + c;
    sj[tj] = j < m ? sn[j] : 1.0;
  }
  double s = 0.0;
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const long long i = i0 + (2 * wi + ti) * 16 + kq + 4 * q;
      const double ri = i < n ? rn[i] : 1.0;
#pragma unroll
      for (int tj = 0; tj < 2; ++tj) {
        const long long j = j0 + (2 * wj + tj) * 16 + c;
        const double cs = acc[ti][tj][q] / sqrt(ri * sj[tj]);
        const double dist = fmax(2.0 - 2.0 * cs, 0.0);
        const double kap = expm1(-gamma * dist);
        const bool live = i < n && j < m && !(diag && i == j);
        s += live ? kap : 0.0;
      }
    }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) wsum[wave] = s;
  __syncthreads();
  if (tid == 0) {
    const double tot = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    work[blockIdx.x] = (self_pairs && bi != bj) ? 2.0 * tot : tot;
  }
}

__global__ void __launch_bounds__(256)
rbf_final_kernel(const double* __restrict__ work, long long blocks, double* __restrict__ out) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (long long i = tid; i < blocks; i += 256) s += work[i];
  red[tid] = s;
  __syncthreads();
#pragma unroll
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  if (tid == 0) out[0] = red[0];
}

constexpr long long RBF_MAX_ROWS = 1LL << 30;        // tile counts and the triangle's block count stay far inside int64
constexpr long long RBF_MAX_BLOCKS = 0x7fffffffLL;   // one grid dimension

long long rbf_blocks(long long n, long long m, int self_pairs) {
  if (n < 1 || m < 1 || n > RBF_MAX_ROWS || m > RBF_MAX_ROWS || (self_pairs && m != n)) return -1;
  const long long ti = (n + PT - 1) / PT, tj = (m + PT - 1) / PT;
  const long long b = self_pairs ? ti * (ti + 1) / 2 : ti * tj;
  return b <= RBF_MAX_BLOCKS ? b : -1;
}

}  // namespace

extern "C" int64_t adm_rbf_work_elems(int64_t n, int64_t m, int self_pairs) {
  const long long b = rbf_blocks(n, m, self_pairs != 0);
  if (b < 0) {
    adm_set_error("adm_rbf_work_elems: unsupported shape n=%lld m=%lld self_pairs=%d", (long long)n, (long long)m, self_pairs);
    return -1;
  }
  return b + n + m;
}

extern "C" int adm_rbf_sums(const float* x, int64_t n, const float* y, int64_t m, int d, double gamma, double* work,
                            int64_t work_elems, double* out, void* stream, int self_pairs) {
  ADM_REQUIRE(self_pairs == 0 || self_pairs == 1, ADM_E_ARG, "adm_rbf_sums: self_pairs=%d is neither 0 nor 1", self_pairs);
  ADM_REQUIRE(x && work && out && (y || self_pairs), ADM_E_ARG, "adm_rbf_sums: null pointer");
  ADM_REQUIRE(n >= 1 && m >= 1, ADM_E_ARG, "adm_rbf_sums: need n >= 1 and m >= 1 (n=%lld m=%lld)", (long long)n, (long long)m);
  ADM_REQUIRE(!self_pairs || ((y == nullptr || y == x) && m == n), ADM_E_ARG,
              "adm_rbf_sums: self_pairs needs y == x (or NULL) and m == n (n=%lld m=%lld)", (long long)n, (long long)m);
  ADM_REQUIRE(d >= 4 && d % 4 == 0, ADM_E_SHAPE, "adm_rbf_sums: d=%d must be a positive multiple of 4", d);
  ADM_REQUIRE(gamma > 0.0 && gamma <= 1.7976931348623157e308, ADM_E_ARG, "adm_rbf_sums: gamma=%g must be finite and positive", gamma);
  const long long blocks = rbf_blocks(n, m, self_pairs);
  ADM_REQUIRE(blocks > 0, ADM_E_SHAPE, "adm_rbf_sums: n=%lld m=%lld too large for the grid", (long long)n, (long long)m);
  ADM_REQUIRE(work_elems >= blocks + n + m, ADM_E_ARG, "adm_rbf_sums: work holds %lld doubles, adm_rbf_work_elems says %lld",
              (long long)work_elems, blocks + (long long)n + (long long)m);
  ADM_REQUIRE(adm_aligned16(x) && (y == nullptr || adm_aligned16(y)), ADM_E_ALIGN, "adm_rbf_sums: 16-byte aligned rows required");
  ADM_REQUIRE((((uintptr_t)work) & 7u) == 0 && (((uintptr_t)out) & 7u) == 0, ADM_E_ALIGN, "adm_rbf_sums: 8-byte aligned work / out required");
  hipStream_t s = (hipStream_t)stream;
  const int tiles_j = (int)((m + PT - 1) / PT);
  const float* yy = y ? y : x;
  double* rn = work + blocks;
  double* sn = rn + n;
  hipLaunchKernelGGL(norm_kernel, dim3((unsigned)((n + m + 3) / 4)), dim3(256), 0, s, x, (long long)n, yy, (long long)m, d, rn);
  hipLaunchKernelGGL(rbf_tile_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, (long long)n, yy, (long long)m, d, gamma, work,
                     (const double*)rn, (const double*)sn, tiles_j, self_pairs);
  hipLaunchKernelGGL(rbf_final_kernel, dim3(1), dim3(256), 0, s, (const double*)work, blocks, out);
  return adm_check_launch("adm_rbf_sums");
}
