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
//   * pass 1, rbf_tile_kernel: the 64 x 64 f64 Gram tile of adm_pairsum.h (shared with K16, adm_kid.hip; staging, operand and C/D
//     maps and the reductions are described there) with the epilogue above: a true f64 sqrt and division, then expm1.  Masked BY
//     INDEX: a zero-filled row past n or m has norm 0 and gives 0 / 0 = NaN, not 0.  Lane sum: 16 values in the order ti, q, tj
//     (the row norm is hoisted); one partial per block into work[block].
//   * pass 2, pair_final_kernel (adm_pairsum.h) adds the partials.
// No floating-point atomics: two calls on the same inputs are bitwise equal.  Longest chain of additions behind out[0]:
// 16 + 6 + 3 + ceil(blocks / 256) + 8 (cmmd.reduction_chain); behind a norm: 4 ceil(d / 256) + 6 (cmmd.norm_chain).
// A row of norm 0 (or one whose r_i s_j overflows f64) makes out[0] NaN; cmmd.py refuses such rows from the norms in work.
#include "adm_pairsum.h"

namespace {

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

__global__ void __launch_bounds__(256)
rbf_tile_kernel(const float* __restrict__ x, long long n, const float* __restrict__ y, long long m, int d, double gamma,
                double* __restrict__ work, const double* __restrict__ rn, const double* __restrict__ sn, int tiles_j, int self_pairs) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1, kq = lane >> 4, c = lane & 15;
  const PairTile tile = pair_tile_of_block(tiles_j, self_pairs);
  const long long i0 = tile.i0, j0 = tile.j0;
  f64x4 acc[2][2];
  pair_gram_tile(acc, x, n, y, m, d, i0, j0);

  // epilogue: a lane's 4 results of an MFMA tile are rows kq + 4 q, column c (the f64 C/D map).  A row or column past the set
  // takes norm 1 (its Gram entries are 0, so its value is finite) and is masked below by index.
  const bool diag = self_pairs && tile.bi == tile.bj;
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
  pair_block_sum(s, work, self_pairs && tile.bi != tile.bj);
}

}  // namespace

extern "C" int64_t adm_rbf_work_elems(int64_t n, int64_t m, int self_pairs) {
  const long long b = pair_blocks(n, m, self_pairs != 0);
  if (b < 0) {
    adm_set_error("adm_rbf_work_elems: unsupported shape n=%lld m=%lld self_pairs=%d", (long long)n, (long long)m, self_pairs);
    return -1;
  }
  return b + n + m;
}

extern "C" int adm_rbf_sums(const float* x, int64_t n, const float* y, int64_t m, int d, double gamma, double* work,
                            int64_t work_elems, double* out, void* stream, int self_pairs) {
  long long blocks;
  const int rc = pair_check_args("rbf", x, n, y, m, d, work, work_elems, 1, out, self_pairs, &blocks);
  if (rc) return rc;
  ADM_REQUIRE(gamma > 0.0 && gamma <= 1.7976931348623157e308, ADM_E_ARG, "adm_rbf_sums: gamma=%g must be finite and positive", gamma);
  hipStream_t s = (hipStream_t)stream;
  const int tiles_j = (int)((m + PT - 1) / PT);
  const float* yy = y ? y : x;
  double* rn = work + blocks;
  double* sn = rn + n;
  hipLaunchKernelGGL(norm_kernel, dim3((unsigned)((n + m + 3) / 4)), dim3(256), 0, s, x, (long long)n, yy, (long long)m, d, rn);
  hipLaunchKernelGGL(rbf_tile_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, (long long)n, yy, (long long)m, d, gamma, work,
                     (const double*)rn, (const double*)sn, tiles_j, self_pairs);
  hipLaunchKernelGGL(pair_final_kernel, dim3(1), dim3(256), 0, s, (const double*)work, blocks, out);
  return adm_check_launch("adm_rbf_sums");
}
