// K16: the cubic polynomial kernel sums of the Kernel Inception Distance (Binkowski et al. 2018; project-defined: the
// reference has no KID).
//
//   k(a, b) = (a . b / d + 1)^3        S_xy = sum_i sum_j k(x_i, y_j)        S_xx = sum_{i != j} k(x_i, x_j)
//
// The f64 Gram  G[i][j] = x_i . y_j,  its 64 x 64 tile loop, the block and final reductions and the workspace are adm_pairsum.h's
// (shared with K18, adm_cmmd.hip; the tile, the masking rule and the reduction chain are described there).  This file adds
//   * the epilogue: t = G / d + 1 (a true f64 division), t * t * t, masked BY INDEX: a zero-filled row past n or m would add
//     k = (0 + 1)^3 = 1, not 0; in self mode i == j is skipped inside diagonal tiles.  Lane sum: 16 values in the order ti, tj, q.
// Longest chain of additions behind out[0]: 16 + 6 + 3 + ceil(blocks / 256) + 8 (kid.reduction_chain restates it).
#include "adm_pairsum.h"

namespace {

__global__ void __launch_bounds__(256)
poly3_tile_kernel(const float* __restrict__ x, long long n, const float* __restrict__ y, long long m, int d,
                  double* __restrict__ work, int tiles_j, int self_pairs) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1, kq = lane >> 4, c = lane & 15;
  const PairTile tile = pair_tile_of_block(tiles_j, self_pairs);
  const long long i0 = tile.i0, j0 = tile.j0;
  f64x4 acc[2][2];
  pair_gram_tile(acc, x, n, y, m, d, i0, j0);

  // epilogue: a lane's 4 results of an MFMA tile are rows kq + 4 q, column c (the f64 C/D map)
  const double dd = (double)d;
  const bool diag = self_pairs && tile.bi == tile.bj;
  double s = 0.0;
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const long long i = i0 + (2 * wi + ti) * 16 + kq + 4 * q, j = j0 + (2 * wj + tj) * 16 + c;
        const double t = acc[ti][tj][q] / dd + 1.0;
        const double k3 = (t * t) * t;
        const bool live = i < n && j < m && !(diag && i == j);
        s += live ? k3 : 0.0;
      }
  pair_block_sum(s, work, self_pairs && tile.bi != tile.bj);
}

}  // namespace

extern "C" int64_t adm_poly3_work_elems(int64_t n, int64_t m, int self_pairs) {
  const long long b = pair_blocks(n, m, self_pairs != 0);
  if (b < 0) adm_set_error("adm_poly3_work_elems: unsupported shape n=%lld m=%lld self_pairs=%d", (long long)n, (long long)m, self_pairs);
  return b;
}

extern "C" int adm_poly3_sums(const float* x, int64_t n, const float* y, int64_t m, int d, double* work, int64_t work_elems,
                              double* out, void* stream, int self_pairs) {
  long long blocks;
  const int rc = pair_check_args("poly3", x, n, y, m, d, work, work_elems, 0, out, self_pairs, &blocks);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int tiles_j = (int)((m + PT - 1) / PT);
  hipLaunchKernelGGL(poly3_tile_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, (long long)n, y ? y : x, (long long)m, d, work,
                     tiles_j, self_pairs);
  hipLaunchKernelGGL(pair_final_kernel, dim3(1), dim3(256), 0, s, (const double*)work, blocks, out);
  return adm_check_launch("adm_poly3_sums");
}
