// The f64 Gram tile and the reduction tree that the pair-sum kernels share: K16 (adm_kid.hip, cubic polynomial kernel) and K18
// (adm_cmmd.hip, Gaussian RBF kernel) both sum a function of  G[i][j] = x_i . y_j  over all pairs, or over the pairs i != j of one set.
//
// One f64 GEMM on v_mfma_f64_16x16x4_f64 (fp32 rows widened to f64: every product is exact, the accumulation is f64 -- the operand
// and C/D maps are those of gram_mfma_kernel, adm_fid.hip) with the kernel function and the sum in the caller's epilogue: the n x m
// matrix never exists in memory (0.1 .. 2.5 G entries at a 10 000 .. 50 000-row reference set).
//   * block = one 64 x 64 tile of G, 4 waves of 32 x 32 (2 x 2 MFMA tiles); the feature axis is staged 64 wide through LDS
//     (pitch 68 floats: 16-byte aligned rows, 17 16-byte units apart, so the 16 rows x 4 segments of a ds_read_b128 spread
//     over the banks), the next chunk's global loads in flight under the MFMAs.  A lane reads 4 consecutive features at once
//     and feeds element e to MFMA e: MFMA e of a 16-feature group sums features 16 g + 4 kq + e -- a fixed permutation of
//     the summation order, the same for both operands.
//   * a lane's 4 results of MFMA tile (ti, tj) are rows (2 wi + ti) 16 + kq + 4 q, column (2 wj + tj) 16 + c (the f64 C/D map),
//     wi = wave >> 1, wj = wave & 1, kq = lane >> 4, c = lane & 15.  The caller's epilogue masks BY INDEX: a zero-filled row past
//     n or m does not give a kernel value of 0; in self mode i == j is skipped inside diagonal tiles.  It owns the order of the
//     lane's 16 additions.
//   * pair_block_sum: wave sum (6 xor shuffles), block sum (4 waves through LDS, in wave order), one partial per block into
//     work[block].  Self mode computes the tiles on and above the diagonal only; a tile above it counts twice (the partial
//     times 2: exact).
//   * pair_final_kernel, a single block, adds the partials: thread t adds work[t], work[t + 256], ... in index order, then a
//     fixed 8-level tree.  No floating-point atomics anywhere: two calls on the same inputs are bitwise equal.
// Longest chain of additions behind out[0]: 16 + 6 + 3 + ceil(blocks / 256) + 8 (mmd.reduction_chain restates it).
// Algorithmic work: 2 n m d FLOP (self mode: n (n + 64) d), all on the f64 matrix pipe.
#pragma once
#include "adm_common.h"

constexpr int PT = 64;         // tile edge (rows of x and rows of y per block)
constexpr int PK = 64;         // features staged per step
constexpr int PP = PK + 4;     // LDS row pitch in floats
typedef double f64x4 __attribute__((ext_vector_type(4)));

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

// block -> tile: row-major over the rectangle, or over the rows of the upper triangle (row bi holds tiles_j - bi tiles)
struct PairTile {
  int bi, bj;
  long long i0, j0;     // first row of x, first row of y
};

__device__ __forceinline__ PairTile pair_tile_of_block(int tiles_j, int self_pairs) {
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
  return PairTile{bi, bj, (long long)bi * PT, (long long)bj * PT};
}

// acc = the block's 64 x 64 tile of G at (i0, j0), this lane's 2 x 2 x 4 entries of it
__device__ __forceinline__ void pair_gram_tile(f64x4 (&acc)[2][2], const float* __restrict__ x, long long n,
                                               const float* __restrict__ y, long long m, int d, long long i0, long long j0) {
  __shared__ __attribute__((aligned(16))) float Xs[PT * PP];
  __shared__ __attribute__((aligned(16))) float Ys[PT * PP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1, kq = lane >> 4, c = lane & 15;
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
}

// the lane sums s of a block -> work[block], times 2 (exact) where `twice`
__device__ __forceinline__ void pair_block_sum(double s, double* __restrict__ work, bool twice) {
  __shared__ double wsum[4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double tot = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    work[blockIdx.x] = twice ? 2.0 * tot : tot;
  }
}

static __global__ void __launch_bounds__(256)
pair_final_kernel(const double* __restrict__ work, long long blocks, double* __restrict__ out) {
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

constexpr long long PAIR_MAX_ROWS = 1LL << 30;        // tile counts and the triangle's block count stay far inside int64
constexpr long long PAIR_MAX_BLOCKS = 0x7fffffffLL;   // one grid dimension

// blocks of the tile pass (= partials in work), or -1 for a shape it does not take
static inline long long pair_blocks(long long n, long long m, int self_pairs) {
  if (n < 1 || m < 1 || n > PAIR_MAX_ROWS || m > PAIR_MAX_ROWS || (self_pairs && m != n)) return -1;
  const long long ti = (n + PT - 1) / PT, tj = (m + PT - 1) / PT;
  const long long b = self_pairs ? ti * (ti + 1) / 2 : ti * tj;
  return b <= PAIR_MAX_BLOCKS ? b : -1;
}

// The argument checks of adm_<stem>_sums; work holds the per-block partials and `row_doubles` doubles per row of x and of y.
// 0 and *blocks, or the error code with the text set.
static inline int pair_check_args(const char* stem, const float* x, long long n, const float* y, long long m, int d, const double* work,
                                  long long work_elems, int row_doubles, const double* out, int self_pairs, long long* blocks) {
  ADM_REQUIRE(self_pairs == 0 || self_pairs == 1, ADM_E_ARG, "adm_%s_sums: self_pairs=%d is neither 0 nor 1", stem, self_pairs);
  ADM_REQUIRE(x && work && out && (y || self_pairs), ADM_E_ARG, "adm_%s_sums: null pointer", stem);
  ADM_REQUIRE(n >= 1 && m >= 1, ADM_E_ARG, "adm_%s_sums: need n >= 1 and m >= 1 (n=%lld m=%lld)", stem, n, m);
  ADM_REQUIRE(!self_pairs || ((y == nullptr || y == x) && m == n), ADM_E_ARG,
              "adm_%s_sums: self_pairs needs y == x (or NULL) and m == n (n=%lld m=%lld)", stem, n, m);
  ADM_REQUIRE(d >= 4 && d % 4 == 0, ADM_E_SHAPE, "adm_%s_sums: d=%d must be a positive multiple of 4", stem, d);
  *blocks = pair_blocks(n, m, self_pairs);
  ADM_REQUIRE(*blocks > 0, ADM_E_SHAPE, "adm_%s_sums: n=%lld m=%lld too large for the grid", stem, n, m);
  const long long need = *blocks + row_doubles * (n + m);
  ADM_REQUIRE(work_elems >= need, ADM_E_ARG, "adm_%s_sums: work holds %lld doubles, adm_%s_work_elems says %lld", stem, work_elems, stem,
              need);
  ADM_REQUIRE(adm_aligned16(x) && (y == nullptr || adm_aligned16(y)), ADM_E_ALIGN, "adm_%s_sums: 16-byte aligned rows required", stem);
  ADM_REQUIRE((((uintptr_t)work) & 7u) == 0 && (((uintptr_t)out) & 7u) == 0, ADM_E_ALIGN, "adm_%s_sums: 8-byte aligned work / out required",
              stem);
  return 0;
}
