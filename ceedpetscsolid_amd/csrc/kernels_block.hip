// kernels_block.hip -- operations on a BLOCK of vectors: k columns of length n in one array, column j at element j * ld (ld >= n,
// column-major, f64).  The Gram matrix of two column ranges and the combination of a column range with a small dense matrix: what the
// Rayleigh-Ritz step of a block eigensolver (modal.py) does to [W | X | P] once per iteration.  Both stream over the rows, grid-stride:
// every column of a row chunk is fetched once per call.  No atomics; every sum has a fixed order.  Rates: profiles/modal.txt.
#include "kernels_common.hpp"

namespace cps {

constexpr int BG_R = BLOCK_GRAM_ROWS;   // rows of a chunk
constexpr int BG_RP = BG_R + 1;         // doubles between the columns of the LDS copy: odd, so the 3 * BG_RP * 8 bytes between the column
                                        // triples of neighbouring tiles fall on distinct banks for up to 16 tiles (6 k mod 64 dwords)
constexpr int BG_T = 3;                 // a lane owns a BG_T x BG_T tile of G: 16 x 16 tiles = 256 lanes at 48 x 48
constexpr int BG_ACC = 256 * BG_T * BG_T;   // doubles the lanes' tiles take when they meet in LDS at the end
constexpr int BG_NPRE = (2 * BLOCK_MAX_COLS + 1 + 3) / 4;   // columns (the weight included) a lane stages per chunk: every fourth
static_assert(4 * BG_R == 256, "k_block_gram: four waves, each staging 64 rows of a column at a time");

// part[blockIdx.x][i][j] = sum over this workgroup's chunks (blockIdx.x, blockIdx.x + gridDim.x, ...) of w[r] * (A_i[r] * B_j[r]).
// A chunk of BG_R rows of all ka + kb columns and the weight (ones without one) is staged in LDS with coalesced 8-byte loads (any ld
// and any first column: no alignment is assumed), rows >= n as zeros, so the padding of a column is never read.  The ka x kb entries
// are cut into 3 x 3 tiles; with fewer than 256 tiles the rows of a chunk are dealt out to S = 256 / tiles lanes per tile (row r to
// lane r mod S), whose sums meet in LDS, s = 0 .. S - 1 in order, after the last chunk.  Tile shape and S depend on (ka, kb) alone, so every entry of G sums its rows in one order; the product
// A_i[r] * B_j[r] is rounded on its own (no contraction with the weight), so G(A, A) is symmetric bit for bit and an absent weight
// gives the bits of a weight of ones.
__global__ __launch_bounds__(256) void k_block_gram(const double *__restrict__ A, const double *__restrict__ B,
                                                    const double *__restrict__ w, size_t n, size_t ld, int ka, int kb,
                                                    double *__restrict__ part) {
  extern __shared__ double sm[];   // [ka + kb + 1][BG_RP], at least BG_ACC doubles
  const int kt = ka + kb;
  const int ntj = (kb + BG_T - 1) / BG_T, ntiles = ((ka + BG_T - 1) / BG_T) * ntj;
  const int S = min(256 / ntiles, BG_R);
  const int t = threadIdx.x % ntiles, s = threadIdx.x / ntiles;
  const bool active = s < S;
  const int ti = t / ntj, tj = t % ntj;
  int oa[BG_T], ob[BG_T];          // LDS offsets of the tile's columns; the ones past the last column repeat it (computed, never stored)
#pragma unroll
  for (int x = 0; x < BG_T; x++) {
    oa[x] = min(ti * BG_T + x, ka - 1) * BG_RP;
    ob[x] = (ka + min(tj * BG_T + x, kb - 1)) * BG_RP;
  }
  const double *sw = sm + (size_t)kt * BG_RP;
  double acc[BG_T][BG_T];
#pragma unroll
  for (int x = 0; x < BG_T; x++)
#pragma unroll
    for (int y = 0; y < BG_T; y++) acc[x][y] = 0.;

  // A lane stages the same row r of the columns q, q + 4, q + 8, ... (q = its wave) of every chunk: a wave loads 64 consecutive rows of
  // one column.  The loads of the NEXT chunk are issued into registers before the sums over the current one, whose LDS copy they
  // reach after the barrier that ends those sums: the fetch of a chunk runs under the arithmetic of the one before.
  const int lr = threadIdx.x % BG_R, q = threadIdx.x / BG_R;
  double pre[BG_NPRE];
  auto fetch = [&](size_t c) {
    const size_t row = c * BG_R + lr;
#pragma unroll
    for (int u = 0; u < BG_NPRE; u++) {
      const int col = q + 4 * u;
      double v = 0.;
      if (col <= kt && row < n) v = col < ka ? A[(size_t)col * ld + row] : (col < kt ? B[(size_t)(col - ka) * ld + row] : (w ? w[row] : 1.));
      pre[u] = v;
    }
  };
  const size_t nchunks = (n + BG_R - 1) / BG_R;
  fetch(blockIdx.x);
  for (size_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
#pragma unroll
    for (int u = 0; u < BG_NPRE; u++)
      if (q + 4 * u <= kt) sm[(q + 4 * u) * BG_RP + lr] = pre[u];
    __syncthreads();
    if (c + gridDim.x < nchunks) fetch(c + gridDim.x);
    if (active)
      for (int r = s; r < BG_R; r += S) {
        const double wv = sw[r];
        double a[BG_T], b[BG_T];
#pragma unroll
        for (int x = 0; x < BG_T; x++) { a[x] = sm[oa[x] + r]; b[x] = sm[ob[x] + r]; }
#pragma unroll
        for (int x = 0; x < BG_T; x++)
#pragma unroll
          for (int y = 0; y < BG_T; y++) acc[x][y] = __fma_rn(wv, __dmul_rn(a[x], b[y]), acc[x][y]);
      }
    __syncthreads();
  }
  if (active)
#pragma unroll
    for (int x = 0; x < BG_T; x++)
#pragma unroll
      for (int y = 0; y < BG_T; y++) sm[(s * ntiles + t) * (BG_T * BG_T) + x * BG_T + y] = acc[x][y];
  __syncthreads();
  double *out = part + (size_t)blockIdx.x * (size_t)(ka * kb);
  for (int e = threadIdx.x; e < ka * kb; e += 256) {
    const int i = e / kb, j = e % kb;
    const int slot = ((i / BG_T) * ntj + j / BG_T) * (BG_T * BG_T) + (i % BG_T) * BG_T + j % BG_T;
    double sum = sm[slot];
    for (int sp = 1; sp < S; sp++) sum += sm[sp * ntiles * (BG_T * BG_T) + slot];
    out[e] = sum;
  }
}

// G[e] = the sum of part[p][e], p < nparts, in a fixed order: 64 entries per workgroup, the partials of an entry dealt out to four lanes
// (p mod 4) whose sums are added in lane order
__global__ __launch_bounds__(256) void k_block_gram_final(const double *__restrict__ part, int nparts, int nent, double *__restrict__ G) {
  __shared__ double sh[256];
  const int e = blockIdx.x * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
  double sum = 0.;
  if (e < nent)
    for (int p = q; p < nparts; p += 4) sum += part[(size_t)p * nent + e];
  sh[threadIdx.x] = sum;
  __syncthreads();
  if (q == 0 && e < nent) G[e] = ((sh[threadIdx.x] + sh[threadIdx.x + 64]) + sh[threadIdx.x + 128]) + sh[threadIdx.x + 192];
}

// Y_j[r] = sum_{i < ka} A_i[r] C[i][j] + beta Y_j[r], j < ky: a lane per pair of rows (r, r + 256) of a 512-row chunk, the accumulators
// of its KYT >= ky output columns in registers, one coalesced load of A_i per row and step, row i of C (zero-padded to KYT, staged in LDS
// once per workgroup) read at a wave-uniform address.  beta == 0 does not read Y; rows >= n are neither read nor written; Y's
// columns must not overlap A's (the host refuses).
template <int KYT>
__global__ __launch_bounds__(256) void k_block_combine(double *__restrict__ Y, const double *__restrict__ A, const double *__restrict__ C,
                                                       double beta, size_t n, size_t ld, int ka, int ky) {
  __shared__ double sC[BLOCK_MAX_COLS * KYT];
  for (int idx = threadIdx.x; idx < ka * KYT; idx += 256) {
    const int i = idx / KYT, j = idx % KYT;
    sC[idx] = j < ky ? C[i * ky + j] : 0.;
  }
  __syncthreads();
  const size_t nchunks = (n + BLOCK_COMBINE_ROWS - 1) / BLOCK_COMBINE_ROWS;
  for (size_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const size_t r0 = c * BLOCK_COMBINE_ROWS + threadIdx.x, r1 = r0 + 256;
    const bool v0 = r0 < n, v1 = r1 < n;
    double acc0[KYT], acc1[KYT];
#pragma unroll
    for (int j = 0; j < KYT; j++) acc0[j] = acc1[j] = 0.;
#pragma unroll 2
    for (int i = 0; i < ka; i++) {
      const double a0 = v0 ? A[(size_t)i * ld + r0] : 0., a1 = v1 ? A[(size_t)i * ld + r1] : 0.;
#pragma unroll
      for (int j = 0; j < KYT; j++) {
        const double cij = sC[i * KYT + j];
        acc0[j] = __fma_rn(a0, cij, acc0[j]);
        acc1[j] = __fma_rn(a1, cij, acc1[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < KYT; j++)
      if (j < ky) {
        double *y = Y + (size_t)j * ld;
        if (v0) y[r0] = beta == 0. ? acc0[j] : __fma_rn(beta, y[r0], acc0[j]);
        if (v1) y[r1] = beta == 0. ? acc1[j] : __fma_rn(beta, y[r1], acc1[j]);
      }
  }
}

hipError_t launch_block_gram(const double *A, int ka, const double *B, int kb, const double *w, size_t n, size_t ld, double *part,
                             double *G, hipStream_t s) {
  if (ka < 1 || kb < 1 || ka > BLOCK_MAX_COLS || kb > BLOCK_MAX_COLS || !n || ld < n) return hipErrorInvalidValue;
  const size_t nchunks = (n + BG_R - 1) / BG_R;
  const int grid = (int)(nchunks < (size_t)BLOCK_GRAM_MAX_PARTS ? nchunks : (size_t)BLOCK_GRAM_MAX_PARTS);
  const size_t lds = sizeof(double) * (size_t)max((ka + kb + 1) * BG_RP, BG_ACC);
  hipLaunchKernelGGL(k_block_gram, dim3(grid), dim3(256), lds, s, A, B, w, n, ld, ka, kb, part);
  hipLaunchKernelGGL(k_block_gram_final, dim3((ka * kb + 63) / 64), dim3(256), 0, s, (const double *)part, grid, ka * kb, G);
  return hipGetLastError();
}

hipError_t launch_block_combine(double *Y, int ky, const double *A, int ka, const double *C, double beta, size_t n, size_t ld,
                                hipStream_t s) {
  if (ka < 1 || ky < 1 || ka > BLOCK_MAX_COLS || ky > BLOCK_MAX_COLS || !n || ld < n) return hipErrorInvalidValue;
  static_assert(BLOCK_COMBINE_ROWS == 2 * 256, "k_block_combine: a lane owns two rows of a chunk");
  const size_t nchunks = (n + BLOCK_COMBINE_ROWS - 1) / BLOCK_COMBINE_ROWS;
  const dim3 g((unsigned)(nchunks < (size_t)BLOCK_COMBINE_MAX_GROUPS ? nchunks : (size_t)BLOCK_COMBINE_MAX_GROUPS)), b(256);
  if (ky <= 8) hipLaunchKernelGGL(k_block_combine<8>, g, b, 0, s, Y, A, C, beta, n, ld, ka, ky);
  else if (ky <= 16) hipLaunchKernelGGL(k_block_combine<16>, g, b, 0, s, Y, A, C, beta, n, ld, ka, ky);
  else if (ky <= 32) hipLaunchKernelGGL(k_block_combine<32>, g, b, 0, s, Y, A, C, beta, n, ld, ka, ky);
  else hipLaunchKernelGGL(k_block_combine<48>, g, b, 0, s, Y, A, C, beta, n, ld, ka, ky);
  return hipGetLastError();
}

}  // namespace cps
