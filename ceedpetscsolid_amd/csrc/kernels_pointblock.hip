// kernels_pointblock.hip -- point-block Jacobi: the 3 x 3 nodal blocks of B^T D B (CeedOperatorLinearAssemblePointBlockDiagonal,
// the matrix PCPBJACOBI inverts), their inverses, and the Chebyshev step that multiplies by them.
//
// The element blocks are k_pbdiag_sf's: the scalar diagonal's sum-factorised scheme in three rounds, one per input component, defined
// beside k_diag_sf in kernel_diag_sf.hpp.  This file instantiates it (the scalar kernel's instantiations are kernels_dispatch.hip's) and
// holds the four lane-per-node kernels: the sum over a node's elements, the inverses, the product, the smoother step.
#include "kernel_diag_sf.hpp"
#include "kernels_pointblock.hpp"

namespace cps {

hipError_t launch_pbdiag(int P, int Q, int qf, const BasisTables &t, const DiagArgs &a, hipStream_t s, const char **name) {
#define CPS_PB(Pv, Qv) CPS_DIAG_CASES(k_pbdiag_sf, "pbdiag", Pv, Qv)
  CPS_DIAG_PQ(CPS_PB)
#undef CPS_PB
  return hipErrorInvalidValue;
}

// One lane per L-node, the contributors summed in element order as k_assemble sums them; nine values per contributor.
// (A loop of its own: node_sum3 written generically over the width compiles k_assemble to other code than the one its traffic profile was taken with.)
__global__ void k_pb_assemble(const uint32_t *rowptr, const uint32_t *cols, const uint32_t *node_off, const double *evec,
                              double *blocks, int nnodes) {
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < nnodes; r += gridDim.x * blockDim.x) {
    double acc[9];
#pragma unroll
    for (int j = 0; j < 9; j++) acc[j] = 0.;
    for (uint32_t k = rowptr[r]; k < rowptr[r + 1]; k++) {
      const double *p = evec + (size_t)cols[k] * 9;
#pragma unroll
      for (int j = 0; j < 9; j++) acc[j] += p[j];
    }
    double *dst = blocks + 3 * (size_t)(node_off[r] & OFF_MASK);
#pragma unroll
    for (int j = 0; j < 9; j++) dst[j] = acc[j];
  }
}

// Inverse of the principal sub-block of the kept components, embedded in zeros.  A dropped component is replaced by a unit row and
// column first (products with 1 and 0 are exact), so one code path serves all eight patterns: inverse = adjugate / determinant, the
// pivots of the elimination without interchanges (all positive iff the block is positive definite) decide what is counted as bad.
__global__ void k_pb_invert(double *blocks, size_t nnodes, int *n_bad) {
#pragma clang fp contract(off)
  int nb = 0;
  for (size_t n = blockIdx.x * (size_t)blockDim.x + threadIdx.x; n < nnodes; n += (size_t)gridDim.x * blockDim.x) {
    double *B = blocks + 9 * n;
    double m[3][3];
    bool keep[3];
#pragma unroll
    for (int i = 0; i < 3; i++) keep[i] = B[4 * i] != 0.;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) m[i][j] = (keep[i] && keep[j]) ? B[3 * i + j] : (i == j ? 1. : 0.);
    const double p0 = m[0][0];
    const double l1 = m[1][0] / p0, l2 = m[2][0] / p0;
    const double b11 = m[1][1] - l1 * m[0][1], b12 = m[1][2] - l1 * m[0][2];
    const double b21 = m[2][1] - l2 * m[0][1], b22 = m[2][2] - l2 * m[0][2];
    const double p1 = b11, p2 = b22 - (b21 / p1) * b12;
    const double big = 1.7976931348623157e308;
    if (!(p0 > 0. && p0 <= big && p1 > 0. && p1 <= big && p2 > 0. && p2 <= big)) nb++;
    const double c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1];
    const double c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2];
    const double c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
    const double det = (m[0][0] * c00 + m[0][1] * c01) + m[0][2] * c02;
    double inv[3][3];
    inv[0][0] = c00 / det;
    inv[1][0] = c01 / det;
    inv[2][0] = c02 / det;
    inv[0][1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) / det;
    inv[1][1] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) / det;
    inv[2][1] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) / det;
    inv[0][2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) / det;
    inv[1][2] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) / det;
    inv[2][2] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) / det;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) B[3 * i + j] = (keep[i] && keep[j]) ? inv[i][j] : 0.;
  }
  if (n_bad) {     // (every lane of the wave is back here: one atomic per wave that has something to report)
    for (int o = 32; o > 0; o >>= 1) nb += __shfl_down(nb, o, 64);
    if ((threadIdx.x & 63) == 0 && nb) atomicAdd(n_bad, nb);
  }
}

CPS_DEV void pb_mult3(const double *B, double r0, double r1, double r2, double *z) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 3; i++) z[i] = (B[3 * i] * r0 + B[3 * i + 1] * r1) + B[3 * i + 2] * r2;
}
__global__ void k_pb_mult(double *w, const double *blocks, const double *x, size_t nnodes) {
  for (size_t n = blockIdx.x * (size_t)blockDim.x + threadIdx.x; n < nnodes; n += (size_t)gridDim.x * blockDim.x) {
    double B[9], z[3];
#pragma unroll
    for (int j = 0; j < 9; j++) B[j] = blocks[9 * n + j];
    const double x0 = x[3 * n], x1 = x[3 * n + 1], x2 = x[3 * n + 2];
    pb_mult3(B, x0, x1, x2, z);
    w[3 * n] = z[0]; w[3 * n + 1] = z[1]; w[3 * n + 2] = z[2];
  }
}
// One node of a Chebyshev step with blocks: cheb_dof's definition (kernel_node_sum.hpp) with dinv .* r replaced by B_n r_n; explicit
// operation order, no contraction left to the compiler.
__global__ void k_pb_cheb_step(double *x, double *d, double *r, const double *b, const double *t, const double *blocks, double c1,
                               double c2, int assign_x, size_t nnodes) {
#pragma clang fp contract(off)
  for (size_t n = blockIdx.x * (size_t)blockDim.x + threadIdx.x; n < nnodes; n += (size_t)gridDim.x * blockDim.x) {
    double B[9], ri[3], z[3];
#pragma unroll
    for (int j = 0; j < 9; j++) B[j] = blocks[9 * n + j];
#pragma unroll
    for (int c = 0; c < 3; c++) ri[c] = t ? b[3 * n + c] - t[3 * n + c] : b[3 * n + c];
    if (r) { r[3 * n] = ri[0]; r[3 * n + 1] = ri[1]; r[3 * n + 2] = ri[2]; }
    pb_mult3(B, ri[0], ri[1], ri[2], z);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      double di = c1 * z[c];
      if (c2 != 0.) di = __builtin_fma(c2, d[3 * n + c], di);
      const double xi = assign_x ? 0. : x[3 * n + c];
      d[3 * n + c] = di;
      x[3 * n + c] = assign_x ? di : xi + di;
    }
  }
}

hipError_t launch_pb_assemble(const NodeMap &m, const double *evec, double *blocks, hipStream_t s) {
  return launch_stream(k_pb_assemble, (size_t)(m.nnodes > 0 ? m.nnodes : 0), s, m.rowptr + m.row0, m.cols, m.node_off + m.row0, evec, blocks, m.nnodes);
}
hipError_t launch_pb_invert(double *blocks, size_t nnodes, int *n_bad, hipStream_t s) {
  return launch_stream(k_pb_invert, nnodes, s, blocks, nnodes, n_bad);
}
hipError_t launch_pb_mult(double *w, const double *blocks, const double *x, size_t nnodes, hipStream_t s) {
  return launch_stream(k_pb_mult, nnodes, s, w, blocks, x, nnodes);
}
hipError_t launch_pb_cheb_step(double *x, double *d, double *r, const double *b, const double *t, const double *blocks, double c1,
                               double c2, int assign_x, size_t nnodes, hipStream_t s) {
  return launch_stream(k_pb_cheb_step, nnodes, s, x, d, r, b, t, blocks, c1, c2, assign_x, nnodes);
}

}  // namespace cps
