// kernel_node_sum.hpp -- the sums and the update that several kernels must form with the SAME bits, each stated once: the
// deterministic restriction transpose of one node (k_assemble, k_assemble_epi), the unpack-add of a halo exchange (k_halo_unpack_add,
// k_assemble's extra workgroups) and one dof of a Chebyshev step (k_cheb_update, k_assemble_epi).
#pragma once
#include "kernels_common.hpp"

namespace cps {

// Row r of the transpose map, three values per contributor (the E-vector is interlaced [elem][node][3]), added to a0, a1, a2.
// Four contributors per trip: the index loads, then the twelve value loads, are issued together (the chain rowptr -> cols ->
// E-vector is latency bound otherwise); lanes with fewer contributors re-read their last one and discard it.  Sums are still
// formed in contributor (= element) order.
CPS_DEV void node_sum3(const uint32_t *rowptr, const uint32_t *cols, const double *evec, int r, double &a0, double &a1, double &a2) {
  const uint32_t k0 = rowptr[r], k1 = rowptr[r + 1];
  for (uint32_t k = k0; k < k1; k += 4) {
    uint32_t c[4];
#pragma unroll
    for (int j = 0; j < 4; j++) c[j] = cols[k + j < k1 ? k + j : k1 - 1];
    double v[4][3];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const double *p = evec + (size_t)c[j] * 3;
      v[j][0] = p[0]; v[j][1] = p[1]; v[j][2] = p[2];
    }
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (k + j < k1) { a0 += v[j][0]; a1 += v[j][1]; a2 += v[j][2]; }
  }
}

// Destination entries first, first + stride, ... of a halo exchange: y[dst[u]] += its arrivals, in neighbour-list order.
CPS_DEV void halo_unpack_add(const HaloUnpackArgs &un, double *y, int first, int stride) {
  for (int u = first; u < un.n; u += stride) {
    double v = y[un.dst[u]];
    for (uint32_t k = un.ptr[u]; k < un.ptr[u + 1]; k++) v += un.recv[un.slot[k]];
    y[un.dst[u]] = v;
  }
}

// One dof of a Chebyshev step: r = rbase - t (has_t), d = c1 dinv r + c2 d, x = d or x + d.  Explicit operation order, no
// contraction left to the compiler, so that the stand-alone update and the epilogue of the fused apply give the same bits.
CPS_DEV void cheb_dof_regs(double rbase, bool has_t, double ti, bool store_r, size_t i, double dinv_i, double d_i, double x_i, double *x, double *d,
                           double *r, double c1, double c2, int assign_x) {
#pragma clang fp contract(off)
  const double ri = has_t ? rbase - ti : rbase;
  if (store_r) r[i] = ri;
  double di = (c1 * dinv_i) * ri;
  if (c2 != 0.) di = __builtin_fma(c2, d_i, di);
  d[i] = di;
  x[i] = assign_x ? di : x_i + di;
}
CPS_DEV void cheb_dof(double rbase, bool has_t, double ti, bool store_r, size_t i, double *x, double *d, double *r, const double *dinv,
                      double c1, double c2, int assign_x) {
  cheb_dof_regs(rbase, has_t, ti, store_r, i, dinv[i], c2 != 0. ? d[i] : 0., assign_x ? 0. : x[i], x, d, r, c1, c2, assign_x);
}

}  // namespace cps
