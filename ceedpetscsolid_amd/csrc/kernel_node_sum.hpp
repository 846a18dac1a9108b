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

// The same sum from the row's STENCIL CODE (row_code.hpp): contributor j at pos0[r] + distance j of stencil sid[r] -- one load (the
// row's six bytes) and a table lookup before the E-vector, where node_sum3 has the dependent pair rowptr -> cols.  The table is read
// with plain loads: it is small (17 stencils = 544 bytes for the swept cylinder of bench.py, 32 bytes each) and every wave of the launch reads it, so it
// stays in the CU's L1; a copy in LDS would cost each 256-row workgroup -- one trip over its rows -- a staging pass and a barrier in
// front of its first E-vector load, and would bound the table by what eight workgroups per CU leave of the LDS.  The table repeats a
// stencil's last distance past its count, so the loads of a half (four contributors) are issued together unconditionally, as
// node_sum3 issues them; the additions are node_sum3's, in contributor order: same bits.  Escape rows ARE node_sum3's.
constexpr int ROWCODE_LANE_MAXC = 8;     // row_code.hpp's ROWCODE_MAXC: contributors of a coded row
struct RowCodeView { const uint32_t *pos0; const uint16_t *sid; const uint32_t *stencil; };
CPS_DEV void node_sum3_coded(const RowCodeView &rc, const uint32_t *rowptr, const uint32_t *cols, const double *evec, int r, double &a0, double &a1, double &a2) {
  const uint32_t s = rc.sid[r];
  uint32_t p0 = rc.pos0[r];
  asm volatile("" : "+v"(p0));                 // (requested beside sid, not behind the escape test: see `hi` below)
  if (s == 0xFFFFu) { node_sum3(rowptr, cols, evec, r, a0, a1, a2); return; }
  const uint4 *st = reinterpret_cast<const uint4 *>(rc.stencil) + 2 * (size_t)s;
  uint4 lo = st[0], hi = st[1];                // {count, distances 1 .. 3}, {distances 4 .. 7}: one 32-byte sector
  // (both halves are values HERE: left to itself hipcc sinks the load of `hi` into the branch below, behind a wait for every load in flight)
  asm volatile("" : "+v"(lo.x), "+v"(lo.y), "+v"(lo.z), "+v"(lo.w), "+v"(hi.x), "+v"(hi.y), "+v"(hi.z), "+v"(hi.w));
  const uint32_t n = lo.x;
  const uint32_t d[ROWCODE_LANE_MAXC] = {0u, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  const bool more = n > 4u;                    // (a vertex of the mesh: one or two lanes of most waves)
  double v[ROWCODE_LANE_MAXC][3] = {};
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const double *p = evec + (size_t)(p0 + d[j]) * 3;
    v[j][0] = p[0]; v[j][1] = p[1]; v[j][2] = p[2];
  }
  if (more) {                                  // requested BEFORE the first half is waited for: one round trip to memory for either count
#pragma unroll
    for (int j = 4; j < 8; j++) {
      const double *p = evec + (size_t)(p0 + d[j]) * 3;
      v[j][0] = p[0]; v[j][1] = p[1]; v[j][2] = p[2];
    }
  }
  // selects, not branches, around the additions: hipcc sinks a load into the branch of its only use, and the loads then go out one
  // dependent group at a time
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const bool take = (uint32_t)j < n;
    const double t0 = a0 + v[j][0], t1 = a1 + v[j][1], t2 = a2 + v[j][2];
    a0 = take ? t0 : a0; a1 = take ? t1 : a1; a2 = take ? t2 : a2;
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
