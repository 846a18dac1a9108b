// kernels_assemble.hip -- the restriction and its deterministic transpose: the plain gather (k_rstr) and its ordered transpose for
// the libCEED E-layout (k_rstr_transpose, k_multiplicity), the per-node sum in element order of the interlaced E-vector (k_assemble), the
// same sum with a consumer behind it (k_assemble_epi), and the halo pack / unpack-add that the interface sum of several GPUs puts around
// it.  The sums of the interlaced E-vector are kernel_node_sum.hpp's.
#include <algorithm>
#include "kernel_node_sum.hpp"

namespace cps {

// E-layout [e][c][n]
__global__ void k_rstr(const uint32_t *off, size_t total, int elemsize, int ncomp, int compstride, const double *l, double *e) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t n = i % elemsize, ec = i / elemsize, c = ec % ncomp, el = ec / ncomp;
    e[i] = l[(size_t)(off[el * elemsize + n] & OFF_MASK) + c * (size_t)compstride];
  }
}
// The transpose of the same layout, for any ncomp / compstride / elemsize (cold path: CeedElemRestrictionApply(CEED_TRANSPOSE) and the
// set-up / post-processing operators).  One lane per (row r of the restriction's transpose map, component c): the row's contributors
// cols[k] = e * elemsize + n, in element order, are summed into a register; then ONE add (or, with add == 0, a store) goes to the
// row's entry -- the rows of a map own disjoint entries of y, as k_assemble's do.
__global__ void k_rstr_transpose(const uint32_t *rowptr, const uint32_t *cols, const uint32_t *node_off, size_t total, int elemsize,
                                 int ncomp, int compstride, const double *evec, double *y, int add) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / ncomp, c = i % ncomp;
    double sum = 0.;
    for (uint32_t k = rowptr[r]; k < rowptr[r + 1]; k++) {
      const size_t e = cols[k] / (uint32_t)elemsize, n = cols[k] % (uint32_t)elemsize;
      sum += evec[(e * ncomp + c) * elemsize + n];
    }
    double *dst = y + (node_off[r] & OFF_MASK) + c * (size_t)compstride;
    *dst = add ? *dst + sum : sum;
  }
}
// the contributors of every row, counted: the entries of nodes no element holds are not written
__global__ void k_multiplicity(const uint32_t *rowptr, const uint32_t *node_off, size_t total, int ncomp, int compstride, double *y) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / ncomp, c = i % ncomp;
    y[(node_off[r] & OFF_MASK) + c * (size_t)compstride] = (double)(rowptr[r + 1] - rowptr[r]);
  }
}
// One lane per L-node.  The E-vector is interlaced [elem][node][3] like the L-vector: a contributor is
// 24 contiguous bytes, consecutive lanes (consecutively numbered nodes of one element) read and write
// consecutive 24-byte rows, so the three strided 8-byte accesses of a wave cover whole cache lines.
// Workgroups [nb_rows, gridDim.x) -- present only with `un.n` > 0 -- add the arrivals of a halo exchange instead
// (HaloUnpackArgs: different entries of y than any row of this launch).
// With the stencil code of the rows (rc.sid set) a row is summed by node_sum3_coded.
__global__ void k_assemble(const uint32_t *rowptr, const uint32_t *cols, const uint32_t *node_off,
                           const unsigned char *flags, const double *evec, double *y, int nnodes, int add, int nb_rows,
                           const HaloUnpackArgs un, const HaloPackFold pk, const RowCodeView rc) {
  // (no wave priority of its own: the row sums at priority 3 beside a fused kernel measured +2 %, profiles/r03_ab_experiments.txt item 15c)
  if ((int)blockIdx.x >= nb_rows) {
    halo_unpack_add(un, y, ((int)blockIdx.x - nb_rows) * blockDim.x + threadIdx.x, ((int)gridDim.x - nb_rows) * blockDim.x);
    return;
  }
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < nnodes; r += nb_rows * blockDim.x) {
    double a0 = 0., a1 = 0., a2 = 0.;
    if (rc.sid) node_sum3_coded(rc, rowptr, cols, evec, r, a0, a1, a2);
    else node_sum3(rowptr, cols, evec, r, a0, a1, a2);
    const unsigned fl = flags ? flags[r] : 0u;
    double *dst = y + (node_off[r] & OFF_MASK);
    if (fl & 1u) a0 = 0.;
    if (fl & 2u) a1 = 0.;
    if (fl & 4u) a2 = 0.;
    if (add) { a0 += dst[0]; a1 += dst[1]; a2 += dst[2]; }
    dst[0] = a0; dst[1] = a1; dst[2] = a2;
    if (pk.ptr)   // interface node: its finished sums go straight into the exchange's send buffer (no pack launch)
      for (uint32_t k = pk.ptr[r]; k < pk.ptr[r + 1]; k++) {
        const uint32_t e = pk.slot[k], cmp = e >> 30;
        pk.send[e & 0x3FFFFFFFu] = cmp == 0 ? a0 : (cmp == 1 ? a1 : a2);
      }
  }
}

// k_assemble with an EPILOGUE instead of the store of y (round 5): the operator's output t = A v is consumed where it is formed.
//   EPI_CHEB : one step of the Chebyshev smoother (elasticity.c:539-552) -- r = (r0 or r) - t, d = c1 dinv r + c2 d, x = d or x + d
//   EPI_RESID: w = b - t (the residual between the smoother and the restriction of a V-cycle)
// Rows [0, nnodes): the shell nodes of the transpose map, summed in contributor order exactly as k_assemble does.  Workgroups
// [nb_rows, gridDim.x): the dofs of the ELEMENT-INTERIOR nodes (int_off: their node offsets, elements in order), whose t the fused
// kernel stored into `t` itself.  t at the shell nodes is never written.  The apply's input may be d (or x) itself: a row is
// summed only after the last element that holds its node has finished (pipelined form: rows belong to the segment of their LAST
// contributor), and no later element gathers it.
__global__ void k_assemble_epi(const uint32_t *rowptr, const uint32_t *cols, const uint32_t *node_off, const unsigned char *flags,
                               const double *evec, int nnodes, int nb_rows, const EpilogueArgs ep, const RowCodeView rc) {
  if ((int)blockIdx.x >= nb_rows) {
    const size_t n = (size_t)ep.n_int * 3;
    for (size_t u = ((size_t)blockIdx.x - nb_rows) * blockDim.x + threadIdx.x; u < n; u += ((size_t)gridDim.x - nb_rows) * blockDim.x) {
      const size_t i = (size_t)(ep.int_off[u / 3] & OFF_MASK) + u % 3;
      const double ti = ep.t[i];
      if (ep.kind == EPI_CHEB) cheb_dof(ep.r0 ? ep.r0[i] : ep.r[i], true, ti, ep.r != nullptr, i, ep.x, ep.d, ep.r, ep.dinv, ep.c1, ep.c2, ep.assign_x);
      else ep.w[i] = ep.b[i] - ti;
    }
    return;
  }
  // The SUM is formed a lane per row (node), as k_assemble forms it -- one walk of rowptr / cols per node, the same additions in the
  // same order: same bits.  The CONSUMER then runs a lane per DOF: the 64 rows of a wave are 192 dofs = three rounds of 64 lanes,
  // dof j = 64 q + lane belongs to the row of lane j / 3, component j % 3 (sums and node offsets fetched from that lane by
  // ds_bpermute), so every stream of the epilogue -- r, dinv, d, x, b, w -- is read and written 8 bytes per lane, contiguous over the
  // wave where the rows' nodes are numbered consecutively, instead of three 24-byte-strided accesses per lane (measured 164 -> 100 us
  // per launch over a 99 000-hex solve); the streams are requested BEFORE the dependent chain rowptr -> cols -> E-vector.
  const int lane = threadIdx.x & 63;
  const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), nwaves = (int)((nb_rows * blockDim.x) >> 6);
  for (int row0 = wave * 64; row0 < nnodes; row0 += nwaves * 64) {     // (wave-uniform trip count: every lane takes part in the shuffles)
    const int r = row0 + lane;
    const bool live = r < nnodes;
    const uint32_t off = live ? (node_off[r] & OFF_MASK) : 0u;
    size_t idx[3];
    bool ok[3];
    double s0[3], s1[3], s2[3], s3[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const int j = 64 * q + lane, src = j / 3, c = j % 3;
      idx[q] = (size_t)__shfl(off, src, 64) + c;
      ok[q] = row0 + src < nnodes;
      s0[q] = s1[q] = s2[q] = s3[q] = 0.;
      if (ok[q]) {
        if (ep.kind == EPI_CHEB) {
          s0[q] = ep.r0 ? ep.r0[idx[q]] : ep.r[idx[q]]; s1[q] = ep.dinv[idx[q]];
          s2[q] = ep.c2 != 0. ? ep.d[idx[q]] : 0.; s3[q] = ep.assign_x ? 0. : ep.x[idx[q]];
        } else s0[q] = ep.b[idx[q]];
      }
    }
    double a0 = 0., a1 = 0., a2 = 0.;
    if (live) {
      if (rc.sid) node_sum3_coded(rc, rowptr, cols, evec, r, a0, a1, a2);
      else node_sum3(rowptr, cols, evec, r, a0, a1, a2);
      const unsigned fl = flags ? flags[r] : 0u;
      if (fl & 1u) a0 = 0.;
      if (fl & 2u) a1 = 0.;
      if (fl & 4u) a2 = 0.;
    }
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const int j = 64 * q + lane, src = j / 3, c = j % 3;
      const double t0 = __shfl(a0, src, 64), t1 = __shfl(a1, src, 64), t2 = __shfl(a2, src, 64);
      const double ti = c == 0 ? t0 : (c == 1 ? t1 : t2);
      if (!ok[q]) continue;
      if (ep.kind == EPI_CHEB) cheb_dof_regs(s0[q], true, ti, ep.r != nullptr, idx[q], s1[q], s2[q], s3[q], ep.x, ep.d, ep.r, ep.c1, ep.c2, ep.assign_x);
      else ep.w[idx[q]] = s0[q] - ti;
    }
  }
}
// the stencil code of the rows of a launch (null: none was built, every row takes rowptr / cols)
static RowCodeView row_code_view(const NodeMap &m) {
  return m.sid ? RowCodeView{m.pos0 + m.row0, m.sid + m.row0, m.stencil} : RowCodeView{nullptr, nullptr, nullptr};
}
hipError_t launch_assemble_epi(const NodeMap &m, const unsigned char *flags, const double *evec, const EpilogueArgs &ep, hipStream_t s) {
  if (m.nnodes <= 0 && ep.n_int <= 0) return hipSuccess;
  constexpr int AB = 256;
  const unsigned nb_rows = (unsigned)((std::max(m.nnodes, 0) + AB - 1) / AB);
  const unsigned nb_int = (unsigned)std::min<size_t>(((size_t)std::max(ep.n_int, 0) * 3 + AB - 1) / AB, 4096);
  hipLaunchKernelGGL(k_assemble_epi, dim3(nb_rows + nb_int), dim3(AB), 0, s, m.rowptr + m.row0, m.cols, m.node_off + m.row0,
                     flags ? flags + m.row0 : nullptr, evec, m.nnodes, (int)nb_rows, ep, row_code_view(m));
  return hipGetLastError();
}
hipError_t launch_assemble(const NodeMap &m, const unsigned char *flags, const double *evec, double *y, int add, hipStream_t s,
                           const HaloUnpackArgs *unpack, const HaloPackFold *pack) {
  const int nun = unpack ? unpack->n : 0;
  if (m.nnodes <= 0 && nun <= 0) return hipSuccess;
  constexpr int AB = 256;      // threads per workgroup of k_assemble: 64, 128 and 512 measured in round 4, nothing (profiles/r04_ab_experiments.txt item 18)
  const unsigned nb_rows = (unsigned)((std::max(m.nnodes, 0) + AB - 1) / AB);
  const unsigned nb_un = (unsigned)std::min((nun + AB - 1) / AB, 1024);
  hipLaunchKernelGGL(k_assemble, dim3(nb_rows + nb_un), dim3(AB), 0, s, m.rowptr + m.row0, m.cols, m.node_off + m.row0,
                     flags ? flags + m.row0 : nullptr, evec, y, m.nnodes, add, (int)nb_rows,
                     unpack ? *unpack : HaloUnpackArgs{nullptr, nullptr, nullptr, nullptr, 0},
                     pack ? HaloPackFold{pack->ptr + m.row0, pack->slot, pack->send} : HaloPackFold{nullptr, nullptr, nullptr},
                     row_code_view(m));
  return hipGetLastError();
}

__global__ void k_halo_pack(const uint32_t *idx, int n, const double *y, double *buf) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) buf[i] = y[idx[i]];
}
__global__ void k_halo_unpack_add(const HaloUnpackArgs un, double *y) {
  halo_unpack_add(un, y, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}
hipError_t launch_halo_pack(const uint32_t *idx, int n, const double *y, double *buf, hipStream_t s) {
  return launch_stream(k_halo_pack, (size_t)std::max(n, 0), s, idx, n, y, buf);
}
hipError_t launch_halo_unpack_add(const HaloUnpackArgs &u, double *y, hipStream_t s) {
  return launch_stream(k_halo_unpack_add, (size_t)std::max(u.n, 0), s, u, y);
}

hipError_t launch_rstr_gather(const uint32_t *off, int nelem, int elemsize, int ncomp, int compstride,
                              const double *l, double *e, hipStream_t s) {
  const size_t total = (size_t)nelem * elemsize * ncomp;
  return launch_stream(k_rstr, total, s, off, total, elemsize, ncomp, compstride, l, e);
}
hipError_t launch_rstr_transpose(const NodeMap &m, int elemsize, int ncomp, int compstride, const double *e, double *l, int add, hipStream_t s) {
  const size_t total = (size_t)std::max(m.nnodes, 0) * ncomp;
  return launch_stream(k_rstr_transpose, total, s, m.rowptr + m.row0, m.cols, m.node_off + m.row0, total, elemsize, ncomp, compstride, e, l, add);
}
hipError_t launch_multiplicity(const NodeMap &m, int ncomp, int compstride, double *l, hipStream_t s) {
  const size_t total = (size_t)std::max(m.nnodes, 0) * ncomp;
  return launch_stream(k_multiplicity, total, s, m.rowptr + m.row0, m.node_off + m.row0, total, ncomp, compstride, l);
}

}  // namespace cps
