// kernels_transfer.hip -- p-multigrid transfer (setuplibceed.c:847-862; matops.c:115-203), round 5: pencil passes, OWNER form;
// k_transfer's instantiations over the level pairs, and the weights.
//
// A prolonged H1 field is single-valued at a fine node shared by several elements (the tensor-product interpolant on a
// face sees that face's coarse nodes only), so sum_e contribution_e / multiplicity (matops.c:149) IS any one element's
// contribution, to rounding.  Every fine node therefore has ONE owning element (the first that holds it, in element
// order: TransferArgs::own_f):
//   PROLONG : coarse gather -> interp Pc -> Pf in three pencil passes -> each element STORES the fine nodes it owns.
//             No fine E-vector, no scatter-add, no k_assemble, no multVec read on one rank.
//   RESTRICT: each element GATHERS the fine nodes it owns (the others read as zero) -> interp^T -> coarse E-vector
//             -> launch_assemble() (27 nodes per element at Pc = 3: small, and bit-reproducible) -- exactly the transpose.
// The per-dof weight w = (fine-side scale) x (local multiplicity) is 1 where the scale is 1 / multiplicity (one rank); it is
// read (w_f) only when the host found an entry that differs: the interface nodes of an element partition, whose scale holds
// the multiplicity over ALL ranks, or the extension-free form without a scale (plain libCEED semantics: w = multiplicity).
//
// One wave64 = one workgroup owns XferGeom::E elements.  In a pass a lane owns one line of an element along the contraction
// direction, one component; tables are wave-uniform (kernarg segment -> SGPR operands).  LDS arrays are laid out so that the
// lane-fastest index of the pass that reads them is contiguous: U0 [kc][jc][ic][c], U1 [kc][jc][if][c], U2 [kc][jf][if][c].
#include "kernels_common.hpp"

namespace cps {

constexpr uint32_t XFER_SKIP = 0xFFFFFFFFu;    // own_f entry of a fine node another element owns
constexpr int xfer_group_elems(int PF) { return PF <= 3 ? 4 : (PF == 4 ? 4 : (PF == 5 ? 2 : 1)); }
template <int PC, int PF> struct XferGeom {
  static constexpr int C3 = PC * PC * PC, F2 = PF * PF, F3 = PF * PF * PF;
  static constexpr int E = xfer_group_elems(PF);
  static constexpr int N0 = 3 * C3, N1 = 3 * PC * PC * PF, N2 = 3 * PC * F2;   // doubles per element of U0, U1, U2
  static constexpr int NI = E * PC * PC * 3, NJ = E * PC * PF * 3, NK = E * F2 * 3;   // pencils of the i-, j-, k-pass
  static constexpr int KR = (NK + 63) / 64;                                    // rounds of the k-pass
};

template <int PC, int PF, bool PROLONG, bool WEIGHTED>
__global__ __launch_bounds__(64) void k_transfer(const BasisTables tab, const TransferArgs a) {
  using G = XferGeom<PC, PF>;
  constexpr int C3 = G::C3, F2 = G::F2, F3 = G::F3, E = G::E, N0 = G::N0, N1 = G::N1, N2 = G::N2, KR = G::KR;
  constexpr int SR = (E * N0 + 63) / 64;           // rounds of the coarse-side staging (a lane per coarse value)
  // U0 (the coarse values: read by the first pass of a prolongation, written by the last of a restriction) shares its storage with U2
  // (written by the j-pass / read by the j^T pass: never live together) -- 5.8 instead of 7.1 KB per wave at (3, 5): 27 instead of 22 waves per CU
  static_assert(N0 <= N2, "the coarse slab fits the widest intermediate");
  __shared__ double U1[E * N1], U2[E * N2];
  double *const U0 = U2;
  const int lane = threadIdx.x;
  // XCD-aware: the groups are cut into 8 contiguous chunks; block b serves chunk b % 8 (blocks b and b + 8 share an XCD under the
  // round-robin placement), so the elements that share coarse and fine nodes meet in one L2 (prolong p2 -> p4 at 99 000 hexes:
  // 175 -> 82 MB fetched).  One group per workgroup, NOT a persistent loop: a wave that ends never waits for its stores, a wave
  // that goes on to a next group does (its next loads count behind them in vmcnt) -- measured 47 -> 69 us for that prolongation.
  const int ngroups = (a.nelem + E - 1) / E, chunk = (ngroups + 7) / 8;
  const int grp = (int)(blockIdx.x % 8) * chunk + (int)(blockIdx.x / 8);
  if (grp >= min(ngroups, (int)(blockIdx.x % 8 + 1) * chunk)) return;
  // B[f][c] = tab.interp[f * PC + c]: value of coarse basis function c at fine node f (GLL points of the fine level).
  // Loads are written as straight-line rounds (no data-dependent control flow around them: all are in flight together); a lane
  // without work reads a valid entry of its group and discards it.
  auto load_own = [&](int g, uint32_t (&o)[KR][PF]) {      // the k-pass columns of this lane: the fine nodes they own
    const int e0 = g * E, ne = min(E, a.nelem - e0);
#pragma unroll
    for (int r = 0; r < KR; r++) {
      const int t = lane + 64 * r, el = t / (3 * F2), n2 = (t % (3 * F2)) / 3;
      const bool live = t < ne * 3 * F2;
#pragma unroll
      for (int k = 0; k < PF; k++) {
        const uint32_t v = a.own_f[(size_t)e0 * F3 + (live ? el * F3 + k * F2 + n2 : 0)];
        o[r][k] = live ? v : XFER_SKIP;
      }
    }
  };
  auto load_offc = [&](int g, uint32_t (&o)[SR]) {
    const int e0 = g * E, ne = min(E, a.nelem - e0);
#pragma unroll
    for (int r = 0; r < SR; r++) {
      const int t = lane + 64 * r;
      o[r] = a.off_c[(size_t)e0 * C3 + (t < ne * N0 ? t / 3 : 0)];
    }
  };
  uint32_t own[KR][PF], offc[SR];
  load_own(grp, own);
  load_offc(grp, offc);
  {
    const int e0 = grp * E, ne = min(E, a.nelem - e0);
    if constexpr (PROLONG) {
      double xin[SR];
#pragma unroll
      for (int r = 0; r < SR; r++) xin[r] = a.x[(offc[r] & OFF_MASK) + (lane + 64 * r) % 3];
      // ApplyAdd (the V-cycle's correction added in place): the old values of the owned nodes are requested NOW, behind the
      // owner list that has just landed, so that their latency passes under the three passes instead of in front of the stores
      double yold[KR][PF];
      if (a.add) {
#pragma unroll
        for (int r = 0; r < KR; r++) {
          const int c = ((lane + 64 * r) % (3 * F2)) % 3;
#pragma unroll
          for (int f = 0; f < PF; f++) yold[r][f] = own[r][f] == XFER_SKIP ? 0. : a.y[(own[r][f] & OFF_MASK) + c];
        }
      }
#pragma unroll
      for (int r = 0; r < SR; r++) {
        const int t = lane + 64 * r, c = t % 3;
        const bool dead = a.mask_c && ((offc[r] >> (OFF_FLAG_SHIFT + c)) & 1u);
        if (t < ne * N0) U0[t] = dead ? 0. : xin[r];
      }
      __syncthreads();
      for (int t = lane; t < G::NI; t += 64) {          // i: U0[kc][jc][ic][c] -> U1[kc][jc][if][c]
        const int el = t / (PC * PC * 3), r = t % (PC * PC * 3), m = r / 3, c = r % 3;
        double u[PC];
#pragma unroll
        for (int i = 0; i < PC; i++) u[i] = U0[el * N0 + (m * PC + i) * 3 + c];
#pragma unroll
        for (int f = 0; f < PF; f++) {
          double s = 0.;
#pragma unroll
          for (int i = 0; i < PC; i++) s += tab.interp[f * PC + i] * u[i];
          U1[el * N1 + (m * PF + f) * 3 + c] = s;
        }
      }
      __syncthreads();
      for (int t = lane; t < G::NJ; t += 64) {          // j: U1[kc][jc][if][c] -> U2[kc][jf][if][c]
        const int el = t / (PC * PF * 3), r = t % (PC * PF * 3), kc = r / (PF * 3), ic = r % (PF * 3);
        double u[PC];
#pragma unroll
        for (int j = 0; j < PC; j++) u[j] = U1[el * N1 + (kc * PC + j) * PF * 3 + ic];
#pragma unroll
        for (int f = 0; f < PF; f++) {
          double s = 0.;
#pragma unroll
          for (int j = 0; j < PC; j++) s += tab.interp[f * PC + j] * u[j];
          U2[el * N2 + (kc * PF + f) * PF * 3 + ic] = s;
        }
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < KR; r++) {                    // k: U2[kc][jf][if][c] -> the owned fine nodes of the column, stored
        const int t = lane + 64 * r, el = t / (3 * F2), rem = t % (3 * F2), c = rem % 3;
        if (t >= ne * 3 * F2) break;
        double u[PC];
#pragma unroll
        for (int k = 0; k < PC; k++) u[k] = U2[el * N2 + k * F2 * 3 + rem];
#pragma unroll
        for (int f = 0; f < PF; f++) {
          const uint32_t off = own[r][f];
          if (off == XFER_SKIP) continue;
          double s = 0.;
#pragma unroll
          for (int k = 0; k < PC; k++) s += tab.interp[f * PC + k] * u[k];
          double *dst = a.y + (off & OFF_MASK) + c;
          if constexpr (WEIGHTED) s *= a.w_f[(off & OFF_MASK) + c];
          if (a.mask_f && ((off >> (OFF_FLAG_SHIFT + c)) & 1u)) s = 0.;
          *dst = a.add ? yold[r][f] + s : s;
        }
      }
    } else {
      // all gathers of the wave's columns are issued together (lanes without an owned node read entry 0 and discard it)
      double xv[KR][PF];
#pragma unroll
      for (int r = 0; r < KR; r++) {
        const int c = ((lane + 64 * r) % (3 * F2)) % 3;
#pragma unroll
        for (int f = 0; f < PF; f++) {
          const uint32_t off = own[r][f];
          const uint32_t idx = off == XFER_SKIP ? 0u : (off & OFF_MASK) + c;
          xv[r][f] = a.x[idx];
          if constexpr (WEIGHTED) xv[r][f] *= a.w_f[idx];
        }
      }
#pragma unroll
      for (int r = 0; r < KR; r++) {                    // k^T: the owned fine nodes of the column -> U2[kc][jf][if][c]
        const int t = lane + 64 * r, el = t / (3 * F2), rem = t % (3 * F2), c = rem % 3;
        double v[PF];
#pragma unroll
        for (int f = 0; f < PF; f++) {
          const uint32_t off = own[r][f];
          const bool dead = off == XFER_SKIP || (a.mask_f && ((off >> (OFF_FLAG_SHIFT + c)) & 1u));
          v[f] = dead ? 0. : xv[r][f];
        }
        if (t < E * 3 * F2) {
#pragma unroll
          for (int k = 0; k < PC; k++) {
            double s = 0.;
#pragma unroll
            for (int f = 0; f < PF; f++) s += tab.interp[f * PC + k] * v[f];
            U2[el * N2 + k * F2 * 3 + rem] = s;
          }
        }
      }
      __syncthreads();
      for (int t = lane; t < G::NJ; t += 64) {          // j^T: U2[kc][jf][if][c] -> U1[kc][jc][if][c]
        const int el = t / (PC * PF * 3), r = t % (PC * PF * 3), kc = r / (PF * 3), ic = r % (PF * 3);
        double v[PF];
#pragma unroll
        for (int f = 0; f < PF; f++) v[f] = U2[el * N2 + (kc * PF + f) * PF * 3 + ic];
#pragma unroll
        for (int j = 0; j < PC; j++) {
          double s = 0.;
#pragma unroll
          for (int f = 0; f < PF; f++) s += tab.interp[f * PC + j] * v[f];
          U1[el * N1 + (kc * PC + j) * PF * 3 + ic] = s;
        }
      }
      __syncthreads();
      for (int t = lane; t < G::NI; t += 64) {          // i^T: U1[kc][jc][if][c] -> U0[kc][jc][ic][c]
        const int el = t / (PC * PC * 3), r = t % (PC * PC * 3), m = r / 3, c = r % 3;
        double v[PF];
#pragma unroll
        for (int f = 0; f < PF; f++) v[f] = U1[el * N1 + (m * PF + f) * 3 + c];
#pragma unroll
        for (int i = 0; i < PC; i++) {
          double s = 0.;
#pragma unroll
          for (int f = 0; f < PF; f++) s += tab.interp[f * PC + i] * v[f];
          U0[el * N0 + (m * PC + i) * 3 + c] = s;
        }
      }
      __syncthreads();
      // the group's block of the coarse E-vector [elem][node][3] is contiguous: whole-line stores; masked entries travel as zeros
#pragma unroll
      for (int r = 0; r < SR; r++) {
        const int t = lane + 64 * r, c = t % 3;
        const bool dead = a.mask_c && ((offc[r] >> (OFF_FLAG_SHIFT + c)) & 1u);
        if (t < ne * N0) a.evec[(size_t)e0 * N0 + t] = dead ? 0. : U0[t];
      }
    }
  }
}
template <int PC, int PF>
static hipError_t transfer_t(bool prolong, const BasisTables &t, const TransferArgs &a, hipStream_t s) {
  using G = XferGeom<PC, PF>;
  if (a.nelem <= 0) return hipSuccess;
  const int ngroups = (a.nelem + G::E - 1) / G::E;
  const dim3 grid(8 * ((ngroups + 7) / 8)), block(64);
  const bool w = a.w_f != nullptr;
  if (prolong) { if (w) hipLaunchKernelGGL((k_transfer<PC, PF, true, true>), grid, block, 0, s, t, a); else hipLaunchKernelGGL((k_transfer<PC, PF, true, false>), grid, block, 0, s, t, a); }
  else { if (w) hipLaunchKernelGGL((k_transfer<PC, PF, false, true>), grid, block, 0, s, t, a); else hipLaunchKernelGGL((k_transfer<PC, PF, false, false>), grid, block, 0, s, t, a); }
  return hipGetLastError();
}
hipError_t launch_transfer(int Pc, int Pf, bool prolong, const BasisTables &t, const TransferArgs &a,
                           hipStream_t s, const char **name) {
#define CPS_TR(C, F)                                                                  \
  if (Pc == C && Pf == F) {                                                           \
    *name = prolong ? "prolong<Pc=" #C ",Pf=" #F ">" : "restrict<Pc=" #C ",Pf=" #F ">"; \
    return transfer_t<C, F>(prolong, t, a, s);                                        \
  }
  // adjacent level pairs of the logarithmic (1,2,4,..,p) and uniform ladders up to p = 7
  CPS_TR(2, 3) CPS_TR(3, 4) CPS_TR(3, 5) CPS_TR(4, 5) CPS_TR(5, 6) CPS_TR(5, 7) CPS_TR(6, 7) CPS_TR(5, 8)
  CPS_TR(7, 8) CPS_TR(2, 4) CPS_TR(2, 5)
  return hipErrorInvalidValue;
}
// w[i] = (local multiplicity, as counted into w by launch_multiplicity) * (scale ? scale[i] : 1); *n_not_unit counts the
// covered entries whose weight is not 1 (to 4 ulp: (1 / m) m rounds to 1 for the multiplicities of a mesh, not for every integer)
__global__ void k_xfer_weights(double *w, const double *scale, size_t n, int *n_not_unit) {
  int bad = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const double m = w[i], v = scale ? m * scale[i] : m;
    w[i] = v;
    if (m != 0. && fabs(v - 1.) > 1e-15) bad = 1;
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicAdd(n_not_unit, 1);
}
hipError_t launch_transfer_weights(double *w, const double *scale, size_t n, int *n_not_unit, hipStream_t s) {
  return launch_stream(k_xfer_weights, n, s, w, scale, n, n_not_unit);
}

}  // namespace cps
