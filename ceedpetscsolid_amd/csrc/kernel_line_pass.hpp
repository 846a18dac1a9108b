// kernel_line_pass.hpp -- the LINE-PER-LANE tensor passes that k_mass (kernels_mass.hip) and k_stress (kernels_stress.hip) share.
//
// The slab of an element is one array [c][Q][Q][QP] in LDS, QP = Q | 1 (an odd row pitch: the lanes of the x passes, QP doubles apart,
// then fall on different banks).  Every pass is IN PLACE: a lane reads the P (or Q) entries of its line into registers, multiplies by
// the 1-D table and writes Q (or P) entries back into the same line, which no other lane touches in that pass (Q >= P: the longer line
// always fits); a barrier separates the passes.
// Packing: an element owns TPE = 3 Q^2 rounded up to a power of two lanes (16, 32, 64, 128, 128, 256, 256 for Q = 2 .. 8), a workgroup of
// 256 lanes EPB = 256 / TPE elements (16, 8, 4, 2, 2, 1, 1), so that no wave idles on a handful of lines.
#pragma once
#include "kernels_common.hpp"

namespace cps {

template <int Q> struct MassGeom {
  static constexpr int QP = Q | 1, LINES = 3 * Q * Q;
  static constexpr int TPE = next_pow2(LINES) > 256 ? 256 : next_pow2(LINES), EPB = 256 / TPE;
  static constexpr int NE = 3 * Q * Q * QP;      // doubles per element
  static_assert(TPE >= LINES, "a lane per line in the fullest stage");
  static_assert(sizeof(double) * ((size_t)EPB * NE + MAXN1D * MAXN1D) <= 64 * 1024, "static LDS");
};

// One line, in place: in[i] = s[i * stride], i < NIN;  s[o * stride] = sum_i M(o, i) in[i], o < NOUT.
// sB is B[q][p] (Q x P row-major).  Forward (P -> Q): M(o, i) = B[o][i];  transposed (Q -> P): M(o, i) = B[i][o].
template <int P, int Q, bool TR> CPS_DEV void mass_line(double *s, int stride, const double *sB) {
  constexpr int NIN = TR ? Q : P, NOUT = TR ? P : Q;
  double in[NIN];
#pragma unroll
  for (int i = 0; i < NIN; i++) in[i] = s[i * stride];
#pragma unroll
  for (int o = 0; o < NOUT; o++) {
    double v = 0.;
#pragma unroll
    for (int i = 0; i < NIN; i++) v += (TR ? sB[i * P + o] : sB[o * P + i]) * in[i];
    s[o * stride] = v;
  }
}

}  // namespace cps
