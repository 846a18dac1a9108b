// kernels_fused_inst.hip -- instantiations of the fused operator kernel for one
// quadrature size.  Compiled once per -DCPS_Q=<Q> -DCPS_PART=<k> (see Makefile) so the
// instantiations build in parallel; each object exports launch_fused_grad_q<Q>p<k> and holds
// the kernels with (Q - P) % pencil_inst_parts(Q) == k.
//
// Node counts P per Q follow the level-degree rules of the reference
// (cloptions.c:195-225): the fine level has P = Q (qextra = 0), coarse levels
// use degrees 1, 2, 4 (logarithmic) or every degree below the fine one (uniform) with the FINE quadrature (setuplibceed.c:757).
// Residual kernels (which write the stored state) only exist on the fine level (P = Q, and P = Q - 1, Q - 2 for -qextra 1, 2).
//
// With -DCPS_MASS the object holds the OTHER entry of the same body instead: k_fused_pencil_mass, K + c M (kernel_fused_pencil.hpp), for the
// Jacobian functors of the same (P, Q) set, behind launch_fused_mass_q<Q>p<k> (build/fusedm_q<Q>p<k>.o).
#include "kernel_fused_pencil.hpp"

#ifndef CPS_Q
#error "compile with -DCPS_Q=<points per direction>"
#endif
#ifndef CPS_PART
#define CPS_PART 0
#endif
#ifdef CPS_MASS
#define CPS_WITH_MASS true
#define CPS_NAME_TAIL "+mass>/pencil"
#define CPS_LAUNCH_STEM launch_fused_mass_q
#else
#define CPS_WITH_MASS false
#define CPS_NAME_TAIL ">/pencil"
#define CPS_LAUNCH_STEM launch_fused_grad_q
#endif

namespace cps {

#define CPS_CAT_(a, b) a##b
#define CPS_CAT(a, b) CPS_CAT_(a, b)
#define CPS_STR_(x) #x
#define CPS_STR(x) CPS_STR_(x)

// (Every `if constexpr` below tests the template parameter PART, too: only then is a discarded branch not instantiated -- the kernels
// of the other parts, of P > Q and the derived-state tangent below Q = 6 do not exist in this object.)
#define CPS_CASE(Pv, QFv, QFname)                                                   \
  if constexpr ((CPS_Q - (Pv)) % pencil_inst_parts(CPS_Q) == PART) {                \
    if (P == Pv && qf == QFv) {                                                     \
      *name = "fused_grad<P=" #Pv ",Q=" CPS_STR(CPS_Q) "," QFname CPS_NAME_TAIL;    \
      return launch_fused_pencil_t<Pv, CPS_Q, QFv, CPS_WITH_MASS>(t, a, l, s);      \
    }                                                                               \
  }
// The derived-state tangent is instantiated where it measured a gain: Q >= 6 (one element per wave; -2.6 ... -3.1 % on config 5's
// block, same box); at Q = 5 it removes 9 % of the VALU instructions and 0 % of the time (pencil_derived_state, kernels.hpp).
#define CPS_DERIVED(Pv) \
  if constexpr (PART >= 0 && pencil_derived_state(CPS_Q)) { CPS_CASE(Pv, QF_HYPERFS_DF_DS, "HyperFSdF+derived") }
#define CPS_JACOBIANS(Pv)              \
  CPS_CASE(Pv, QF_LINELAS, "LinElas")  \
  CPS_CASE(Pv, QF_HYPERSS_DF, "HyperSSdF") \
  CPS_CASE(Pv, QF_HYPERFS_DF, "HyperFSdF") \
  CPS_DERIVED(Pv)

// Residual kernels (they write the stored state) run on the FINE level only: P = Q, and P = Q - 1, Q - 2 for -qextra 1, 2
// (src/cloptions.c:53-55: Q = degree + 1 + qextra, setuplibceed.c:252).  A larger qextra is a loud "no fused kernel instantiated".
#ifdef CPS_MASS
#define CPS_RESIDUALS(Pv)     // the mass term belongs to the tangents
#else
#define CPS_RESIDUALS(Pv) CPS_CASE(Pv, QF_HYPERSS_F, "HyperSSF") CPS_CASE(Pv, QF_HYPERFS_F, "HyperFSF")
#endif
#define CPS_FINE_WITH_QEXTRA(Pv) ((CPS_Q) > (Pv) && (CPS_Q) - (Pv) <= 2)
// a coarse degree (or the fine one under -qextra): its Jacobians, and the residuals where it can be the fine level
#define CPS_LEVEL(Pv)                                                                  \
  if constexpr (PART >= 0 && (CPS_Q) > (Pv)) {                                         \
    CPS_JACOBIANS(Pv)                                                                  \
    if constexpr (PART >= 0 && CPS_FINE_WITH_QEXTRA(Pv)) { CPS_RESIDUALS(Pv) }         \
  }

template <int PART>
static hipError_t dispatch_part(int P, int qf, const BasisTables &t, const FusedGradArgs &a, FusedLaunch l, hipStream_t s, const char **name) {
  CPS_JACOBIANS(CPS_Q)
  CPS_RESIDUALS(CPS_Q)
  // (degrees 6 and 7: the uniform ladders, cloptions.c:195-225 -- every degree below the fine one is a level)
  CPS_LEVEL(2) CPS_LEVEL(3) CPS_LEVEL(4) CPS_LEVEL(5) CPS_LEVEL(6) CPS_LEVEL(7)
  return hipErrorInvalidValue;
}

hipError_t CPS_CAT(CPS_CAT(CPS_CAT(CPS_LAUNCH_STEM, CPS_Q), p), CPS_PART)(int P, int qf, const BasisTables &t, const FusedGradArgs &a,
                                                                              FusedLaunch l, hipStream_t s, const char **name) {
  static_assert(CPS_PART >= 0 && CPS_PART < pencil_inst_parts(CPS_Q), "part of this quadrature size");
  return dispatch_part<CPS_PART>(P, qf, t, a, l, s, name);
}

}  // namespace cps
