// kernels_dispatch.hip -- the two (P, Q, qf) dispatch tables whose kernels are defined elsewhere: the scalar diagonal's
// instantiations (k_diag_sf, kernel_diag_sf.hpp) and the host-only dispatch over the per-Q objects of the fused kernel.
#include "kernel_diag_sf.hpp"

namespace cps {

// Diagonal of B^T D B (matops.c:227): the instantiations of k_diag_sf (the point-block form defined beside it is
// instantiated by kernels_pointblock.hip).
hipError_t launch_diag(int P, int Q, int qf, const BasisTables &t, const DiagArgs &a, hipStream_t s,
                       const char **name) {
#define CPS_DG(Pv, Qv) CPS_DIAG_CASES(k_diag_sf, "diag", Pv, Qv)
  CPS_DIAG_PQ(CPS_DG)
#undef CPS_DG
  return hipErrorInvalidValue;
}

// Fused-operator dispatch over the per-Q objects (kernels_fused_inst.hip).
#define CPS_DECL_QP(Qv, Pt) hipError_t launch_fused_grad_q##Qv##p##Pt(int, int, const BasisTables &, const FusedGradArgs &, FusedLaunch, hipStream_t, const char **);
CPS_DECL_QP(2, 0) CPS_DECL_QP(3, 0) CPS_DECL_QP(4, 0) CPS_DECL_QP(5, 0) CPS_DECL_QP(6, 0) CPS_DECL_QP(7, 0) CPS_DECL_QP(7, 1)
CPS_DECL_QP(8, 0) CPS_DECL_QP(8, 1) CPS_DECL_QP(8, 2) CPS_DECL_QP(8, 3)
hipError_t launch_fused_grad(int P, int Q, int qf, const BasisTables &t, const FusedGradArgs &a, FusedLaunch l,
                             hipStream_t s, const char **name) {
  static_assert(pencil_inst_parts(7) == 2 && pencil_inst_parts(8) == 4 && pencil_inst_parts(6) == 1, "the objects declared above");
  const int part = (Q >= 2 && Q <= MAXN1D && P <= Q) ? (Q - P) % pencil_inst_parts(Q) : 0;
  switch (Q) {
    case 2: return launch_fused_grad_q2p0(P, qf, t, a, l, s, name);
    case 3: return launch_fused_grad_q3p0(P, qf, t, a, l, s, name);
    case 4: return launch_fused_grad_q4p0(P, qf, t, a, l, s, name);
    case 5: return launch_fused_grad_q5p0(P, qf, t, a, l, s, name);
    case 6: return launch_fused_grad_q6p0(P, qf, t, a, l, s, name);
    case 7: return part == 0 ? launch_fused_grad_q7p0(P, qf, t, a, l, s, name) : launch_fused_grad_q7p1(P, qf, t, a, l, s, name);
    case 8: return part == 0 ? launch_fused_grad_q8p0(P, qf, t, a, l, s, name) : (part == 1 ? launch_fused_grad_q8p1(P, qf, t, a, l, s, name) :
                   (part == 2 ? launch_fused_grad_q8p2(P, qf, t, a, l, s, name) : launch_fused_grad_q8p3(P, qf, t, a, l, s, name)));
  }
  return hipErrorInvalidValue;
}

// The same dispatch over the objects of the entry with the mass term (kernels_fused_inst.hip with -DCPS_MASS; csrc/Makefile FUSEDM_QP).
#define CPS_DECL_MQP(Qv, Pt) hipError_t launch_fused_mass_q##Qv##p##Pt(int, int, const BasisTables &, const FusedGradArgs &, FusedLaunch, hipStream_t, const char **);
CPS_DECL_MQP(2, 0) CPS_DECL_MQP(3, 0) CPS_DECL_MQP(4, 0) CPS_DECL_MQP(5, 0) CPS_DECL_MQP(6, 0) CPS_DECL_MQP(7, 0) CPS_DECL_MQP(7, 1)
hipError_t launch_fused_mass(int P, int Q, int qf, const BasisTables &t, const FusedGradArgs &a, FusedLaunch l,
                             hipStream_t s, const char **name) {
  static_assert(FUSED_MASS_QMAX == 7, "the objects declared above");
  if (!fused_mass_instantiated(P, Q, qf)) return hipErrorInvalidValue;
  switch (Q) {
    case 2: return launch_fused_mass_q2p0(P, qf, t, a, l, s, name);
    case 3: return launch_fused_mass_q3p0(P, qf, t, a, l, s, name);
    case 4: return launch_fused_mass_q4p0(P, qf, t, a, l, s, name);
    case 5: return launch_fused_mass_q5p0(P, qf, t, a, l, s, name);
    case 6: return launch_fused_mass_q6p0(P, qf, t, a, l, s, name);
    case 7: return (Q - P) % pencil_inst_parts(7) == 0 ? launch_fused_mass_q7p0(P, qf, t, a, l, s, name) : launch_fused_mass_q7p1(P, qf, t, a, l, s, name);
  }
  return hipErrorInvalidValue;
}

}  // namespace cps
