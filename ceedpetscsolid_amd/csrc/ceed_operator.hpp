// ceed_operator.hpp -- what the operator sources share: ceed_operator.cpp (the object, op_plan, the dispatch), ceed_op_fused.cpp (the
// residual / Jacobian family), ceed_op_other.cpp (transfers, SetupGeo, coordinate and energy operators), ceed_op_mass.cpp (the mass
// operator), ceed_op_thermal.cpp (the thermal loads).  Private, like ceed_impl.hpp.
#pragma once
#include "ceed_impl.hpp"
#include "index_maps.hpp"

// the launches of one apply between two events on its stream, while the operator is timed (CeedXOperatorSetTiming)
struct TimerScope {
  CeedOperator op; hipStream_t s; hipEvent_t a = nullptr, b = nullptr;
  TimerScope(CeedOperator o, hipStream_t st) : op(o), s(st) {
    if (op->timing && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess) (void)hipEventRecord(a, s);
  }
  ~TimerScope() { if (a && b) { (void)hipEventRecord(b, s); op->events.emplace_back(a, b); } }
};

#pragma GCC visibility push(hidden)   // from here on: shared by the objects of the library, exported by none (TimerScope's two symbols were, before these sources were split)
// Match the operator's field signature against the supported kernel families (once: CeedOperatorSetField resets the plan).
int op_plan(CeedOperator op);
// The preamble of an entry point `who`: no composite operator, the plan, and -- but for Kind::any -- an operator of the residual /
// Jacobian family of the kind the entry point is provided for (residual: it stores grad u; Jacobian: it does not).
enum class Kind { any, either, jacobian, residual };
int need_fused(CeedOperator op, const char *who, Kind kind);

// One apply of a planned operator, per family.  Each leaves the name of the kernel it launched on the operator (set_kernel_name).
// apply_fused with `H` (overwrite mode only): the interface sum of the output follows IN ORDER on the same stream.
int apply_fused(CeedOperator op, CeedVector in, CeedVector out, bool add, CeedXHalo H = nullptr);
int apply_transfer(CeedOperator op, CeedVector in, CeedVector out, bool add);
int apply_setup_geo(CeedOperator op, CeedVector in, CeedVector out);
int apply_energy(CeedOperator op, CeedVector in, CeedVector out, bool add);
int apply_coord(CeedOperator op, CeedVector in, CeedVector out, bool add);
int apply_mass(CeedOperator op, CeedVector in, CeedVector out, bool add);
int apply_stress(CeedOperator op, CeedVector in, CeedVector out, bool add);
int apply_thermal(CeedOperator op, CeedVector in, CeedVector out, bool add);
// the temperature field of a thermal load or of a stress with the thermal term: its vector against its restriction, then the kernel's
// arguments (theta, its offsets, beta from the context {nu, E, alpha[, model]})
int thermal_field_args(CeedOperator op, CeedVector theta, double nu, double E, cps::ThermalArgs &th);
// CeedOperatorLinearAssembleDiagonal of a PLAN_MASS operator (overwrites `assembled`; masked rows are zero)
int mass_diagonal(CeedOperator op, CeedVector assembled);
// The Dirichlet flags of the operator's mask in the row order of a transpose map, as an apply hands them to launch_assemble (*flags
// null: no mask, or none on the output side); one cache per operator, filled by an eager apply only (ceed_op_fused.cpp).
int op_row_flags(CeedOperator op, CeedElemRestriction r, const RowMap &M, const unsigned char **flags);

// fused: a launch of the fused kernel, whose name CeedXOperatorGetKernelName completes with how the geometric factors were obtained
static inline void set_kernel_name(CeedOperator op, const char *name, bool fused) { op->kernel_name = name; op->kernel_fused = fused; }
// a dispatch that holds no instantiation for the shape returns hipErrorInvalidValue and leaves the name empty
static inline bool no_kernel(hipError_t e, const char *kname) { return e == hipErrorInvalidValue && !*kname; }
// a vector of its own: neither missing nor one of the two sentinels
static inline bool is_passive(CeedVector v) { return v && v != CEED_VECTOR_NONE && v != CEED_VECTOR_ACTIVE; }
static inline int read_phys(CeedQFunction qf, double *nu, double *E) {
  // The reference passes sizeof(pointer) as the context size at setuplibceed.c:826; the
  // context is the 16-byte {nu, E} struct behind the pointer (elasticity.h:33-36).
  if (!qf->ctx) return ceed_error("QFunction '%s' needs its Physics context", qf->name.c_str());
  const double *p = (const double *)qf->ctx;
  *nu = p[0]; *E = p[1];
  return 0;
}
static inline void lame_constants(double nu, double E, double *lambda, double *TwoMu) {
  // hyperSS.h:79-81 / hyperFS.h:164-167, evaluated once per apply on the host
  *TwoMu = E / (1 + nu);
  const double Kbulk = E / (3 * (1 - 2 * nu));
  *lambda = (3 * Kbulk - *TwoMu) / 3;
}
#pragma GCC visibility pop
