// ceed_op_thermal.cpp -- the thermal loads of the MI355X backend (op_plan's PLAN_THERMAL, ceed_operator.cpp): QFunction "ThermalForce",
// the residual of the coupling energy of a nodal temperature change theta with the strain,
//   y (+)= B_grad^T [ -beta theta_h wdetJ dXdx F^-T ],   beta = E alpha / (1 - 2 nu),   F = I (linElas, hyperSS) | I + grad u (hyperFS),
// and "ThermalTangent", its derivative in the finite-strain model, +beta theta_h F^-T (grad du)^T F^-T.  The context is {nu, E, alpha, model}
// (model 0 linElas, 1 hyperSS, 2 hyperFS), borrowed and read at every apply.  k_stress's modes with a field (kernels_stress.hip) store the
// element results into the Ceed's scratch E-vector; launch_assemble sums them per node in element order over the whole transpose map of
// the displacement restriction, under the operator's row flags: no atomics, the same bits every time.
// thermal_field_args is shared with the stress operators that carry the thermal term (apply_stress, ceed_op_other.cpp).
#include "ceed_operator.hpp"

using namespace cps;

// pure: E alpha / (1 - 2 nu) = 3 K alpha
static double thermal_beta(double nu, double E, double alpha) { return E * alpha / (1 - 2 * nu); }

int thermal_field_args(CeedOperator op, CeedVector theta, double nu, double E, ThermalArgs &th) {
  CeedQFunction qf = op->qf;
  OpField &f = op->in[op->i_theta];
  if (!qf->ctx || qf->ctxsize < 3 * sizeof(double))
    return ceed_error("QFunction '%s' needs its context {nu, E, alpha%s}", qf->name.c_str(), op->plan == PLAN_THERMAL ? ", model" : "");
  // theta's address is the launch argument: new values written behind it are seen by a recorded apply
  if (!is_passive(theta) || theta->length < f.rstr->lsize)
    return ceed_error("theta vector shorter than its restriction's L-size: %d entries for %d", is_passive(theta) ? (int)theta->length : 0, (int)f.rstr->lsize);
  double *pt;
  CHK(vec_dev(theta, false, &pt));
  th.theta = pt;
  th.theta_offsets = f.rstr->d_offsets.get();
  th.beta = thermal_beta(nu, E, ((const double *)qf->ctx)[2]);
  return 0;
}

int apply_thermal(CeedOperator op, CeedVector in, CeedVector out, bool add) {
  Ceed c = op->ceed;
  hipStream_t s = c->stream;
  CeedQFunction qf = op->qf;
  const bool tangent = qf->kind == QF_THERMAL_TANGENT;
  OpField &v = op->out[0];
  CeedElemRestriction r = v.rstr;
  const int P = v.basis->P1d, Q = v.basis->Q1d;
  if (!in || in == CEED_VECTOR_NONE || !out || out == CEED_VECTOR_NONE) return ceed_error("active vectors required");
  if (in == out) return ceed_error("in-place operator apply is not supported");
  if (out->length < r->lsize || (tangent && in->length < r->lsize)) return ceed_error("active vector shorter than the restriction's L-size");
  if (!qf->ctx || qf->ctxsize < 4 * sizeof(double)) return ceed_error("QFunction '%s' needs its context {nu, E, alpha, model}", qf->name.c_str());
  const double *ctx = (const double *)qf->ctx;
  StressArgs a{};
  ThermalArgs th{};
  a.nu = ctx[0]; a.E = ctx[1];
  if (ctx[3] != 0. && ctx[3] != 1. && ctx[3] != 2.) return ceed_error("QFunction '%s': the model in the context must be 0 (linElas), 1 (hyperSS) or 2 (hyperFS)", qf->name.c_str());
  a.model = (int)ctx[3];
  if (tangent && a.model != 2)
    return ceed_error("ThermalTangent is the tangent of the finite-strain model alone (model 2): the small-strain thermal load is dead and has none");
  if (a.model == 2 && op->i_du < 0) return ceed_error("ThermalForce with the finite-strain model (model 2) needs the displacement field du");
  lame_constants(a.nu, a.E, &a.lambda, &a.TwoMu);
  CeedVector qd = op->in[op->i_qdata].vec;
  if (!is_passive(qd)) return ceed_error("qdata needs a passive vector");
  if ((size_t)qd->length < (size_t)r->nelem * 10 * Q * Q * Q) return ceed_error("qdata vector too short");
  CeedVector u = op->i_du >= 0 ? op->in[op->i_du].vec : nullptr;
  if (u && (!is_passive(u) || u->length < r->lsize)) return ceed_error("du vector shorter than the restriction's L-size");
  if (u == out || (tangent && u == in)) return ceed_error("in-place operator apply is not supported");
  CHK(thermal_field_args(op, tangent ? op->in[op->i_theta].vec : in, a.nu, a.E, th));
  double *px = nullptr, *py, *pq, *pu = nullptr;
  if (tangent) CHK(vec_dev(in, false, &px));
  if (u && a.model == 2) CHK(vec_dev(u, false, &pu));
  CHK(vec_dev(out, true, &py));
  CHK(vec_dev(qd, false, &pq));
  a.offsets = op->d_off_flagged ? op->d_off_flagged.get() : r->d_offsets.get();
  a.x = pu; a.qdata = pq; a.nelem = r->nelem;
  th.dx = px;
  th.mask_in = (op->d_off_flagged && (op->mask_mode & 1)) ? 1 : 0;
  th.mask_out = (op->d_off_flagged && (op->mask_mode & 2)) ? 1 : 0;
  // the transpose map and the row flags are made by an eager apply: a first apply while a graph is recorded is refused there
  CHK(build_csr(r, r->csr, nullptr));
  const unsigned char *flags = nullptr;
  CHK(op_row_flags(op, r, r->csr, &flags));
  CHK(ceed_need_evec(c, (size_t)r->nelem * 3 * (size_t)r->elemsize));
  a.out = c->evec.get();
  // overwrite mode: zeros wherever the sum does not store (entries no element holds, the tail of a longer vector); masked rows are
  // stored as zeros by the sum itself.  Add mode touches neither.
  if (!add && (!r->csr.full_cover || out->length > r->lsize)) CHK(dev_zero(c, py, (size_t)out->length));
  TimerScope ts(op, s);
  const char *kname = "";
  hipError_t e = launch_stress_thermal(P, Q, tangent ? THERMAL_MODE_TANGENT : THERMAL_MODE_FORCE, op->tables, a, th, s, &kname);
  if (no_kernel(e, kname)) return ceed_error("no thermal load kernel instantiated for P=%d Q=%d", P, Q);
  HIPCHK(e);
  HIPCHK(launch_assemble(r->csr.view(), flags, a.out, py, add ? 1 : 0, s));
  set_kernel_name(op, kname, false);
  op->launches++;
  return 0;
}
