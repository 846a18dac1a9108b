// ceed_op_mass.cpp -- the mass operator family of the MI355X backend (op_plan's PLAN_MASS, ceed_operator.cpp): QFunction "Mass",
// v = c qdata[0] u with u and v through INTERP -- y (+)= c B^T (w det J) B x on three interlaced components -- and its diagonal.
// k_mass (kernels_mass.hip) stores the element results into the Ceed's scratch E-vector; launch_assemble sums them per node in element
// order over the restriction's whole transpose map, under the operator's row flags: no atomics, the same bits every time.
// QFunction "MassField" (op->i_rho >= 0) is the same operator with a density field: v = c rho_h qdata[0] u, rho a passive scalar field
// through INTERP on a restriction of its own -- k_mass's modes with a field, the same sum.
#include "ceed_operator.hpp"

using namespace cps;

// what the apply and the diagonal check and read alike: the qdata vector, the context, the kernel's arguments but for the vectors
static int mass_args(CeedOperator op, MassArgs &a, MassFieldArgs &f) {
  OpField &u = op->in[op->i_active];
  CeedElemRestriction r = u.rstr;
  const int Q = u.basis->Q1d;
  CeedVector qd = op->in[op->i_qdata].vec;
  if (!is_passive(qd)) return ceed_error("qdata needs a passive vector");
  if ((size_t)qd->length < (size_t)r->nelem * 10 * Q * Q * Q) return ceed_error("qdata vector too short");
  if (!op->qf->ctx) return ceed_error("QFunction '%s' needs its context (one double: the coefficient c)", op->qf->name.c_str());
  a.coef = *(const double *)op->qf->ctx;      // borrowed, re-read at every apply; a launch argument, so frozen in a recording
  a.nelem = r->nelem;
  a.offsets = op->d_off_flagged ? op->d_off_flagged.get() : r->d_offsets.get();
  a.mask_in = (op->d_off_flagged && (op->mask_mode & 1)) ? 1 : 0;
  a.mask_out = (op->d_off_flagged && (op->mask_mode & 2)) ? 1 : 0;
  if (op->i_rho >= 0) {
    // rho's address is the launch argument: new values written behind it are seen by a recorded apply
    OpField &rh = op->in[op->i_rho];
    if (!is_passive(rh.vec) || rh.vec->length < rh.rstr->lsize)
      return ceed_error("rho vector shorter than its restriction's L-size: %d entries for %d", is_passive(rh.vec) ? (int)rh.vec->length : 0, (int)rh.rstr->lsize);
    double *pr;
    CHK(vec_dev(rh.vec, false, &pr));
    f.rho = pr;
    f.rho_offsets = rh.rstr->d_offsets.get();
  }
  return 0;
}
// the launch of either QFunction: the kernels with the field take the PLAIN table in both forms
static hipError_t mass_launch(CeedOperator op, bool diag, const MassArgs &a, const MassFieldArgs &f, hipStream_t s, const char **kname) {
  CeedBasis b = op->in[op->i_active].basis;
  if (op->i_rho >= 0) return launch_mass_field(b->P1d, b->Q1d, diag, op->tables, a, f, s, kname);
  return launch_mass(b->P1d, b->Q1d, diag, diag ? op->tables_sq : op->tables, a, s, kname);
}

int apply_mass(CeedOperator op, CeedVector in, CeedVector out, bool add) {
  Ceed c = op->ceed;
  hipStream_t s = c->stream;
  OpField &u = op->in[op->i_active];
  CeedElemRestriction r = u.rstr;
  if (!in || in == CEED_VECTOR_NONE || !out || out == CEED_VECTOR_NONE) return ceed_error("active vectors required");
  if (in->length < r->lsize || out->length < r->lsize) return ceed_error("active vector shorter than the restriction's L-size");
  if (in == out) return ceed_error("in-place operator apply is not supported");
  MassArgs a{};
  MassFieldArgs f{};
  CHK(mass_args(op, a, f));
  double *px, *py, *pq;
  CHK(vec_dev(in, false, &px));
  CHK(vec_dev(out, true, &py));
  CHK(vec_dev(op->in[op->i_qdata].vec, false, &pq));
  a.x = px; a.qdata = pq;
  // the transpose map and the row flags are made by an eager apply: a first apply while a graph is recorded is refused there
  CHK(build_csr(r, r->csr, nullptr));
  const unsigned char *flags = nullptr;
  CHK(op_row_flags(op, r, r->csr, &flags));
  CHK(ceed_need_evec(c, (size_t)r->nelem * 3 * (size_t)r->elemsize));
  a.evec = c->evec.get();
  // overwrite mode: zeros wherever the sum does not store (entries no element holds, the tail of a longer vector); masked rows are
  // stored as zeros by the sum itself, as the Jacobian operators' are.  Add mode touches neither.
  if (!add && (!r->csr.full_cover || out->length > r->lsize)) CHK(dev_zero(c, py, (size_t)out->length));
  TimerScope ts(op, s);
  const char *kname = "";
  hipError_t e = mass_launch(op, false, a, f, s, &kname);
  if (no_kernel(e, kname)) return ceed_error("no mass kernel instantiated for P=%d Q=%d", u.basis->P1d, u.basis->Q1d);
  HIPCHK(e);
  HIPCHK(launch_assemble(r->csr.view(), flags, a.evec, py, add ? 1 : 0, s));
  set_kernel_name(op, kname, false);
  op->launches++;
  return 0;
}

// diag_n = c sum_q B(q, n)^2 wdetJ(q), the same for the three components: the transposed half of k_mass on wdetJ with the squared table
// (op->tables_sq, op_plan).  `assembled` is overwritten; masked rows and entries no element holds are zero.
int mass_diagonal(CeedOperator op, CeedVector assembled) {
  Ceed c = op->ceed;
  hipStream_t s = c->stream;
  OpField &u = op->in[op->i_active];
  CeedElemRestriction r = u.rstr;
  if (!is_passive(assembled) || assembled->length < r->lsize)
    return ceed_error("diagonal vector too short: %d entries for the L-size %d", assembled ? (int)assembled->length : 0, (int)r->lsize);
  MassArgs a{};
  MassFieldArgs f{};
  CHK(mass_args(op, a, f));
  double *pd, *pq;
  CHK(vec_dev(assembled, true, &pd));
  CHK(vec_dev(op->in[op->i_qdata].vec, false, &pq));
  a.qdata = pq;
  CHK(build_csr(r, r->csr, nullptr));
  CHK(ceed_need_evec(c, (size_t)r->nelem * 3 * (size_t)r->elemsize));
  a.evec = c->evec.get();
  CHK(dev_zero(c, pd, (size_t)assembled->length));
  const char *kname = "";
  hipError_t e = mass_launch(op, true, a, f, s, &kname);
  if (no_kernel(e, kname)) return ceed_error("no mass diagonal kernel instantiated for P=%d Q=%d", u.basis->P1d, u.basis->Q1d);
  HIPCHK(e);
  HIPCHK(launch_assemble(r->csr.view(), nullptr, a.evec, pd, 0, s));
  set_kernel_name(op, kname, false);
  return 0;
}
