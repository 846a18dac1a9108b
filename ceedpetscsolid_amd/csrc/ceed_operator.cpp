// ceed_operator.cpp -- CeedOperator of the MI355X backend: the object, its lowering to a kernel family, the dispatch of an apply.
//
// A CeedOperator is lowered, at its first apply, to one hand-written gfx950 kernel family by matching its field
// signature against the operator graphs the reference builds:
//
//   fused_grad : GRAD active in, NONE qdata (+ NONE state in / out), GRAD active out
//                -> opApply (setuplibceed.c:517-542) and opJacob per level (:817-839)
//                (CeedXOperatorApplyState of a residual-shaped operator: its stored state alone, kernels_state.hip --
//                 also on a basis with more nodes than points, for which no fused kernel exists)
//   setup_geo  : GRAD coords + WEIGHT -> NONE qdata             (:370-389)
//   prolong    : Identity, INTERP in -> NONE out                (:857-862)
//   restrict   : Identity, NONE in  -> INTERP out               (:849-854)
//   coord / energy : forcing, MMS, strain energy, diagnostics   (:555-737)
//   mass       : INTERP active in, NONE qdata, INTERP active out (no call site in the reference: the elastodynamic solve, dynamics.py)
//   stress     : GRAD active in, NONE qdata -> NONE (6, at the points) or INTERP (7, summed at the nodes) (none either: postprocess.py)
//   thermal    : INTERP (1) theta, NONE qdata[, GRAD displacement] -> GRAD active out; its tangent; the stress with theta (thermal.py)
//
// There is NO host fallback: a graph outside these families or a QFunction without a device functor (ceed_qfunction.cpp) is a loud
// error.  The families' applies: ceed_op_fused.cpp (fused_grad, with its diagonals and the state kernel), ceed_op_other.cpp (the rest but the mass operator: ceed_op_mass.cpp).
#include "ceed_operator.hpp"

using namespace cps;

extern "C" int CeedOperatorCreate(Ceed ceed, CeedQFunction qf, CeedQFunction, CeedQFunction, CeedOperator *op) {
  CeedOperator o = new CeedOperator_private;
  o->ceed = ceed; ceed_ref(ceed);
  o->qf = qf; qf->refcount++;
  o->in.resize(qf->in.size()); o->out.resize(qf->out.size());
  *op = o;
  return 0;
}
extern "C" int CeedCompositeOperatorCreate(Ceed ceed, CeedOperator *op) {
  CeedOperator o = new CeedOperator_private;
  o->ceed = ceed; ceed_ref(ceed);
  o->composite = true;
  *op = o;
  return 0;
}
extern "C" int CeedCompositeOperatorAddSub(CeedOperator comp, CeedOperator sub) {
  if (!comp->composite) return ceed_error("not a composite operator");
  comp->sub.push_back(sub); sub->refcount++;
  return 0;
}
extern "C" int CeedOperatorSetField(CeedOperator op, const char *name, CeedElemRestriction r, CeedBasis b, CeedVector v) {
  if (op->composite) return ceed_error("cannot set a field on a composite operator");
  if (op->in.size() != op->qf->in.size()) op->in.resize(op->qf->in.size());
  if (op->out.size() != op->qf->out.size()) op->out.resize(op->qf->out.size());
  OpField *f = nullptr;
  for (size_t i = 0; i < op->qf->in.size() && !f; i++) if (op->qf->in[i].name == name) f = &op->in[i];
  for (size_t i = 0; i < op->qf->out.size() && !f; i++) if (op->qf->out[i].name == name) f = &op->out[i];
  if (!f) return ceed_error("QFunction '%s' has no field named '%s'", op->qf->name.c_str(), name);
  f->set = true; f->rstr = r; f->basis = b; f->vec = v;
  if (r != CEED_ELEMRESTRICTION_NONE) r->refcount++;
  if (b != CEED_BASIS_COLLOCATED) b->refcount++;
  if (v != CEED_VECTOR_ACTIVE && v != CEED_VECTOR_NONE) v->refcount++;
  op->plan = PLAN_NONE;
  return 0;
}
// everything derived from the Dirichlet mask (recorded graphs may still read the arrays: they are DevArrays)
static void op_free_flags(CeedOperator o) {
  o->d_off_flagged.release(); o->d_own_f.release();
  o->row_flags.clear(); o->h_mask.clear(); o->h_mask_fine.clear();
  o->mask_mode = 0;
}
extern "C" int CeedOperatorDestroy(CeedOperator *op) {
  if (!op || !*op) return 0;
  CeedOperator o = *op;
  *op = nullptr;
  if (--o->refcount > 0) return 0;
  if (o->composite) {
    for (CeedOperator s : o->sub) CeedOperatorDestroy(&s);
  } else {
    for (auto *arr : {&o->in, &o->out})
      for (OpField &f : *arr) {
        if (!f.set) continue;
        CeedElemRestrictionDestroy(&f.rstr); CeedBasisDestroy(&f.basis); CeedVectorDestroy(&f.vec);
      }
    CeedQFunctionDestroy(&o->qf);
  }
  CeedVectorDestroy(&o->scale);
  for (auto &ev : o->events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
  Ceed c = o->ceed;
  delete o;            // (before the reference goes: its arrays and its split map retire into a Ceed that still exists)
  ceed_unref(c);
  return 0;
}

void fill_tables(BasisTables &t, CeedBasis b) {
  memset(&t, 0, sizeof t);
  memcpy(t.interp, b->interp1d.data(), sizeof(double) * b->interp1d.size());
  memcpy(t.grad, b->grad1d.data(), sizeof(double) * b->grad1d.size());
  memcpy(t.colo, b->colo1d.data(), sizeof(double) * b->colo1d.size());
  memcpy(t.qw, b->qweight1d.data(), sizeof(double) * b->qweight1d.size());
}
// Even-odd form of one 1-D table (FusedGradArgs::eo).  M(o, m) = TR ? tab[m * LD + o] : tab[o * LD + m], NOUT x NIN,
// expected centro-symmetric (sgn = +1) or centro-antisymmetric (sgn = -1); false if it is not (to 1e-13).
static bool build_eo_table(const double *tab, int NOUT, int NIN, int LD, bool TR, int sgn, double *T) {
  auto M = [&](int o, int m) { return TR ? tab[m * LD + o] : tab[o * LD + m]; };
  double mx = 0.;
  for (int o = 0; o < NOUT; o++) for (int m = 0; m < NIN; m++) mx = std::max(mx, fabs(M(o, m)));
  for (int o = 0; o < NOUT; o++) for (int m = 0; m < NIN; m++)
    if (fabs(M(NOUT - 1 - o, NIN - 1 - m) - sgn * M(o, m)) > 1e-13 * mx) return false;
  const int HIN = NIN / 2, COUT = (NOUT + 1) / 2;
  if (COUT > 4 || HIN > 4 || 2 * COUT * HIN + COUT > 30) return false;   // table must stay within 60 SGPRs
  for (int i = 0; i < EO_TAB; i++) T[i] = 0.;
  for (int r = 0; r < COUT; r++) {
    for (int j = 0; j < HIN; j++) {
      T[r * HIN + j] = 0.5 * (M(r, j) + M(r, NIN - 1 - j));
      T[16 + r * HIN + j] = 0.5 * (M(r, j) - M(r, NIN - 1 - j));
    }
    if (NIN & 1) T[32 + r] = M(r, HIN);
  }
  return true;
}

// The field shapes the families share (the messages stay with the families: each names what it expected).
static int cube(int n) { return n * n * n; }
static bool interlaced3(CeedElemRestriction r) { return is_offsets(r) && r->ncomp == 3 && r->compstride == 1; }
// a displacement field: 3 interlaced components through offsets, on a basis (its element size against P^3 has a message of its own)
static bool is_disp(const OpField &f) { return interlaced3(f.rstr) && f.basis != CEED_BASIS_COLLOCATED; }
static bool nodes_fit(const OpField &f) { return f.rstr->elemsize == cube(f.basis->P1d); }
// qdata / stored state at Q points per direction: strided, 10 / 9 values per point
static bool is_qdata(const OpField &f, int Q) { return is_strided(f.rstr) && f.rstr->ncomp == 10 && f.rstr->elemsize == cube(Q); }
static bool is_state(const OpField &f, int Q) { return is_strided(f.rstr) && f.rstr->ncomp == 9 && f.rstr->elemsize == cube(Q); }
// the coordinates of trilinear elements (setuplibceed.c:279,339)
static bool is_trilinear(const OpField &f) { return is_disp(f) && f.rstr->elemsize == 8 && f.basis->P1d == 2; }

// The temperature field of the thermal loads and of the stress with a thermal term against the displacement field `u` it rides with: the
// rules of rho in MassField (the same nodes and points: the kernel interpolates theta with u's table, compared entry by entry).
static const char *const THETA_COMPONENTS = "theta must be a 1-component field through INTERP: a scalar temperature change per node";
static const char *theta_defect(const OpField &th, const OpField &u) {
  const int P = u.basis->P1d, Q = u.basis->Q1d;
  if (!is_offsets(th.rstr) || th.rstr->ncomp != 1) return "theta must be on an offsets restriction with 1 component";
  if (th.rstr->nelem != u.rstr->nelem) return "theta's restriction must have the element count of u's";
  if (th.rstr->elemsize != cube(P)) return "theta's restriction must have the element size P^3 of u's";
  if (th.basis == CEED_BASIS_COLLOCATED || th.basis->P1d != P || th.basis->Q1d != Q || th.basis->interp1d != u.basis->interp1d)
    return "theta's basis must have u's P, Q and interp table";
  return nullptr;
}

int op_plan(CeedOperator op) {
  if (op->plan != PLAN_NONE) return 0;
  CeedQFunction qf = op->qf;
  for (size_t i = 0; i < qf->in.size(); i++) if (!op->in[i].set) return ceed_error("operator field '%s' not set", qf->in[i].name.c_str());
  for (size_t i = 0; i < qf->out.size(); i++) if (!op->out[i].set) return ceed_error("operator field '%s' not set", qf->out[i].name.c_str());
  op->i_active = op->i_qdata = op->i_state = op->i_weight = op->o_active = op->o_state = op->o_qdata = op->i_rho = op->i_theta = op->i_du = -1;
  const int k = qf->kind;
  auto unsupported = [&](const char *why) {
    return ceed_error("operator with QFunction '%s' is outside the kernel families of /gpu/hip/mi355x: %s", qf->name.c_str(), why);
  };
  if (k == QF_LINELAS || k == QF_HYPERSS_F || k == QF_HYPERSS_DF || k == QF_HYPERFS_F || k == QF_HYPERFS_DF) {
    // inputs: GRAD active (9) | NONE qdata (10) | [NONE state (9)]
    for (size_t i = 0; i < qf->in.size(); i++) {
      const QFField &f = qf->in[i];
      if (f.emode == CEED_EVAL_GRAD && op->in[i].vec == CEED_VECTOR_ACTIVE && f.size == 9 && op->i_active < 0) op->i_active = (int)i;
      else if (f.emode == CEED_EVAL_NONE && f.size == 10 && op->i_qdata < 0) op->i_qdata = (int)i;
      else if (f.emode == CEED_EVAL_NONE && f.size == 9 && op->i_state < 0) op->i_state = (int)i;
      else return unsupported("unexpected input field");
    }
    for (size_t i = 0; i < qf->out.size(); i++) {
      const QFField &f = qf->out[i];
      if (f.emode == CEED_EVAL_GRAD && op->out[i].vec == CEED_VECTOR_ACTIVE && f.size == 9 && op->o_active < 0) op->o_active = (int)i;
      else if (f.emode == CEED_EVAL_NONE && f.size == 9 && op->o_state < 0) op->o_state = (int)i;
      else return unsupported("unexpected output field");
    }
    if (op->i_active != 0 || op->i_qdata != 1) return unsupported("inputs must be (GRAD active, NONE qdata[, NONE state])");
    const bool st_in = (k == QF_HYPERSS_DF || k == QF_HYPERFS_DF), st_out = (k == QF_HYPERSS_F || k == QF_HYPERFS_F);
    if (st_in != (op->i_state >= 0) || st_out != (op->o_state >= 0) || op->o_active != 0)
      return unsupported("stored-state fields do not match the QFunction");
    OpField &ai = op->in[op->i_active], &ao = op->out[op->o_active], &qd = op->in[op->i_qdata];
    if (!is_offsets(ai.rstr) || ai.rstr != ao.rstr || ai.basis != ao.basis || ai.basis == CEED_BASIS_COLLOCATED)
      return unsupported("active input and output must share one offsets restriction and one basis");
    if (!is_disp(ai)) return unsupported("active fields must be 3 interlaced components");
    CeedBasis b = ai.basis;
    const int P = b->P1d, Q = b->Q1d;
    if (!nodes_fit(ai)) return unsupported("restriction element size is not P^3");
    if (!is_qdata(qd, Q) || qd.rstr->nelem != ai.rstr->nelem) return unsupported("qdata must be a strided 10 x Q^3 field");
    if (st_in && !is_state(op->in[op->i_state], Q)) return unsupported("state input must be strided 9 x Q^3");
    if (st_out && !is_state(op->out[op->o_state], Q)) return unsupported("state output must be strided 9 x Q^3");
    fill_tables(op->tables, b);
    if (pencil_even_odd(Q) && P <= Q) {   // even-odd forms of the six products, built once here (not per apply); P > Q: the state kernel only
      const BasisTables &t = op->tables;
      const bool ok = build_eo_table(t.interp, Q, P, P, false, +1, op->eo[0]) && build_eo_table(t.interp, P, Q, P, true, +1, op->eo[1]) &&
                      build_eo_table(t.colo, Q, Q, Q, false, -1, op->eo[2]) && build_eo_table(t.colo, Q, Q, Q, true, -1, op->eo[3]) &&
                      build_eo_table(t.grad, Q, P, P, false, -1, op->eo[4]) && build_eo_table(t.grad, P, Q, P, true, -1, op->eo[5]);
      if (!ok) return unsupported("the basis tables are not centro-symmetric (they are for every CeedBasisCreateTensorH1Lagrange basis)");
    }
    op->plan = PLAN_FUSED_GRAD;
    return 0;
  }
  if (k == QF_SETUP_GEO) {
    if (qf->in.size() != 2 || qf->out.size() != 1) return unsupported("SetupGeo takes (dx, weight) -> qdata");
    if (qf->in[0].emode != CEED_EVAL_GRAD || qf->in[1].emode != CEED_EVAL_WEIGHT || qf->out[0].emode != CEED_EVAL_NONE)
      return unsupported("SetupGeo eval modes must be GRAD, WEIGHT -> NONE");
    OpField &x = op->in[0];
    if (!is_trilinear(x)) return unsupported("coordinates must be trilinear (P=2), 3 interlaced components (setuplibceed.c:279,339)");
    if (!is_qdata(op->out[0], x.basis->Q1d)) return unsupported("qdata must be strided 10 x Q^3");
    op->i_active = 0; op->i_weight = 1; op->o_qdata = 0;
    fill_tables(op->tables, x.basis);
    op->plan = PLAN_SETUP_GEO;
    return 0;
  }
  if (k == QF_IDENTITY) {
    if (qf->identity_size != 3) return unsupported("identity transfer operators carry 3 components");
    OpField &fi = op->in[0], &fo = op->out[0];
    const CeedEvalMode mi = qf->in[0].emode, mo = qf->out[0].emode;
    if (!is_offsets(fi.rstr) || !is_offsets(fo.rstr) || fi.rstr->nelem != fo.rstr->nelem) return unsupported("transfer needs offsets restrictions on both sides");
    if (!interlaced3(fi.rstr) || !interlaced3(fo.rstr)) return unsupported("3 interlaced components expected");
    if (mi == CEED_EVAL_INTERP && mo == CEED_EVAL_NONE && fi.basis != CEED_BASIS_COLLOCATED && fo.basis == CEED_BASIS_COLLOCATED) {
      CeedBasis b = fi.basis;
      if (!nodes_fit(fi) || fo.rstr->elemsize != cube(b->Q1d)) return unsupported("prolongation sizes");
      fill_tables(op->tables, b);
      op->plan = PLAN_PROLONG;
    } else if (mi == CEED_EVAL_NONE && mo == CEED_EVAL_INTERP && fi.basis == CEED_BASIS_COLLOCATED && fo.basis != CEED_BASIS_COLLOCATED) {
      CeedBasis b = fo.basis;
      if (!nodes_fit(fo) || fi.rstr->elemsize != cube(b->Q1d)) return unsupported("restriction sizes");
      fill_tables(op->tables, b);
      op->plan = PLAN_RESTRICT;
    } else return unsupported("identity operator is neither INTERP->NONE nor NONE->INTERP");
    op->i_active = 0; op->o_active = 0;
    return 0;
  }
  const bool energy = k == QF_ENERGY_LINELAS || k == QF_ENERGY_HYPERSS || k == QF_ENERGY_HYPERFS;
  if (energy || k == QF_DIAG_LINELAS || k == QF_DIAG_HYPERSS || k == QF_DIAG_HYPERFS) {
    // opEnergy (setuplibceed.c:651-670): (du GRAD active, qdata NONE) -> energy INTERP, 1 component
    // opDiagnostic (:712-737): (u INTERP, du GRAD, qdata NONE) -> diagnostic NONE, 8 components
    const size_t nin = energy ? 2 : 3;
    if (qf->in.size() != nin || qf->out.size() != 1) return unsupported(energy ? "energy takes (du, qdata) -> energy" : "diagnostic takes (u, du, qdata) -> diagnostic");
    const QFField &fdu = qf->in[nin - 2], &fqd = qf->in[nin - 1], &fo = qf->out[0];
    bool modes = fdu.emode == CEED_EVAL_GRAD && fdu.size == 9 && fqd.emode == CEED_EVAL_NONE && fqd.size == 10;
    if (energy) modes = modes && fo.emode == CEED_EVAL_INTERP && fo.size == 1;
    else modes = qf->in[0].emode == CEED_EVAL_INTERP && qf->in[0].size == 3 && modes && fo.emode == CEED_EVAL_NONE && fo.size == 8;
    if (!modes) return unsupported(energy ? "energy eval modes must be GRAD(9), NONE(10) -> INTERP(1)" : "diagnostic eval modes must be INTERP(3), GRAD(9), NONE(10) -> NONE(8)");
    OpField &u = op->in[0], &du = op->in[nin - 2], &qd = op->in[nin - 1], &o = op->out[0];
    if (!energy && (u.vec != CEED_VECTOR_ACTIVE || du.vec != CEED_VECTOR_ACTIVE || u.rstr != du.rstr || u.basis != du.basis))
      return unsupported("u and du must be the same active field");
    if (!is_disp(u)) return unsupported("displacement field");
    const int P = u.basis->P1d, Q = u.basis->Q1d;
    if (!nodes_fit(u)) return unsupported("restriction element size is not P^3");
    if (!is_qdata(qd, Q) || qd.rstr->nelem != u.rstr->nelem) return unsupported("qdata must be strided 10 x Q^3");
    if (energy) {
      // (the same points: the kernel takes INTERP^T of the energy basis from the displacement basis's table, compared entry by entry)
      if (!is_offsets(o.rstr) || o.rstr->ncomp != 1 || o.rstr->nelem != u.rstr->nelem || o.basis == CEED_BASIS_COLLOCATED ||
          !nodes_fit(o) || o.basis->Q1d != Q || o.basis->P1d != P || o.basis->interp1d != u.basis->interp1d)
        return unsupported("energy field must be a 1-component field on the displacement's nodes and points");
    } else if (!is_offsets(o.rstr) || o.rstr->ncomp != 8 || o.rstr->compstride != 1 || o.rstr->nelem != u.rstr->nelem ||
               o.rstr->elemsize != cube(Q) || o.basis != CEED_BASIS_COLLOCATED)
      return unsupported("diagnostic field must be 8 interlaced components collocated with the points");
    op->i_active = 0; op->i_qdata = (int)nin - 1; op->o_active = 0;
    fill_tables(op->tables, u.basis);
    op->plan = PLAN_ENERGY;
    return 0;
  }
  if (k == QF_CONST_FORCE || k == QF_MMS_FORCE || k == QF_MMS_TRUE) {
    // opSetupForce: (x INTERP, qdata NONE) -> force INTERP (setuplibceed.c:555-583); opTrue: x INTERP -> true_soln NONE (:608-623)
    const bool force = k != QF_MMS_TRUE;
    if (qf->in.size() != (force ? 2u : 1u) || qf->out.size() != 1) return unsupported("expected (x[, qdata]) -> one output");
    if (qf->in[0].emode != CEED_EVAL_INTERP || qf->in[0].size != 3 || qf->out[0].size != 3) return unsupported("x must be 3 components, INTERP");
    OpField &x = op->in[0], &o = op->out[0];
    if (!is_trilinear(x)) return unsupported("coordinates must be trilinear (P=2), 3 interlaced components");
    if (!interlaced3(o.rstr) || o.rstr->nelem != x.rstr->nelem) return unsupported("output must be an offsets restriction with 3 interlaced components");
    const int Q = x.basis->Q1d;
    if (force) {
      if (qf->in[1].emode != CEED_EVAL_NONE || qf->in[1].size != 10 || qf->out[0].emode != CEED_EVAL_INTERP) return unsupported("forcing takes qdata NONE and gives force INTERP");
      if (!is_qdata(op->in[1], Q) || op->in[1].rstr->nelem != x.rstr->nelem) return unsupported("qdata must be strided 10 x Q^3");
      if (o.basis == CEED_BASIS_COLLOCATED || o.basis->Q1d != Q || !nodes_fit(o)) return unsupported("force basis must share the quadrature of the coordinate basis");
      op->i_qdata = 1;
      fill_tables(op->tables, o.basis);
    } else {
      if (qf->out[0].emode != CEED_EVAL_NONE || o.basis != CEED_BASIS_COLLOCATED || o.rstr->elemsize != cube(Q)) return unsupported("true solution is collocated on the points of the coordinate basis");
    }
    op->i_active = 0; op->o_active = 0;
    op->plan = PLAN_COORD;
    return 0;
  }
  if (k == QF_MASS) {
    // (u INTERP active (3), qdata NONE (10)) -> v INTERP active (3): v = c qdata[0] u
    if (qf->in.size() != 2 || qf->out.size() != 1) return unsupported("Mass takes (u, qdata) -> v");
    const QFField &fu = qf->in[0], &fq = qf->in[1], &fv = qf->out[0];
    if (fu.emode != CEED_EVAL_INTERP || fu.size != 3 || fq.emode != CEED_EVAL_NONE || fq.size != 10 || fv.emode != CEED_EVAL_INTERP || fv.size != 3 ||
        op->in[0].vec != CEED_VECTOR_ACTIVE || op->out[0].vec != CEED_VECTOR_ACTIVE)
      return unsupported("Mass eval modes must be INTERP(3) active, NONE(10) -> INTERP(3) active");
    OpField &ai = op->in[0], &ao = op->out[0], &qd = op->in[1];
    if (!is_offsets(ai.rstr) || ai.rstr != ao.rstr || ai.basis != ao.basis || ai.basis == CEED_BASIS_COLLOCATED)
      return unsupported("active input and output must share one offsets restriction and one basis");
    if (!is_disp(ai)) return unsupported("active fields must be 3 interlaced components");
    CeedBasis b = ai.basis;
    const int P = b->P1d, Q = b->Q1d;
    if (!nodes_fit(ai)) return unsupported("restriction element size is not P^3");
    if (!is_qdata(qd, Q) || qd.rstr->nelem != ai.rstr->nelem) return unsupported("qdata must be a strided 10 x Q^3 field");
    if (P > Q) return unsupported("the mass kernel needs P <= Q");
    fill_tables(op->tables, b);
    op->tables_sq = op->tables;
    for (double &v : op->tables_sq.interp) v *= v;
    op->i_active = 0; op->i_qdata = 1; op->o_active = 0;
    op->plan = PLAN_MASS;
    return 0;
  }
  if (k == QF_MASS_FIELD) {
    // (u INTERP active (3), rho INTERP passive (1), qdata NONE (10)) -> v INTERP active (3): v = c rho qdata[0] u.  PLAN_MASS with i_rho set:
    // the mask, the diagonal and the composite treat it as they treat "Mass"
    if (qf->in.size() != 3 || qf->out.size() != 1) return unsupported("MassField takes (u, rho, qdata) -> v");
    const QFField &fu = qf->in[0], &fr = qf->in[1], &fq = qf->in[2], &fv = qf->out[0];
    if (fu.emode != CEED_EVAL_INTERP || fu.size != 3 || fr.emode != CEED_EVAL_INTERP || fr.size != 1 || fq.emode != CEED_EVAL_NONE || fq.size != 10 ||
        fv.emode != CEED_EVAL_INTERP || fv.size != 3 || op->in[0].vec != CEED_VECTOR_ACTIVE || op->out[0].vec != CEED_VECTOR_ACTIVE)
      return unsupported("MassField eval modes must be INTERP(3) active, INTERP(1), NONE(10) -> INTERP(3) active");
    OpField &ai = op->in[0], &ao = op->out[0], &rh = op->in[1], &qd = op->in[2];
    if (!is_passive(rh.vec)) return unsupported("rho must be a passive field with a vector of its own, not the active one");
    if (!is_offsets(ai.rstr) || ai.rstr != ao.rstr || ai.basis != ao.basis || ai.basis == CEED_BASIS_COLLOCATED)
      return unsupported("active input and output must share one offsets restriction and one basis");
    if (!is_disp(ai)) return unsupported("active fields must be 3 interlaced components");
    CeedBasis b = ai.basis;
    const int P = b->P1d, Q = b->Q1d;
    if (!nodes_fit(ai)) return unsupported("restriction element size is not P^3");
    if (!is_qdata(qd, Q) || qd.rstr->nelem != ai.rstr->nelem) return unsupported("qdata must be a strided 10 x Q^3 field");
    if (P > Q) return unsupported("the mass kernel needs P <= Q");
    if (!is_offsets(rh.rstr) || rh.rstr->ncomp != 1) return unsupported("rho must be on an offsets restriction with 1 component");
    if (rh.rstr->nelem != ai.rstr->nelem) return unsupported("rho's restriction must have the element count of u's");
    if (rh.rstr->elemsize != cube(P)) return unsupported("rho's restriction must have the element size P^3 of u's");
    // (the same nodes and points: the kernel interpolates rho with u's table, compared entry by entry)
    if (rh.basis == CEED_BASIS_COLLOCATED || rh.basis->P1d != P || rh.basis->Q1d != Q || rh.basis->interp1d != b->interp1d)
      return unsupported("rho's basis must have u's P, Q and interp table");
    fill_tables(op->tables, b);      // the diagonal squares the table in the kernel: tables_sq is not used
    op->i_active = 0; op->i_rho = 1; op->i_qdata = 2; op->o_active = 0;
    op->plan = PLAN_MASS;
    return 0;
  }
  const bool stress_thermal = k == QF_STRESS_LINELAS_THERMAL || k == QF_STRESS_HYPERSS_THERMAL || k == QF_STRESS_HYPERFS_THERMAL;
  if (k == QF_STRESS_LINELAS || k == QF_STRESS_HYPERSS || k == QF_STRESS_HYPERFS || stress_thermal) {
    // (du GRAD(9) active, qdata NONE(10)) -> stress NONE(6) at the points (strided 6 x Q^3, collocated)
    //                                      | stress INTERP(7) at the nodes (7 interlaced components: w det J {sigma, 1} summed per node)
    // the QFunctions with the thermal term: (du, theta INTERP(1) passive, qdata) -> the same outputs
    const size_t nin = stress_thermal ? 3 : 2;
    if (qf->in.size() != nin || qf->out.size() != 1) return unsupported(stress_thermal ? "stress with the thermal term takes (du, theta, qdata) -> stress" : "stress takes (du, qdata) -> stress");
    const QFField &fdu = qf->in[0], &fqd = qf->in[nin - 1], &fo = qf->out[0];
    const bool points = fo.emode == CEED_EVAL_NONE && fo.size == 6, nodal = fo.emode == CEED_EVAL_INTERP && fo.size == 7;
    if (fdu.emode != CEED_EVAL_GRAD || fdu.size != 9 || fqd.emode != CEED_EVAL_NONE || fqd.size != 10 || !(points || nodal))
      return unsupported("stress eval modes must be GRAD(9), NONE(10) -> NONE(6) at the points or INTERP(7) at the nodes");
    if (stress_thermal && (qf->in[1].emode != CEED_EVAL_INTERP || qf->in[1].size != 1)) return unsupported(THETA_COMPONENTS);
    OpField &u = op->in[0], &qd = op->in[nin - 1], &o = op->out[0];
    if (u.vec != CEED_VECTOR_ACTIVE) return unsupported("du must be the active input of a stress operator");
    if (o.vec != CEED_VECTOR_ACTIVE) return unsupported("stress must be the active output");
    if (!is_disp(u)) return unsupported("displacement field");
    const int P = u.basis->P1d, Q = u.basis->Q1d;
    if (!nodes_fit(u)) return unsupported("restriction element size is not P^3");
    if (!is_qdata(qd, Q) || qd.rstr->nelem != u.rstr->nelem) return unsupported("qdata must be strided 10 x Q^3");
    if (P > Q) return unsupported("the stress kernel needs P <= Q");
    if (points) {
      // (a strided restriction of this backend has one layout, [elem][comp][point]: CeedElemRestrictionCreateStrided takes no other)
      if (!is_strided(o.rstr) || o.rstr->ncomp != 6 || o.rstr->elemsize != cube(Q) || o.rstr->nelem != u.rstr->nelem)
        return unsupported("stress at the points must be a strided 6 x Q^3 field on the displacement's elements");
      if (o.basis != CEED_BASIS_COLLOCATED) return unsupported("stress at the points is collocated: it takes no basis");
    } else {
      if (!is_offsets(o.rstr) || o.rstr->ncomp != 7 || o.rstr->compstride != 1 || o.rstr->nelem != u.rstr->nelem || o.rstr->elemsize != cube(P))
        return unsupported("nodal stress must be an offsets restriction with 7 interlaced components on the displacement's elements and nodes");
      // (the same points: the kernel takes INTERP^T of the stress basis from the displacement basis's table, compared entry by entry)
      if (o.basis == CEED_BASIS_COLLOCATED || o.basis->P1d != P || o.basis->Q1d != Q || o.basis->interp1d != u.basis->interp1d)
        return unsupported("nodal stress basis must have the displacement basis's P, Q and interp table");
    }
    if (stress_thermal) {
      if (!nodes_fit(u)) return unsupported("restriction element size is not P^3");
      if (const char *why = theta_defect(op->in[1], u)) return unsupported(why);
      op->i_theta = 1;
    }
    op->i_active = 0; op->i_qdata = (int)nin - 1; op->o_active = 0;
    fill_tables(op->tables, u.basis);
    op->plan = PLAN_STRESS;
    return 0;
  }
  if (k == QF_THERMAL_FORCE || k == QF_THERMAL_TANGENT) {
    // ThermalForce:   (theta INTERP(1) active, qdata NONE(10)[, du GRAD(9) passive]) -> dv GRAD(9) active
    // ThermalTangent: (ddu GRAD(9) active, du GRAD(9) passive, theta INTERP(1) passive, qdata NONE(10)) -> dv GRAD(9) active
    // theta rides with the displacement field of dv: a scalar restriction of its own on the same elements, the same nodes and points.
    // Which model the context states is read at every apply (apply_thermal), where hyperFS without du and a small-strain tangent are refused.
    const bool tangent = k == QF_THERMAL_TANGENT;
    if (qf->out.size() != 1 || (tangent ? qf->in.size() != 4 : (qf->in.size() != 2 && qf->in.size() != 3)))
      return unsupported(tangent ? "ThermalTangent takes (ddu, du, theta, qdata) -> dv" : "ThermalForce takes (theta, qdata[, du]) -> dv");
    const int it = tangent ? 2 : 0, iq = tangent ? 3 : 1, iu = tangent ? 1 : (qf->in.size() == 3 ? 2 : -1);
    const QFField &ft = qf->in[it], &fq = qf->in[iq], &fv = qf->out[0];
    if (ft.emode != CEED_EVAL_INTERP || ft.size != 1) return unsupported(THETA_COMPONENTS);
    bool modes = fq.emode == CEED_EVAL_NONE && fq.size == 10 && fv.emode == CEED_EVAL_GRAD && fv.size == 9;
    if (iu >= 0) modes = modes && qf->in[iu].emode == CEED_EVAL_GRAD && qf->in[iu].size == 9;
    if (tangent) modes = modes && qf->in[0].emode == CEED_EVAL_GRAD && qf->in[0].size == 9;
    if (!modes) return unsupported(tangent ? "ThermalTangent eval modes must be GRAD(9) active, GRAD(9), INTERP(1), NONE(10) -> GRAD(9) active"
                                           : "ThermalForce eval modes must be INTERP(1) active, NONE(10)[, GRAD(9)] -> GRAD(9) active");
    OpField &th = op->in[it], &qd = op->in[iq], &v = op->out[0];
    if (op->in[0].vec != CEED_VECTOR_ACTIVE || v.vec != CEED_VECTOR_ACTIVE) return unsupported("the first input and dv must be the active fields");
    if (tangent && !is_passive(th.vec)) return unsupported("theta must be a passive field with a vector of its own, not the active one");
    if (iu >= 0 && !is_passive(op->in[iu].vec)) return unsupported("du must be a passive field with a vector of its own, not the active one");
    if (!is_disp(v)) return unsupported("dv must be 3 interlaced components through offsets, on a basis");
    if (!nodes_fit(v)) return unsupported("restriction element size is not P^3");
    if (iu >= 0 && (op->in[iu].rstr != v.rstr || op->in[iu].basis != v.basis)) return unsupported("du must share dv's restriction and basis");
    if (tangent && (op->in[0].rstr != v.rstr || op->in[0].basis != v.basis)) return unsupported("ddu must share dv's restriction and basis");
    const int P = v.basis->P1d, Q = v.basis->Q1d;
    if (!is_qdata(qd, Q) || qd.rstr->nelem != v.rstr->nelem) return unsupported("qdata must be a strided 10 x Q^3 field");
    if (P > Q) return unsupported("the thermal load kernel needs P <= Q");
    if (const char *why = theta_defect(th, v)) return unsupported(why);
    op->i_active = 0; op->i_theta = it; op->i_qdata = iq; op->i_du = iu; op->o_active = 0;
    fill_tables(op->tables, v.basis);
    op->plan = PLAN_THERMAL;
    return 0;
  }
  return unsupported("no kernel family");
}

int need_fused(CeedOperator op, const char *who, Kind kind) {
  if (op->composite) return ceed_error("%s: not provided for composite operators (call it on the sub-operators)", who);
  CHK(op_plan(op));
  if (kind == Kind::any) return 0;
  if (op->plan != PLAN_FUSED_GRAD || (kind != Kind::either && (kind == Kind::residual) != (op->o_state >= 0)))
    return ceed_error("%s is provided for the %s", who, kind == Kind::jacobian ? "Jacobian operators" :
                      (kind == Kind::residual ? "residual operators (the ones that store grad u)" : "residual / Jacobian operators"));
  return 0;
}

// One apply of a non-composite operator: the plan its fields were lowered to (op_plan).
static int op_apply_single(CeedOperator op, CeedVector in, CeedVector out, bool add) {
  CHK(op_plan(op));
  switch (op->plan) {
  case PLAN_FUSED_GRAD: return apply_fused(op, in, out, add);
  case PLAN_SETUP_GEO: return apply_setup_geo(op, in, out);
  case PLAN_PROLONG:
  case PLAN_RESTRICT: return apply_transfer(op, in, out, add);
  case PLAN_ENERGY: return apply_energy(op, in, out, add);
  case PLAN_COORD: return apply_coord(op, in, out, add);
  case PLAN_MASS: return apply_mass(op, in, out, add);
  case PLAN_STRESS: return apply_stress(op, in, out, add);
  case PLAN_THERMAL: return apply_thermal(op, in, out, add);
  default: return ceed_error("operator has no plan");
  }
}

extern "C" int CeedOperatorApplyAdd(CeedOperator op, CeedVector in, CeedVector out, CeedRequest *) {
  if (op->composite) { for (CeedOperator s : op->sub) CHK(op_apply_single(s, in, out, true)); return 0; }
  return op_apply_single(op, in, out, true);
}
extern "C" int CeedOperatorApply(CeedOperator op, CeedVector in, CeedVector out, CeedRequest *rq) {
  if (!op->composite) return op_apply_single(op, in, out, false);
  CHK(CeedVectorSetValue(out, 0.));
  return CeedOperatorApplyAdd(op, in, out, rq);
}

// the instantiation of the last launch; for a fused kernel also how the geometric factors were obtained
extern "C" int CeedXOperatorGetKernelName(CeedOperator op, const char **name) {
  op->kernel_name_full = op->kernel_name;
  if (op->kernel_fused)
    op->kernel_name_full += op->geo_mode == 2 ? " [affine elements: dXdx per element]" : (op->geo_mode == 3 ? " [swept elements: 2 x 2 dXdx recomputed per point]" : (op->geo_mode == 1 ? " [dXdx recomputed per point]" : " [qdata read]"));
  *name = op->kernel_name_full.c_str();
  return 0;
}

static int make_flagged(CeedElemRestriction r, const unsigned char *mask, CeedInt lsize, DevArray<uint32_t> &dev) {
  if (lsize < r->lsize) return ceed_error("Dirichlet mask shorter than the L-vector");
  return dev.upload(r->ceed, flagged_offsets(r->h_offsets, mask, r->ncomp, r->compstride));
}
// mode: 1 = masked entries read as zero, 2 = masked rows dropped, 3 = both (default for mode 0)
extern "C" int CeedXOperatorSetDirichletMaskMode(CeedOperator op, CeedMemType mtype, const unsigned char *mask,
                                                 CeedInt lsize, const unsigned char *mask_out, CeedInt lsize_out, int mode) {
  if (op->composite) return ceed_error("set the mask on the sub-operators");
  CHK(op_plan(op));
  op_free_flags(op);
  if (!mask && !mask_out) return 0;
  if (mtype != CEED_MEM_HOST) return ceed_error("pass the Dirichlet mask in host memory (it is folded into the offsets once)");
  if (op->plan == PLAN_FUSED_GRAD || op->plan == PLAN_MASS) {
    CHK(make_flagged(op->in[op->i_active].rstr, mask, lsize, op->d_off_flagged));
    op->h_mask.assign(mask, mask + lsize);
  } else if (op->plan == PLAN_THERMAL) {     // the mask of the DISPLACEMENT L-vector: dv's restriction (ThermalForce's active input is theta)
    if (!mask) return ceed_error("the thermal load operators take the mask of the displacement vector as the input-side mask");
    CHK(make_flagged(op->out[0].rstr, mask, lsize, op->d_off_flagged));
    op->h_mask.assign(mask, mask + lsize);
  } else if (op->plan == PLAN_PROLONG || op->plan == PLAN_RESTRICT) {
    if (!mask || !mask_out) return ceed_error("transfer operators need the input-side and the output-side mask");
    // the COARSE side's flags ride in its offsets (input of a prolongation, output of a restriction); the FINE side's in the
    // owner map (transfer_owner_map), rebuilt at the next apply
    const bool pro = op->plan == PLAN_PROLONG;
    if (pro) CHK(make_flagged(op->in[0].rstr, mask, lsize, op->d_off_flagged));
    else CHK(make_flagged(op->out[0].rstr, mask_out, lsize_out, op->d_off_flagged));
    CeedElemRestriction rf = pro ? op->out[0].rstr : op->in[0].rstr;
    if ((pro ? lsize_out : lsize) < rf->lsize) return ceed_error("Dirichlet mask shorter than the L-vector");
    const unsigned char *mf = pro ? mask_out : mask;
    op->h_mask_fine.assign(mf, mf + rf->lsize);
  } else return ceed_error("this operator takes no Dirichlet mask");
  op->mask_mode = mode ? mode : 3;
  return 0;
}
extern "C" int CeedXOperatorSetDirichletMask(CeedOperator op, CeedMemType mtype, const unsigned char *mask, CeedInt lsize) {
  return CeedXOperatorSetDirichletMaskMode(op, mtype, mask, lsize, nullptr, 0, 3);
}
extern "C" int CeedXOperatorSetTiming(CeedOperator op, int enable) {
  op->timing = enable != 0;
  for (auto &ev : op->events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
  op->events.clear(); op->ms_accum = 0.; op->launches = 0;
  return 0;
}
extern "C" int CeedXOperatorGetTiming(CeedOperator op, double *ms, int64_t *launches) {
  for (auto &ev : op->events) {
    float t = 0.f;
    HIPCHK(hipEventSynchronize(ev.second));
    HIPCHK(hipEventElapsedTime(&t, ev.first, ev.second));
    op->ms_accum += t;
    (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second);
  }
  op->events.clear();
  *ms = op->ms_accum; *launches = op->launches;
  return 0;
}
extern "C" int CeedXOperatorGetLaunchInfo(CeedOperator op, int out[4]) {
  for (int i = 0; i < 4; i++) out[i] = op->launch_info[i];
  return 0;
}
