// ceed_op_other.cpp -- the operator families beside the residual / Jacobian one (op_plan, ceed_operator.cpp): the transfer operators in
// owner form, SetupGeo with the provenance it leaves on the qdata vector, the coordinate-driven and energy operators, and stress recovery.
#include "ceed_operator.hpp"

using namespace cps;

// The transfer operators in OWNER form (kernels_transfer.hip, k_transfer).
// The owner map of the fine side (index_maps.hpp: owner_map), with the fine-side Dirichlet flags.  Set-up time, host; rebuilt when the
// operator's mask changes.
static int transfer_owner_map(CeedOperator op, CeedElemRestriction rf) {
  if (op->d_own_f) return 0;
  Ceed c = op->ceed;
  if (c->capturing) return ceed_error("first apply of a transfer operator during graph capture: apply it once before recording");
  const std::vector<unsigned char> &mk = op->h_mask_fine;
  return op->d_own_f.upload(c, owner_map(rf->h_offsets, rf->lsize, mk.empty() ? nullptr : mk.data(), rf->ncomp, rf->compstride, &op->own_full_cover));
}
// Set-up time only (never while recording): `n` counters on the device, zeroed, counted into by `count` on the Ceed's stream,
// and read back into h[0 .. n).
template <class Count>
static int count_on_device(Ceed c, int n, int *h, Count count) {
  DevArray<int> d_cnt;     // (bound to no Ceed: freed directly on every way out, behind the synchronisation below or an error)
  CHK(d_cnt.alloc(nullptr, (size_t)n));
  HIPCHK(hipMemsetAsync(d_cnt.get(), 0, n * sizeof(int), c->stream));
  CHK(count(d_cnt.get()));
  HIPCHK(hipMemcpyAsync(h, d_cnt.get(), n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
// w = (fine-side scale, CeedXOperatorSetFineScale, or 1) x (local multiplicity of the fine restriction) per fine dof; *w = null
// when every covered entry is 1 (the scale IS 1 / local multiplicity: one rank).  Recomputed when the scale vector was written
// since (CeedVector_private::version) -- with one host read of a counter, so never while recording.
static int transfer_weights(CeedOperator op, CeedElemRestriction rf, const double **w) {
  Ceed c = op->ceed;
  CeedVector sc = op->scale;
  const uint64_t ver = sc ? sc->version : 0;
  if (op->w_ready && op->w_scale == sc && op->w_version == ver) { *w = op->w_unit ? nullptr : op->d_w.get(); return 0; }
  if (c->capturing)
    return ceed_error("transfer operator during graph capture: its fine-side scale was written since the last apply (or this is the first); "
                      "apply the operator once before recording");
  double *psc = nullptr;
  if (sc) CHK(vec_dev(sc, false, &psc));
  const size_t n = (size_t)rf->lsize;
  if (op->d_w.size() < n) CHK(op->d_w.alloc(c, n));
  int cnt = 1;
  CHK(build_csr(rf, rf->csr, nullptr));
  CHK(count_on_device(c, 1, &cnt, [&](int *d_cnt) {
    CHK(dev_zero(c, op->d_w.get(), n));
    HIPCHK(launch_multiplicity(rf->csr.view(), rf->ncomp, rf->compstride, op->d_w.get(), c->stream));
    HIPCHK(launch_transfer_weights(op->d_w.get(), psc, n, d_cnt, c->stream));
    return 0;
  }));
  op->w_unit = cnt == 0; op->w_scale = sc; op->w_version = ver; op->w_ready = true;
  if (op->w_unit) op->d_w.release();     // (not needed again until the scale is rewritten: 8 B per fine dof given back)
  *w = op->w_unit ? nullptr : op->d_w.get();
  return 0;
}
int apply_transfer(CeedOperator op, CeedVector in, CeedVector out, bool add) {
  hipStream_t s = op->ceed->stream;
  const bool pro = op->plan == PLAN_PROLONG;
  CeedElemRestriction rc = pro ? op->in[0].rstr : op->out[0].rstr, rf = pro ? op->out[0].rstr : op->in[0].rstr;
  CeedBasis b = pro ? op->in[0].basis : op->out[0].basis;
  if (in == out) return ceed_error("in-place operator apply is not supported");
  if (in->length < (pro ? rc : rf)->lsize || out->length < (pro ? rf : rc)->lsize) return ceed_error("transfer vector too short");
  TransferArgs a{};
  double *px, *py;
  CHK(vec_dev(in, false, &px));
  CHK(vec_dev(out, true, &py));
  if (op->scale && op->scale->length < rf->lsize) return ceed_error("scale vector too short");
  // OWNER form (kernels_transfer.hip): the fine nodes each element owns, and the weights (null: all 1, the one-rank case)
  CHK(transfer_owner_map(op, rf));
  CHK(transfer_weights(op, rf, &a.w_f));
  // the coarse side's flagged offsets: the input side of a prolongation, the output side of a restriction
  a.off_c = op->d_off_flagged ? op->d_off_flagged.get() : rc->d_offsets.get();
  a.own_f = op->d_own_f.get();
  a.x = px; a.y = py; a.nelem = rc->nelem; a.add = add ? 1 : 0;
  const int m_in = (op->mask_mode & 1) ? 1 : 0, m_out = (op->mask_mode & 2) ? 1 : 0;
  a.mask_c = pro ? m_in : m_out; a.mask_f = pro ? m_out : m_in;
  if (pro) {
    // every fine node is stored by its owner: no E-vector, no sum
    if (!add && !op->own_full_cover) CHK(dev_zero(op->ceed, py, (size_t)out->length));
  } else {
    // deterministic scatter on the COARSE side (Pc^3 nodes per element): element results -> E-vector -> per-node sums in
    // element order over the coarse restriction's transpose map (masked entries travel as zeros)
    CHK(build_csr(rc, rc->csr, nullptr));
    CHK(ceed_need_evec(op->ceed, (size_t)rc->nelem * rc->ncomp * rc->elemsize));
    a.evec = op->ceed->evec.get();
    if (!add && !rc->csr.full_cover) CHK(dev_zero(op->ceed, py, (size_t)out->length));
  }
  TimerScope ts(op, s);
  const char *kname = "";
  hipError_t e = launch_transfer(b->P1d, b->Q1d, pro, op->tables, a, s, &kname);
  if (no_kernel(e, kname)) return ceed_error("no transfer kernel for Pc=%d Pf=%d", b->P1d, b->Q1d);
  HIPCHK(e);
  if (!pro) HIPCHK(launch_assemble(rc->csr.view(), nullptr, a.evec, py, add ? 1 : 0, s));
  set_kernel_name(op, kname, false);
  op->launches++;
  return 0;
}

// SetupGeo, and the coordinate-driven and energy operators.
// Provenance for the fused kernels, kept with the qdata vector SetupGeo just wrote from trilinear elements: the map coefficients,
// and the constant factors of the whole mesh's element class when it has one (affine; else swept along one reference direction).
// Operators reading this vector may then recompute the factors instead of streaming them.  Set-up time only.
static int geo_provenance(CeedOperator op, CeedVector out, const uint32_t *off_x, const double *px, int nelem) {
  Ceed c = op->ceed;
  hipStream_t s = c->stream;
  CeedBasis xb = op->in[0].basis;
  CHK(out->geo.alloc(c, GEO_NCOEF * (size_t)nelem));
  HIPCHK(launch_geo_coeffs(off_x, px, out->geo.get(), nelem, s));
  out->geo_nelem = nelem; out->geo_Q = xb->Q1d;
  if (c->opt.affine_geo) {   // all elements affine (box meshes)?  then dXdx and det J are per-ELEMENT constants
    int cnt = 1;
    CHK(out->geo_aff.alloc(c, GEO_NAFF * (size_t)nelem));
    CHK(count_on_device(c, 1, &cnt, [&](int *d_cnt) { HIPCHK(launch_geo_affine(out->geo.get(), out->geo_aff.get(), nelem, d_cnt, s)); return 0; }));
    if (cnt != 0) out->geo_aff.release();   // a mixed mesh takes the general recompute everywhere
  }
  if (!out->geo_aff && c->opt.swept_geo) {   // every element swept along ONE reference direction (extruded meshes)?
    int cnt[4] = {0, 0, 0, 1};
    CHK(out->geo_swept.alloc(c, GEO_NSWEPT * (size_t)nelem));
    CHK(count_on_device(c, 4, cnt, [&](int *d_cnt) {     // count: every direction an element qualifies for
      HIPCHK(launch_geo_swept(out->geo.get(), out->geo_swept.get(), nelem, d_cnt, -1, s));
      return 0;
    }));
    int axis = -1;
    for (int d = 2; d >= 0; d--) if (cnt[d] == nelem) axis = d;      // a direction ALL elements share
    if (axis < 0) out->geo_swept.release();   // no common direction or general hexes: the general recompute
    else { HIPCHK(launch_geo_swept(out->geo.get(), out->geo_swept.get(), nelem, nullptr, axis, s)); out->geo_axis = axis; }
  }
  for (int i = 0; i < xb->Q1d && i < MAXN1D; i++) { out->geo_qref[i] = xb->qref1d[i]; out->geo_qwt[i] = xb->qweight1d[i]; }
  return 0;
}
int apply_setup_geo(CeedOperator op, CeedVector in, CeedVector out) {
  hipStream_t s = op->ceed->stream;
  OpField &x = op->in[0];
  if (!in || in->length < x.rstr->lsize) return ceed_error("coordinate vector too short");
  SetupGeoArgs a{};
  double *px, *pq;
  CHK(vec_dev(in, false, &px));
  CHK(vec_dev(out, true, &pq));
  a.off_x = x.rstr->d_offsets.get(); a.xcoord = px; a.qdata = pq; a.nelem = x.rstr->nelem;
  if ((size_t)out->length < (size_t)a.nelem * 10 * x.basis->Q1d * x.basis->Q1d * x.basis->Q1d) return ceed_error("qdata vector too short");
  TimerScope ts(op, s);
  const char *kname = "";
  hipError_t e = launch_setup_geo(x.basis->Q1d, op->tables, a, s, &kname);
  if (no_kernel(e, kname)) return ceed_error("no setup_geo kernel for Q=%d", x.basis->Q1d);
  HIPCHK(e);
  op->launches++;
  set_kernel_name(op, kname, false);
  // the elements are trilinear (op_plan takes no other coordinates): keep the map coefficients with the qdata vector
  if (op->ceed->opt.recompute_geo && !op->ceed->capturing) {
    const int ierr = geo_provenance(op, out, a.off_x, px, a.nelem);
    if (ierr) { vec_drop_geo(out); return ierr; }      // no half-built provenance: the vector reads as plain qdata
  }
  return 0;
}
// The element results of an energy / coordinate operator, stored by its kernel in the E-layout of the output restriction `r`, summed into
// `out` per node in element order (k_rstr_transpose).  prepare: the map, the scratch and -- overwrite mode -- zeros wherever the sum
// does not store (entries no element holds, the tail of a longer vector); finish: the sum, after the kernel.
static int cold_sum_prepare(CeedOperator op, CeedElemRestriction r, CeedVector out, double *py, bool add, double **evec) {
  CHK(build_csr(r, r->csr, nullptr));
  CHK(ceed_need_evec(op->ceed, (size_t)r->nelem * r->ncomp * r->elemsize));
  *evec = op->ceed->evec.get();
  if (!add && (!r->csr.full_cover || out->length > r->lsize)) CHK(dev_zero(op->ceed, py, (size_t)out->length));
  return 0;
}
static int cold_sum_finish(CeedOperator op, CeedElemRestriction r, const double *evec, double *py, bool add, const char *kname) {
  HIPCHK(launch_rstr_transpose(r->csr.view(), r->elemsize, r->ncomp, r->compstride, evec, py, add ? 1 : 0, op->ceed->stream));
  set_kernel_name(op, kname, false);
  op->launches++;
  return 0;
}
int apply_energy(CeedOperator op, CeedVector in, CeedVector out, bool add) {
  CeedQFunction qf = op->qf;
  OpField &u = op->in[0], &en = op->out[0];
  if (!in || in->length < u.rstr->lsize || !out || out->length < en.rstr->lsize) return ceed_error("displacement / energy vector too short");
  CeedVector qd = op->in[op->i_qdata].vec;
  if (!is_passive(qd)) return ceed_error("qdata needs a passive vector");
  if ((size_t)qd->length < (size_t)u.rstr->nelem * 10 * u.basis->Q1d * u.basis->Q1d * u.basis->Q1d) return ceed_error("qdata vector too short");
  EnergyOpArgs a{};
  double *pu, *py, *pq;
  CHK(vec_dev(in, false, &pu)); CHK(vec_dev(out, true, &py)); CHK(vec_dev(qd, false, &pq));
  a.off_u = u.rstr->d_offsets.get(); a.u = pu; a.qdata = pq;
  a.nelem = u.rstr->nelem; a.Q = u.basis->Q1d; a.P = u.basis->P1d;
  if (a.Q > MAXN1D || a.P > MAXN1D) return ceed_error("energy operator: Q=%d / P=%d outside the supported range", a.Q, a.P);
  const int kd = qf->kind;
  a.diag = (kd == QF_DIAG_LINELAS || kd == QF_DIAG_HYPERSS || kd == QF_DIAG_HYPERFS) ? 1 : 0;
  a.model = (kd == QF_ENERGY_LINELAS || kd == QF_DIAG_LINELAS) ? 0 : ((kd == QF_ENERGY_HYPERSS || kd == QF_DIAG_HYPERSS) ? 1 : 2);
  double nu, E;
  CHK(read_phys(qf, &nu, &E));
  lame_constants(nu, E, &a.lambda, &a.TwoMu);
  CHK(cold_sum_prepare(op, en.rstr, out, py, add, &a.evec));
  HIPCHK(launch_energy_op(op->tables, a, op->ceed->stream));
  return cold_sum_finish(op, en.rstr, a.evec, py, add,
                         a.diag ? (a.model == 0 ? "diagnostic_op<LinElasDiagnostic>" : (a.model == 1 ? "diagnostic_op<HyperSSDiagnostic>" : "diagnostic_op<HyperFSDiagnostic>"))
                                : (a.model == 0 ? "energy_op<LinElasEnergy>" : (a.model == 1 ? "energy_op<HyperSSEnergy>" : "energy_op<HyperFSEnergy>")));
}
int apply_coord(CeedOperator op, CeedVector in, CeedVector out, bool add) {
  CeedQFunction qf = op->qf;
  OpField &x = op->in[0], &o = op->out[0];
  if (!in || in->length < x.rstr->lsize || !out || out->length < o.rstr->lsize) return ceed_error("coordinate / output vector too short");
  CoordOpArgs a{};
  double *px, *py, *pq = nullptr;
  CHK(vec_dev(in, false, &px)); CHK(vec_dev(out, true, &py));
  a.off_x = x.rstr->d_offsets.get(); a.xcoord = px;
  a.nelem = x.rstr->nelem; a.Q = x.basis->Q1d;
  a.mode = qf->kind == QF_CONST_FORCE ? 0 : (qf->kind == QF_MMS_FORCE ? 1 : 2);
  a.Pout = a.mode == 2 ? a.Q : o.basis->P1d;
  if (a.Q > MAXN1D || a.Pout > MAXN1D) return ceed_error("coordinate operator: Q=%d / P=%d outside the supported range", a.Q, a.Pout);
  if (a.mode != 2) {
    CeedVector qd = op->in[1].vec;
    if (!is_passive(qd)) return ceed_error("qdata needs a passive vector");
    if ((size_t)qd->length < (size_t)a.nelem * 10 * a.Q * a.Q * a.Q) return ceed_error("qdata vector too short");
    CHK(vec_dev(qd, false, &pq)); a.qdata = pq;
    if (!qf->ctx) return ceed_error("QFunction '%s' needs its context", qf->name.c_str());
    const double *cx = (const double *)qf->ctx;   // pointer pass-through: forcing vector (3) or Physics {nu, E} (setuplibceed.c:563-566)
    if (a.mode == 0) for (int i = 0; i < 3; i++) a.ctx[i] = cx[i];
    else lame_constants(cx[0], cx[1], &a.lambda, &a.TwoMu);
  }
  memcpy(a.bx, x.basis->interp1d.data(), sizeof(double) * x.basis->interp1d.size());
  CHK(cold_sum_prepare(op, o.rstr, out, py, add, &a.evec));
  HIPCHK(launch_coord_op(op->tables, a, op->ceed->stream));
  return cold_sum_finish(op, o.rstr, a.evec, py, add,
                         a.mode == 2 ? "coord_op<MMSTrueSoln>" : (a.mode == 1 ? "coord_op<SetupMMSForce>" : "coord_op<SetupConstantForce>"));
}
// Stress recovery (kernels_stress.hip, k_stress; op_plan's PLAN_STRESS).  The displacement is read as it is, boundary values included: the
// restriction's plain offsets, never an operator's flagged ones.  Points: the kernel stores every entry of [nelem][6][Q^3] and nothing else
// (a longer vector keeps its tail; ApplyAdd is refused: nothing is summed).  Nodal: the element results of B^T (w det J {sigma, 1}) go to the
// Ceed's scratch in the E-layout of the 7-component output restriction, whose ordered transpose sums them (cold_sum_prepare / _finish).
// The QFunctions with the thermal term (op->i_theta >= 0) take a passive temperature field beside: the kernel's modes with a field.
int apply_stress(CeedOperator op, CeedVector in, CeedVector out, bool add) {
  CeedQFunction qf = op->qf;
  OpField &u = op->in[0], &o = op->out[0];
  const bool nodal = qf->out[0].emode == CEED_EVAL_INTERP;
  const int P = u.basis->P1d, Q = u.basis->Q1d;
  const size_t npts = (size_t)u.rstr->nelem * Q * Q * Q;
  if (!in || in == CEED_VECTOR_NONE || !out || out == CEED_VECTOR_NONE) return ceed_error("active vectors required");
  if (in == out) return ceed_error("in-place operator apply is not supported");
  if (in->length < u.rstr->lsize) return ceed_error("displacement vector too short");
  if (nodal ? out->length < o.rstr->lsize : (size_t)out->length < 6 * npts)
    return ceed_error("stress vector too short: %lld entries, %lld are written", (long long)out->length, (long long)(nodal ? (size_t)o.rstr->lsize : 6 * npts));
  if (!nodal && add) return ceed_error("the stress at the points is stored, not summed: CeedOperatorApplyAdd is not provided for it");
  CeedVector qd = op->in[op->i_qdata].vec;
  if (!is_passive(qd)) return ceed_error("qdata needs a passive vector");
  if ((size_t)qd->length < 10 * npts) return ceed_error("qdata vector too short");
  StressArgs a{};
  ThermalArgs th{};
  const bool thermal = op->i_theta >= 0;
  double *pu, *py, *pq;
  CHK(read_phys(qf, &a.nu, &a.E));
  lame_constants(a.nu, a.E, &a.lambda, &a.TwoMu);
  a.model = (qf->kind == QF_STRESS_LINELAS || qf->kind == QF_STRESS_LINELAS_THERMAL) ? 0 : ((qf->kind == QF_STRESS_HYPERSS || qf->kind == QF_STRESS_HYPERSS_THERMAL) ? 1 : 2);
  if (thermal) CHK(thermal_field_args(op, op->in[op->i_theta].vec, a.nu, a.E, th));      // (the checks come first: nothing is queued before them)
  CHK(vec_dev(in, false, &pu)); CHK(vec_dev(out, true, &py)); CHK(vec_dev(qd, false, &pq));
  a.offsets = u.rstr->d_offsets.get(); a.x = pu; a.qdata = pq; a.nelem = u.rstr->nelem;
  a.out = py;
  if (nodal) CHK(cold_sum_prepare(op, o.rstr, out, py, add, &a.out));
  TimerScope ts(op, op->ceed->stream);
  const char *kname = "";
  hipError_t e = thermal ? launch_stress_thermal(P, Q, nodal ? THERMAL_MODE_NODAL : THERMAL_MODE_POINTS, op->tables, a, th, op->ceed->stream, &kname)
                         : launch_stress(P, Q, nodal, op->tables, a, op->ceed->stream, &kname);
  if (no_kernel(e, kname)) return ceed_error("no stress kernel instantiated for P=%d Q=%d", P, Q);
  HIPCHK(e);
  if (nodal) return cold_sum_finish(op, o.rstr, a.out, py, add, kname);
  set_kernel_name(op, kname, false);
  op->launches++;
  return 0;
}
// Fine-side multiplicity scale of the transfer operators (matops.c:149,176); NULL clears.
extern "C" int CeedXOperatorSetFineScale(CeedOperator op, CeedVector scale) {
  CeedVectorDestroy(&op->scale);
  op->w_ready = false;
  if (scale && scale != CEED_VECTOR_NONE) { op->scale = scale; scale->refcount++; }
  return 0;
}
