// ceed_qfunction.cpp -- CeedQFunction of the MI355X backend: a QFunction is a NAME that selects a device functor (qfunctions_device.hpp);
// the host callback is kept and never called.
#include "ceed_impl.hpp"

using namespace cps;

static int resolve_qf(const std::string &name) {
  static const struct { const char *n; int k; } tab[] = {
      {"SetupGeo", QF_SETUP_GEO},    {"LinElasF", QF_LINELAS},       {"LinElasdF", QF_LINELAS},
      {"HyperSSF", QF_HYPERSS_F},    {"HyperSSdF", QF_HYPERSS_DF},   {"HyperFSF", QF_HYPERFS_F},
      {"HyperFSdF", QF_HYPERFS_DF},  {"SetupConstantForce", QF_CONST_FORCE}, {"SetupMMSForce", QF_MMS_FORCE},
      {"MMSTrueSoln", QF_MMS_TRUE},  {"LinElasEnergy", QF_ENERGY_LINELAS}, {"HyperSSEnergy", QF_ENERGY_HYPERSS},
      {"HyperFSEnergy", QF_ENERGY_HYPERFS}, {"LinElasDiagnostic", QF_DIAG_LINELAS}, {"HyperSSDiagnostic", QF_DIAG_HYPERSS},
      {"HyperFSDiagnostic", QF_DIAG_HYPERFS}, {"Mass", QF_MASS}, {"MassField", QF_MASS_FIELD},
      {"LinElasStress", QF_STRESS_LINELAS}, {"HyperSSStress", QF_STRESS_HYPERSS}, {"HyperFSStress", QF_STRESS_HYPERFS},
      {"ThermalForce", QF_THERMAL_FORCE}, {"ThermalTangent", QF_THERMAL_TANGENT}, {"LinElasStressThermal", QF_STRESS_LINELAS_THERMAL},
      {"HyperSSStressThermal", QF_STRESS_HYPERSS_THERMAL}, {"HyperFSStressThermal", QF_STRESS_HYPERFS_THERMAL},
  };
  for (auto &t : tab) if (name == t.n) return t.k;
  return QF_NONE;
}
extern "C" int CeedQFunctionCreateInterior(Ceed ceed, CeedInt, CeedQFunctionUser f, const char *source,
                                           CeedQFunction *qf) {
  std::string src = source ? source : "";
  const size_t colon = src.rfind(':');
  std::string name = colon == std::string::npos ? src : src.substr(colon + 1);
  const int kind = resolve_qf(name);
  if (kind == QF_NONE)
    return ceed_error("QFunction '%s' has no gfx950 device functor in this backend (host callbacks are "
                      "never executed on /gpu/hip/mi355x)", src.c_str());
  CeedQFunction q = new CeedQFunction_private;
  q->ceed = ceed; ceed_ref(ceed);
  q->f = f; q->source = src; q->name = name; q->kind = kind;
  *qf = q;
  return 0;
}
// does `name` (the part after ':' of a source string, or the whole of it) select a device functor?
extern "C" int CeedXHasQFunction(Ceed, const char *name, int *has) {
  if (!name || !has) return ceed_error("CeedXHasQFunction: name and result required");
  std::string n = name;
  const size_t colon = n.rfind(':');
  *has = resolve_qf(colon == std::string::npos ? n : n.substr(colon + 1)) != QF_NONE ? 1 : 0;
  return 0;
}
extern "C" int CeedQFunctionCreateIdentity(Ceed ceed, CeedInt size, CeedEvalMode inmode, CeedEvalMode outmode,
                                           CeedQFunction *qf) {
  CeedQFunction q = new CeedQFunction_private;
  q->ceed = ceed; ceed_ref(ceed);
  q->name = q->source = "Identity"; q->kind = QF_IDENTITY; q->identity_size = size;
  q->in.push_back({"input", size, inmode});
  q->out.push_back({"output", size, outmode});
  *qf = q;
  return 0;
}
extern "C" int CeedQFunctionAddInput(CeedQFunction qf, const char *name, CeedInt size, CeedEvalMode em) {
  qf->in.push_back({name, size, em});
  return 0;
}
extern "C" int CeedQFunctionAddOutput(CeedQFunction qf, const char *name, CeedInt size, CeedEvalMode em) {
  if (em == CEED_EVAL_WEIGHT) return ceed_error("WEIGHT is not an output mode");
  qf->out.push_back({name, size, em});
  return 0;
}
extern "C" int CeedQFunctionSetContext(CeedQFunction qf, void *ctx, size_t ctxsize) {
  qf->ctx = ctx; qf->ctxsize = ctxsize;  // borrowed; re-read at every apply (matops.c:215-232)
  return 0;
}
extern "C" int CeedQFunctionDestroy(CeedQFunction *qf) {
  if (!qf || !*qf) return 0;
  CeedQFunction q = *qf;
  *qf = nullptr;
  if (q == CEED_QFUNCTION_NONE) return 0;
  if (--q->refcount > 0) return 0;
  ceed_unref(q->ceed);
  delete q;
  return 0;
}
