// ceed_explicit.cpp -- CeedXVectorLeapfrogStep (kernels_explicit.hip): the explicit time step of dynamics.ExplicitDynamics in one pass.
// Every argument is checked before anything is queued, so a refused call leaves x and vh as they were; the call only queues kernels
// on the Ceed's stream -- no host read, no array made while recording -- so a step can be recorded.
#include "ceed_impl.hpp"

static bool given(CeedVector v) { return v && v != CEED_VECTOR_NONE; }

extern "C" int CeedXVectorLeapfrogStep(CeedVector x, CeedVector vh, CeedVector r, CeedVector f, CeedVector m, double load, double c1,
                                       double c2, double dt, CeedInt n, CeedVector scalars, CeedInt slot) {
  const char *who = "CeedXVectorLeapfrogStep";
  if (!given(x) || !given(vh) || !given(r) || !given(m)) return ceed_error("%s: x, vh, r and m must be vectors", who);
  if (n < 1) return ceed_error("%s: the number of rows n must be at least 1 (n = %d)", who, n);
  const bool has_f = given(f), tally = given(scalars);
  CeedVector ops[5] = {x, vh, r, m, has_f ? f : nullptr};
  const char *names[5] = {"x", "vh", "r", "m", "f"};
  for (int i = 0; i < 5; i++) {
    if (!ops[i]) continue;
    if (ops[i]->length < n) return ceed_error("%s: %s holds %d entries, n = %d are read", who, names[i], ops[i]->length, n);
    for (int j = 0; j < i; j++)
      if (ops[i] == ops[j]) return ceed_error("%s: %s and %s are the same vector: the operands must be pairwise distinct", who, names[j], names[i]);
    if (tally && ops[i] == scalars) return ceed_error("%s: scalars must not be one of the operands (%s)", who, names[i]);
  }
  if (tally && (slot < 0 || slot >= scalars->length)) return ceed_error("%s: scalar %d of %d", who, slot, scalars->length);
  Ceed c = x->ceed;
  if (tally && !c->d_scalar) {   // the per-workgroup partials share the scratch of the dot products (1 + 2048 doubles; one stream)
    if (c->capturing) return ceed_error("%s: take one step with a tally before recording (scratch allocation)", who);
    CHK(c->d_scalar.alloc(nullptr, 1 + 2048));
  }
  double *px, *pv, *pr, *pm, *pf = nullptr, *ps = nullptr;
  CHK(vec_dev(r, false, &pr)); CHK(vec_dev(m, false, &pm));
  if (has_f) CHK(vec_dev(f, false, &pf));
  if (tally) CHK(vec_dev(scalars, true, &ps));
  CHK(vec_dev(vh, true, &pv)); CHK(vec_dev(x, true, &px));
  HIPCHK(cps::launch_leapfrog(px, pv, pr, pf, pm, load, c1, c2, dt, (size_t)n, tally ? c->d_scalar.get() + 1 : nullptr,
                              tally ? ps + slot : nullptr, c->stream));
  return 0;
}
