// api_prior.hip -- the samplers' prior record (include/v21.h: v21_mlp_set_prior): separable in the transformed coordinates
// u in [-1, 1]^in_dim, every column uniform or a truncated normal.  The record is the parameter side's counterpart of the
// nuisance record (api_nuisance.hip): it lives in the handle as the PriorArgs (rowmath.h) that the step kernels of
// the four samplers take by value, and the launch sites (api_sample.hip, api_ensemble.hip, api_nested.hip) pick their
// PRIOR instantiation by m->has_prior.  Host bookkeeping only: nothing is launched or copied here.
#include "api_internal.h"
#include "sample_kernels.h"

extern "C" int v21_mlp_set_prior(v21_mlp* m, const int32_t* kind, const double* mu, const double* sd, int32_t in_dim) {
  if (!m) return fail(V21_ERR_ARG, "null mlp");
  if (!kind || in_dim == 0) {
    m->has_prior = false;
    m->prior = PriorArgs{};
    return V21_OK;
  }
  const int din = m->dims[0];
  if (in_dim != din) return fail(V21_ERR_ARG, "prior: %d columns, stack input = %d", (int)in_dim, din);
  if (din > kFitMaxIn) return fail(V21_ERR_ARG, "prior: %d inputs (at most %d)", din, kFitMaxIn);
  // (built beside the handle's: an error leaves the handle as it was)
  PriorArgs p{};
  bool any = false;
  for (int i = 0; i < din; ++i) {
    if (kind[i] != 0 && kind[i] != 1) return fail(V21_ERR_ARG, "prior: kind[%d] = %d (0 uniform, 1 normal)", i, (int)kind[i]);
    if (!kind[i]) continue;
    if (!mu || !sd) return fail(V21_ERR_ARG, "prior: a normal column without mu or sd");
    if (!std::isfinite(sd[i]) || !(sd[i] >= 1e-3)) return fail(V21_ERR_ARG, "prior: sd[%d] = %g (finite, at least 1e-3)", i, sd[i]);
    if (!std::isfinite(mu[i]) || !(std::fabs(mu[i]) <= 1.0 + 5.0 * sd[i]))
      return fail(V21_ERR_ARG, "prior: mu[%d] = %g (finite, at most 5 sd = %g outside [-1, 1])", i, mu[i], 5.0 * sd[i]);
    p.kind[i] = 1;
    p.mu[i] = mu[i];
    p.w[i] = 1.0 / (sd[i] * sd[i]);
    p.wmu[i] = mu[i] / (sd[i] * sd[i]);
    any = true;
  }
  m->has_prior = any;
  m->prior = any ? p : PriorArgs{};
  return V21_OK;
}
