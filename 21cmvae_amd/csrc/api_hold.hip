// api_hold.hip -- the samplers' hold record (include/v21.h: v21_mlp_set_hold): input columns that are no parameters of a
// sampling call but stay at one value each, in the transformed coordinates u in [-1, 1]^in_dim.  The record is the
// counterpart of the prior record (api_prior.hip): it lives in the handle as the HoldArgs (rowmath.h) that the init,
// step and finish kernels of the four samplers take by value, and the launch sites (api_sample.hip, api_ensemble.hip,
// api_nested.hip) pick their HOLD instantiation by m->has_hold.  Nothing else reads it: the fits (fit_map keeps the
// hold mask of its own options), fisher, loglike and loglike_fwd are what they were.  Host bookkeeping only: nothing
// is launched or copied here.
#include "api_internal.h"

extern "C" int v21_mlp_set_hold(v21_mlp* m, const int32_t* hold, const double* u, int32_t in_dim) {
  if (!m) return fail(V21_ERR_ARG, "null mlp");
  if (!hold || in_dim == 0) {
    m->has_hold = false;
    m->hold = HoldArgs{};
    return V21_OK;
  }
  const int din = m->dims[0];
  if (in_dim != din) return fail(V21_ERR_ARG, "hold: %d columns, stack input = %d", (int)in_dim, din);
  if (din > kFitMaxIn) return fail(V21_ERR_ARG, "hold: %d inputs (at most %d)", din, kFitMaxIn);
  // (built beside the handle's: an error leaves the handle as it was)
  HoldArgs h{};
  int held = 0;
  for (int i = 0; i < din; ++i) {
    if (hold[i] != 0 && hold[i] != 1) return fail(V21_ERR_ARG, "hold: hold[%d] = %d (0 free, 1 held)", i, (int)hold[i]);
    if (!hold[i]) continue;
    if (!u) return fail(V21_ERR_ARG, "hold: a held column without u");
    if (!std::isfinite(u[i]) || !(u[i] >= -1.0 && u[i] <= 1.0)) return fail(V21_ERR_ARG, "hold: u[%d] = %g (finite, inside [-1, 1])", i, u[i]);
    h.mask |= 1u << i;
    h.u[i] = (float)u[i];  // (rounded once: this float32 is the column in every state, proposal and stored sample)
    held += 1;
  }
  if (held == din) return fail(V21_ERR_ARG, "hold: every column is held (nothing to sample)");
  m->has_hold = held > 0;
  m->hold = held > 0 ? h : HoldArgs{};
  return V21_OK;
}
