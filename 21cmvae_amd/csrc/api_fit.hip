// api_fit.hip -- Fisher matrices and batched maximum-likelihood and MAP fits (include/v21.h: v21_mlp_fisher[_dev],
// v21_mlp_fit[_dev], v21_mlp_fit_map[_dev]).  All run the Jacobian kernels of api_jacobian.hip (fused_jac<Arch, Prec> or
// jac_generic_kernel, Jacobian mode) into the likelihood workspace slice by slice, and reduce each slice there with jac_reduce_kernel
// (reduce_run): 4 din^2 (+ 4 (1 + din)) bytes per row leave the workspace.  A fit is a projected
// Levenberg-Marquardt iteration per row in the transformed coordinates u in [-1, 1]^din (fit_lm_kernel); the host
// only launches, and reads one int (the running rows) every check_every iterations.
#include "api_internal.h"
#include "fit_kernels.h"

int call_data_args(const char* what, long long n, bool has_data, long long n_data) {
  if (has_data && (n_data < 1 || n % n_data != 0)) return fail(V21_ERR_ARG, "%s: n = %lld rows, n_data = %lld", what, n, n_data);
  return V21_OK;
}

int call_data(v21_mlp* m, long long n, const float* data, bool on_host, long long n_data, CallData* out) {
  *out = {m->lk_read(), 0, 1};
  if (!data) return V21_OK;
  const int dout = m->dims[m->L];
  if (on_host) {
    CHK(m->fdata.reserve((size_t)n_data * dout));
    HIPCHK(hipMemcpyAsync(m->fdata.p, data, (size_t)n_data * dout * sizeof(float), hipMemcpyHostToDevice, m->ctx->stream));
    data = m->fdata.get();
  }
  CHK(nuis_project(m, data, n_data, &out->d));
  out->ld = dout;
  out->rpd = n / n_data;
  return V21_OK;
}

static v21_fit_opts fit_defaults() {
  v21_fit_opts o;
  o.max_iter = 50;
  o.lambda0 = 1e-3;
  o.xtol = 1e-7;
  o.check_every = 8;
  return o;
}

// the fit of n start rows prepped transformed (their fac is overwritten), then x_hat (x_dtype, pitch in_dim), lnl,
// lnl_start and status (both nullable) and, with d_F, the Fisher matrix at x_hat in raw units: the rows as they are
// handed back, transformed as v21_mlp_fisher transforms them.  Evaluations run on u (no input transform, fac = 1) with
// the caller's output transform.  map: null for the maximum-likelihood fit (fit_lm_kernel<false>, whatever the handle's
// prior record says), else the MAP fit's prior and hold mask (fit_lm_kernel<true>) with its further results mo (device
// pointers, each nullable).
static int fit_run(v21_mlp* m, int route, long long n, const CallData& data, long long row0, const v21_fit_opts& o, int prec, int flags,
                   void* x_hat, int x_dtype, float* d_lnl, float* d_lnl0, int* d_status, float* d_F, const FitMapArgs* map = nullptr,
                   const v21_map_out* mo = nullptr) {
  hipStream_t st = m->ctx->stream;
  const int din = m->dims[0];
  CHK(m->fit.reserve((size_t)n));
  CHK(m->fF.reserve((size_t)n * din * din));
  CHK(m->fl.reserve((size_t)n));
  CHK(m->fg.reserve((size_t)n * din));
  CHK(m->fit_cnt.reserve((size_t)(o.max_iter + 1)));
  FitRow* fs = m->fit.get();
  int* cnt = m->fit_cnt.get();
  float *F = m->fF.get(), *l = m->fl.get(), *g = m->fg.get();
  const dim3 grid((unsigned)((n + 255) / 256));
  HIPCHK(hipMemsetAsync(cnt, 0, (size_t)(o.max_iter + 1) * sizeof(int), st));
  hipLaunchKernelGGL(fit_init_kernel, grid, dim3(256), 0, st, fs, m->jxt.get(), m->jfac.get(), n, din, o.lambda0);
  HIPCHK(hipGetLastError());
  for (int it = 0; it <= o.max_iter; ++it) {
    CHK(reduce_run(m, route, n, F, l, g, nullptr, data.d, data.ld, data.rpd, row0, prec, flags & ~V21_FWD_IN_TRANSFORM));
    if (map)
      hipLaunchKernelGGL((fit_lm_kernel<true, FitMapArgs>), grid, dim3(256), 0, st, fs, m->jxt.get(), (const float*)l, (const float*)g,
                         (const float*)F, n, din, it == 0 ? 1 : 0, o.xtol, cnt + it, *map);
    else
      hipLaunchKernelGGL(fit_lm_kernel<false>, grid, dim3(256), 0, st, fs, m->jxt.get(), (const float*)l, (const float*)g,
                         (const float*)F, n, din, it == 0 ? 1 : 0, o.xtol, cnt + it);
    HIPCHK(hipGetLastError());
    if (it < o.max_iter && (it + 1) % o.check_every == 0) {
      int running = -1;
      HIPCHK(hipMemcpyAsync(&running, cnt + it, sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (running == 0) break;
    }
  }
  if (map) {
    const auto finish = x_dtype == V21_DTYPE_F64 ? fit_map_finish_kernel<double> : fit_map_finish_kernel<float>;
    hipLaunchKernelGGL(finish, grid, dim3(256), 0, st, (const FitRow*)fs, x_hat, d_lnl, d_lnl0, d_status, mo ? mo->lnp : nullptr,
                       mo ? mo->laplace : nullptr, mo ? mo->prec_u : nullptr, n, din, m->tin, *map);
  } else {
    const auto finish = x_dtype == V21_DTYPE_F64 ? fit_finish_kernel<double> : fit_finish_kernel<float>;
    hipLaunchKernelGGL(finish, grid, dim3(256), 0, st, (const FitRow*)fs, x_hat, d_lnl, d_lnl0, d_status, n, din, m->tin);
  }
  HIPCHK(hipGetLastError());
  if (!d_F) return V21_OK;
  CHK(jac_prep(m, x_hat, x_dtype, din, n, 1));
  return reduce_run(m, route, n, d_F, nullptr, nullptr, nullptr, m->lk_read(), 0, 1, 0, prec, flags | V21_FWD_IN_TRANSFORM);
}

static int fit_check(const v21_fit_opts& o) {
  if (o.max_iter < 0 || o.check_every < 1 || !(o.lambda0 > 0.0) || !(o.xtol >= 0.0))
    return fail(V21_ERR_ARG, "fit: options max_iter %d check_every %d lambda0 %g xtol %g", o.max_iter, o.check_every, o.lambda0, o.xtol);
  return V21_OK;
}

// a fit counts once for its iterations, and once more for the Fisher matrix at x_hat when that is asked for (the same
// route: decide_jacobian does not read the input transform)
static int fit_route(v21_mlp* m, int precision, int flags, bool fisher) {
  const int route = jac_route(m, precision, flags, m->dims[m->L]);
  if (fisher) jac_route(m, precision, flags, m->dims[m->L]);
  return route;
}

static constexpr JacEntry kFisher{"Fisher", kJacMaxIn, true, false}, kFit{"fit", kFitMaxIn, true, true},
    kFitMap{"fit_map", kFitMaxIn, true, true};

// ---- Fisher matrices
extern "C" int v21_mlp_fisher_dev(v21_mlp* m, const float* d_x, int64_t ldx, int64_t n, float* d_fisher, float* d_lnl, float* d_grad,
                                  int precision, int flags) {
  CHK(jac_args(m, d_x && d_fisher, n, ldx, kNoPitch, V21_DTYPE_F32, precision, flags, kFisher));
  if (n == 0) return V21_OK;
  CHK(jac_prep(m, d_x, V21_DTYPE_F32, ldx, n, flags & V21_FWD_IN_TRANSFORM));
  return reduce_run(m, jac_route(m, precision, flags, m->dims[m->L]), n, d_fisher, d_lnl, d_grad, nullptr, m->lk_read(), 0, 1, 0, precision,
                    flags);
}

extern "C" int v21_mlp_fisher(v21_mlp* m, const void* x, int x_dtype, int64_t n, float* fisher, float* lnl, float* grad, int precision,
                              int flags) {
  CHK(jac_args(m, x && fisher, n, kNoPitch, kNoPitch, x_dtype, precision, flags, kFisher));
  if (n == 0) return V21_OK;
  const int din = m->dims[0];
  const int route = jac_route(m, precision, flags, m->dims[m->L]);
  ChunkStage sg;
  float *dF, *dl, *dg;
  sg.add(fisher, &dF, (size_t)din * din * sizeof(float));
  sg.add(lnl, &dl, sizeof(float));
  sg.add(grad, &dg, din * sizeof(float));
  return jac_chunks(m, x, x_dtype, n, flags & V21_FWD_IN_TRANSFORM, sg, [&](long long, long long rows) {
    return reduce_run(m, route, rows, dF, dl, dg, nullptr, m->lk_read(), 0, 1, 0, precision, flags);
  });
}

// ---- fits: maximum-likelihood (v21_mlp_fit[_dev]) and MAP (v21_mlp_fit_map[_dev]: the same fit on ln L + ln p with held
// columns, then the Laplace evidence at the accepted point).  Both forms of both share one body each; is_map says which
// entry it serves, and the plain entries launch what they always launched (fit_run without FitMapArgs).
// the MAP options as the kernels take them (NULL: no prior, nothing held); V21_ERR_ARG before any device work
static int fit_map_args(v21_mlp* m, const v21_map_opts* mopts, FitMapArgs* out) {
  *out = FitMapArgs{};
  if (!mopts) return V21_OK;
  if (mopts->use_prior != 0 && mopts->use_prior != 1) return fail(V21_ERR_ARG, "fit_map: use_prior = %d (0 or 1)", mopts->use_prior);
  for (int i = 0; i < kFitMaxIn; ++i) {
    if (mopts->hold[i] != 0 && mopts->hold[i] != 1) return fail(V21_ERR_ARG, "fit_map: hold[%d] = %d (0 or 1)", i, mopts->hold[i]);
    out->hold[i] = mopts->hold[i];
  }
  // (a handle without a record: the uniform prior, its PriorArgs all kind 0)
  out->use_prior = mopts->use_prior;
  if (out->use_prior) out->pr = m->prior;
  return V21_OK;
}

static int fit_dev(v21_mlp* m, const float* d_x0, int64_t ldx, int64_t n, const float* d_data, int64_t n_data, const v21_fit_opts* opts,
                   bool is_map, const v21_map_opts* mopts, float* d_x_hat, float* d_lnl, float* d_lnl_start, float* d_fisher,
                   int32_t* d_status, const v21_map_out* mout, int precision, int flags) {
  const v21_fit_opts o = opts ? *opts : fit_defaults();
  const JacEntry& entry = is_map ? kFitMap : kFit;
  CHK(jac_args(m, d_x0 && d_x_hat && d_lnl, n, ldx, kNoPitch, V21_DTYPE_F32, precision, flags, entry));
  CHK(call_data_args(entry.name, n, d_data != nullptr, n_data));
  CHK(fit_check(o));
  FitMapArgs map;
  if (is_map) CHK(fit_map_args(m, mopts, &map));
  if (n == 0) return V21_OK;
  CallData data;
  CHK(call_data(m, n, d_data, false, n_data, &data));
  const int route = fit_route(m, precision, flags, d_fisher != nullptr);
  CHK(jac_prep(m, d_x0, V21_DTYPE_F32, ldx, n, 1));
  return fit_run(m, route, n, data, 0, o, precision, flags, d_x_hat, V21_DTYPE_F32, d_lnl, d_lnl_start, (int*)d_status, d_fisher,
                 is_map ? &map : nullptr, mout);
}

static int fit_host(v21_mlp* m, const void* x0, int x_dtype, int64_t n, const float* data, int64_t n_data, const v21_fit_opts* opts,
                    bool is_map, const v21_map_opts* mopts, void* x_hat, float* lnl, float* lnl_start, float* fisher, int32_t* status,
                    const v21_map_out* mout, int precision, int flags) {
  const v21_fit_opts o = opts ? *opts : fit_defaults();
  const JacEntry& entry = is_map ? kFitMap : kFit;
  CHK(jac_args(m, x0 && x_hat && lnl, n, kNoPitch, kNoPitch, x_dtype, precision, flags, entry));
  CHK(call_data_args(entry.name, n, data != nullptr, n_data));
  CHK(fit_check(o));
  FitMapArgs map;
  if (is_map) CHK(fit_map_args(m, mopts, &map));
  if (n == 0) return V21_OK;
  CallData cd;
  CHK(call_data(m, n, data, true, n_data, &cd));
  const int din = m->dims[0];
  const int route = fit_route(m, precision, flags, fisher != nullptr);
  ChunkStage sg;
  void* dx;
  float *dF, *dl, *dl0;
  int32_t* ds;
  v21_map_out d{};
  sg.add(fisher, &dF, (size_t)din * din * sizeof(float));
  sg.add(x_hat, &dx, din * (x_dtype == V21_DTYPE_F64 ? sizeof(double) : sizeof(float)));
  sg.add(lnl, &dl, sizeof(float));
  sg.add(lnl_start, &dl0, sizeof(float));
  sg.add(status, &ds, sizeof(int32_t));
  if (is_map && mout) {
    sg.add(mout->lnp, &d.lnp, sizeof(double));
    sg.add(mout->laplace, &d.laplace, sizeof(double));
    sg.add(mout->prec_u, &d.prec_u, (size_t)din * din * sizeof(float));
  }
  return jac_chunks(m, x0, x_dtype, n, 1, sg, [&](long long r0, long long rows) {
    return fit_run(m, route, rows, cd, r0, o, precision, flags, dx, x_dtype, dl, dl0, (int*)ds, dF, is_map ? &map : nullptr, &d);
  });
}

extern "C" int v21_mlp_fit_dev(v21_mlp* m, const float* d_x0, int64_t ldx, int64_t n, const float* d_data, int64_t n_data,
                               const v21_fit_opts* opts, float* d_x_hat, float* d_lnl, float* d_lnl_start, float* d_fisher,
                               int32_t* d_status, int precision, int flags) {
  return fit_dev(m, d_x0, ldx, n, d_data, n_data, opts, false, nullptr, d_x_hat, d_lnl, d_lnl_start, d_fisher, d_status, nullptr, precision,
                 flags);
}

extern "C" int v21_mlp_fit(v21_mlp* m, const void* x0, int x_dtype, int64_t n, const float* data, int64_t n_data, const v21_fit_opts* opts,
                           void* x_hat, float* lnl, float* lnl_start, float* fisher, int32_t* status, int precision, int flags) {
  return fit_host(m, x0, x_dtype, n, data, n_data, opts, false, nullptr, x_hat, lnl, lnl_start, fisher, status, nullptr, precision, flags);
}

extern "C" int v21_mlp_fit_map_dev(v21_mlp* m, const float* d_x0, int64_t ldx, int64_t n, const float* d_data, int64_t n_data,
                                   const v21_fit_opts* opts, const v21_map_opts* mopts, float* d_x_hat, float* d_lnl, float* d_lnl_start,
                                   float* d_fisher, int32_t* d_status, const v21_map_out* mout, int precision, int flags) {
  return fit_dev(m, d_x0, ldx, n, d_data, n_data, opts, true, mopts, d_x_hat, d_lnl, d_lnl_start, d_fisher, d_status, mout, precision, flags);
}

extern "C" int v21_mlp_fit_map(v21_mlp* m, const void* x0, int x_dtype, int64_t n, const float* data, int64_t n_data, const v21_fit_opts* opts,
                               const v21_map_opts* mopts, void* x_hat, float* lnl, float* lnl_start, float* fisher, int32_t* status,
                               const v21_map_out* mout, int precision, int flags) {
  return fit_host(m, x0, x_dtype, n, data, n_data, opts, true, mopts, x_hat, lnl, lnl_start, fisher, status, mout, precision, flags);
}
