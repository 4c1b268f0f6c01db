// api_fit.hip -- Fisher matrices and batched maximum-likelihood fits (include/v21.h: v21_mlp_fisher[_dev],
// v21_mlp_fit[_dev]).  Both run the Jacobian kernels of api_jacobian.hip (fused_jac<Arch, Prec> or jac_generic_kernel,
// Jacobian mode) into the likelihood workspace slice by slice, and reduce each slice there with jac_fisher_kernel
// (fit_kernels.h): 4 din^2 (+ 4 (1 + din)) bytes per row leave the workspace.  A fit is a projected
// Levenberg-Marquardt iteration per row in the transformed coordinates u in [-1, 1]^din (fit_lm_kernel); the host
// only launches, and reads one int (the running rows) every check_every iterations.
#include "api_internal.h"
#include "fit_kernels.h"

// F (n, din, din), and lnl / grad (nullable) of n rows (xt, fac) on `route`; row n of the call reads data row
// (row0 + n) / rpd of pitch ld_data
static int fisher_launch(v21_mlp* m, int route, const float* xt, const float* fac, long long n, float* d_F, float* d_lnl,
                         float* d_grad, const float* d_data, long long ld_data, long long rpd, long long row0, int prec, int flags) {
  hipStream_t st = m->ctx->stream;
  const int din = m->dims[0], dout = m->dims[m->L];
  const long long rows_ws = std::min(n, kLkSlice);
  CHK(lk_ws_reserve(m, rows_ws));
  const bool like = d_lnl || d_grad;
  float* wy = m->d_lk_ws;
  float* wj = m->d_lk_ws + rows_ws * dout;
  for (long long r0 = 0; r0 < n; r0 += kLkSlice) {
    const long long rows = std::min(kLkSlice, n - r0);
    CHK(jac_eval_rows(m, route, xt + r0 * din, fac + r0 * din, rows, like ? wy : nullptr, wj, prec, flags));
    const dim3 grid((unsigned)((rows + 3) / 4));
    auto kern = din <= kFitMaxIn ? jac_fisher_kernel<kFitMaxIn> : jac_fisher_kernel<kFisherMaxIn>;
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, (const float*)wy, (const float*)wj, d_data, ld_data, rpd, row0 + r0,
                       (const float*)m->d_lk_w, d_F + r0 * din * din, d_lnl ? d_lnl + r0 : nullptr, d_grad ? d_grad + r0 * din : nullptr,
                       rows, din, dout);
    HIPCHK(hipGetLastError());
  }
  return V21_OK;
}

static int fisher_route(v21_mlp* m, int flags) {
  const int route = decide_jacobian(m->fused_id >= 0, m->dims[0], flags, m->dims[m->L]);
  m->last_jac_route = route;
  m->jac_route_count[route] += 1;
  return route;
}

// the fit state and the evaluation's results for `rows` rows, the per-iteration counts for `iters` iterations
static int fit_reserve(v21_mlp* m, long long rows, int iters) {
  const int din = m->dims[0];
  if (m->fit_rows < rows) {
    for (float** p : {&m->d_fF, &m->d_fl, &m->d_fg}) if (*p) { HIPCHK(hipFree(*p)); *p = nullptr; }
    if (m->d_fit) { HIPCHK(hipFree(m->d_fit)); m->d_fit = nullptr; }
    m->fit_rows = 0;
    HIPCHK(hipMalloc(&m->d_fit, (size_t)rows * sizeof(FitRow)));
    HIPCHK(hipMalloc((void**)&m->d_fF, (size_t)rows * din * din * sizeof(float)));
    HIPCHK(hipMalloc((void**)&m->d_fl, (size_t)rows * sizeof(float)));
    HIPCHK(hipMalloc((void**)&m->d_fg, (size_t)rows * din * sizeof(float)));
    m->fit_rows = rows;
  }
  if (m->fit_cnt_cap < iters) {
    if (m->d_fit_cnt) { HIPCHK(hipFree(m->d_fit_cnt)); m->d_fit_cnt = nullptr; }
    m->fit_cnt_cap = 0;
    HIPCHK(hipMalloc((void**)&m->d_fit_cnt, (size_t)iters * sizeof(int)));
    m->fit_cnt_cap = iters;
  }
  return V21_OK;
}

// the host API's result staging: F, ln L, ln L at the start, gradient / status of one chunk
static int fit_out_reserve(v21_mlp* m, long long rows) {
  const int din = m->dims[0];
  if (m->fout_rows >= rows) return V21_OK;
  if (m->d_fout) { HIPCHK(hipFree(m->d_fout)); m->d_fout = nullptr; }
  m->fout_rows = 0;
  HIPCHK(hipMalloc((void**)&m->d_fout, (size_t)rows * (din * din + din + 3) * sizeof(float)));
  m->fout_rows = rows;
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

// the fit of `rows` start rows staged transformed in m->d_jxt (their fac in m->d_jfac is overwritten): the state ends
// in m->d_fit.  Evaluations run on u (no input transform, fac = 1) with the caller's output transform.
static int fit_core(v21_mlp* m, int route, long long rows, const float* d_data, long long ld_data, long long rpd, long long row0,
                    const v21_fit_opts& o, int prec, int flags) {
  hipStream_t st = m->ctx->stream;
  const int din = m->dims[0];
  CHK(fit_reserve(m, rows, o.max_iter + 1));
  FitRow* fs = (FitRow*)m->d_fit;
  const dim3 grid((unsigned)((rows + 255) / 256));
  HIPCHK(hipMemsetAsync(m->d_fit_cnt, 0, (size_t)(o.max_iter + 1) * sizeof(int), st));
  hipLaunchKernelGGL(fit_init_kernel, grid, dim3(256), 0, st, fs, m->d_jxt, m->d_jfac, rows, din, o.lambda0);
  HIPCHK(hipGetLastError());
  const int fu = flags & ~V21_FWD_IN_TRANSFORM;
  for (int it = 0; it <= o.max_iter; ++it) {
    CHK(fisher_launch(m, route, m->d_jxt, m->d_jfac, rows, m->d_fF, m->d_fl, m->d_fg, d_data, ld_data, rpd, row0, prec, fu));
    hipLaunchKernelGGL(fit_lm_kernel, grid, dim3(256), 0, st, fs, m->d_jxt, (const float*)m->d_fl, (const float*)m->d_fg,
                       (const float*)m->d_fF, rows, din, it == 0 ? 1 : 0, o.xtol, m->d_fit_cnt + it);
    HIPCHK(hipGetLastError());
    if (it < o.max_iter && (it + 1) % o.check_every == 0) {
      int running = -1;
      HIPCHK(hipMemcpyAsync(&running, m->d_fit_cnt + it, sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (running == 0) break;
    }
  }
  return V21_OK;
}

// has_data: a data matrix of n_data rows was handed in (at least one, dividing n); without one n_data is ignored
static int fit_check(v21_mlp* m, int precision, int flags, long long n, bool has_data, long long n_data, const v21_fit_opts& o) {
  if (m->dims[0] > kFitMaxIn) return fail(V21_ERR_UNSUPPORTED, "fit: %d inputs (at most %d)", m->dims[0], kFitMaxIn);
  if (!m->has_tin) return fail(V21_ERR_STATE, "fit: no input transform (v21_mlp_set_input_transform): it defines the box");
  CHK(jac_check(m, precision, flags & ~V21_FWD_IN_TRANSFORM, true));
  if (has_data && (n_data < 1 || n % n_data != 0)) return fail(V21_ERR_ARG, "fit: n = %lld rows, n_data = %lld", n, n_data);
  if (o.max_iter < 0 || o.check_every < 1 || !(o.lambda0 > 0.0) || !(o.xtol >= 0.0))
    return fail(V21_ERR_ARG, "fit: options max_iter %d check_every %d lambda0 %g xtol %g", o.max_iter, o.check_every, o.lambda0, o.xtol);
  return V21_OK;
}

// ---- Fisher matrices
extern "C" int v21_mlp_fisher_dev(v21_mlp* m, const float* d_x, int64_t ldx, int64_t n, float* d_fisher, float* d_lnl, float* d_grad,
                                  int precision, int flags) {
  if (!m || !d_x || !d_fisher) return fail(V21_ERR_ARG, "null argument");
  if (n < 0 || ldx < m->dims[0]) return fail(V21_ERR_ARG, "bad shape: n=%lld ldx=%lld", (long long)n, (long long)ldx);
  if (m->dims[0] > kFisherMaxIn) return fail(V21_ERR_UNSUPPORTED, "Fisher: %d inputs (at most %d)", m->dims[0], kFisherMaxIn);
  flags &= 0xFF;
  if (n == 0) return V21_OK;
  CHK(use(m->ctx));
  CHK(jac_check(m, precision, flags, true));
  CHK(jac_stage(m, n));
  CHK(jac_prep_rows(m, d_x, V21_DTYPE_F32, ldx, n, (flags & V21_FWD_IN_TRANSFORM) ? 1 : 0));
  return fisher_launch(m, fisher_route(m, flags), m->d_jxt, m->d_jfac, n, d_fisher, d_lnl, d_grad, m->d_lk_data, 0, 1, 0, precision, flags);
}

// host rows (float32 / float64) -> transformed rows and factors in m->d_jxt / d_jfac, through the staging m->d_jx64
static int stage_rows(v21_mlp* m, const void* x, int x_dtype, long long r0, long long rows, int tin) {
  const size_t esz = x_dtype == V21_DTYPE_F64 ? sizeof(double) : sizeof(float);
  const int din = m->dims[0];
  HIPCHK(hipMemcpyAsync(m->d_jx64, (const char*)x + r0 * din * esz, (size_t)rows * din * esz, hipMemcpyHostToDevice, m->ctx->stream));
  return jac_prep_rows(m, m->d_jx64, x_dtype, din, rows, tin);
}

extern "C" int v21_mlp_fisher(v21_mlp* m, const void* x, int x_dtype, int64_t n, float* fisher, float* lnl, float* grad, int precision,
                              int flags) {
  if (!m || !x || !fisher) return fail(V21_ERR_ARG, "null argument");
  if (n < 0) return fail(V21_ERR_ARG, "negative row count");
  if (x_dtype != V21_DTYPE_F32 && x_dtype != V21_DTYPE_F64) return fail(V21_ERR_ARG, "x_dtype %d unknown", x_dtype);
  if (m->dims[0] > kFisherMaxIn) return fail(V21_ERR_UNSUPPORTED, "Fisher: %d inputs (at most %d)", m->dims[0], kFisherMaxIn);
  flags &= 0xFF;
  if (n == 0) return V21_OK;
  CHK(use(m->ctx));
  CHK(jac_check(m, precision, flags, true));
  hipStream_t st = m->ctx->stream;
  const int din = m->dims[0];
  const long long chunk = kJacHostChunk;
  CHK(jac_stage(m, std::min<long long>(n, chunk)));
  CHK(jac_stage_host(m, std::min<long long>(n, chunk)));
  CHK(fit_out_reserve(m, std::min<long long>(n, chunk)));
  const int route = fisher_route(m, flags);
  for (long long r0 = 0; r0 < n; r0 += chunk) {
    const long long rows = std::min<long long>(chunk, n - r0);
    CHK(stage_rows(m, x, x_dtype, r0, rows, (flags & V21_FWD_IN_TRANSFORM) ? 1 : 0));
    float* dF = m->d_fout;
    float* dl = lnl ? dF + rows * din * din : nullptr;
    float* dg = grad ? dF + rows * (din * din + 1) : nullptr;
    CHK(fisher_launch(m, route, m->d_jxt, m->d_jfac, rows, dF, dl, dg, m->d_lk_data, 0, 1, 0, precision, flags));
    HIPCHK(hipMemcpyAsync(fisher + r0 * din * din, dF, (size_t)rows * din * din * sizeof(float), hipMemcpyDeviceToHost, st));
    if (lnl) HIPCHK(hipMemcpyAsync(lnl + r0, dl, (size_t)rows * sizeof(float), hipMemcpyDeviceToHost, st));
    if (grad) HIPCHK(hipMemcpyAsync(grad + r0 * din, dg, (size_t)rows * din * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  return V21_OK;
}

// ---- fits
extern "C" int v21_mlp_fit_dev(v21_mlp* m, const float* d_x0, int64_t ldx, int64_t n, const float* d_data, int64_t n_data,
                               const v21_fit_opts* opts, float* d_x_hat, float* d_lnl, float* d_lnl_start, float* d_fisher,
                               int32_t* d_status, int precision, int flags) {
  if (!m || !d_x0 || !d_x_hat || !d_lnl) return fail(V21_ERR_ARG, "null argument");
  if (n < 0 || ldx < m->dims[0]) return fail(V21_ERR_ARG, "bad shape: n=%lld ldx=%lld", (long long)n, (long long)ldx);
  const v21_fit_opts o = opts ? *opts : fit_defaults();
  flags &= 0xFF;
  CHK(fit_check(m, precision, flags, n, d_data != nullptr, n_data, o));
  if (n == 0) return V21_OK;
  CHK(use(m->ctx));
  hipStream_t st = m->ctx->stream;
  const int din = m->dims[0], dout = m->dims[m->L];
  CHK(jac_stage(m, n));
  const dim3 grid((unsigned)((n + 255) / 256));
  CHK(jac_prep_rows(m, d_x0, V21_DTYPE_F32, ldx, n, 1));
  const float* data = d_data ? d_data : m->d_lk_data;
  const long long ld = d_data ? dout : 0, rpd = d_data ? n / n_data : 1;
  CHK(fit_core(m, fisher_route(m, flags & ~V21_FWD_IN_TRANSFORM), n, data, ld, rpd, 0, o, precision, flags));
  hipLaunchKernelGGL(fit_finish_kernel<float>, grid, dim3(256), 0, st, (const FitRow*)m->d_fit, d_x_hat, d_lnl, d_lnl_start, (int*)d_status,
                     (long long)n, din, m->tin);
  HIPCHK(hipGetLastError());
  if (d_fisher) {
    // the Fisher matrix at x_hat in raw units: the rows as v21_mlp_fisher_dev transforms them
    const int fr = flags | V21_FWD_IN_TRANSFORM;
    CHK(jac_prep_rows(m, d_x_hat, V21_DTYPE_F32, din, n, 1));
    CHK(fisher_launch(m, fisher_route(m, fr), m->d_jxt, m->d_jfac, n, d_fisher, nullptr, nullptr,
                      m->d_lk_data, 0, 1, 0, precision, fr));
  }
  return V21_OK;
}

extern "C" int v21_mlp_fit(v21_mlp* m, const void* x0, int x_dtype, int64_t n, const float* data, int64_t n_data, const v21_fit_opts* opts,
                           void* x_hat, float* lnl, float* lnl_start, float* fisher, int32_t* status, int precision, int flags) {
  if (!m || !x0 || !x_hat || !lnl) return fail(V21_ERR_ARG, "null argument");
  if (n < 0) return fail(V21_ERR_ARG, "negative row count");
  if (x_dtype != V21_DTYPE_F32 && x_dtype != V21_DTYPE_F64) return fail(V21_ERR_ARG, "x_dtype %d unknown", x_dtype);
  const v21_fit_opts o = opts ? *opts : fit_defaults();
  flags &= 0xFF;
  CHK(fit_check(m, precision, flags, n, data != nullptr, n_data, o));
  if (n == 0) return V21_OK;
  CHK(use(m->ctx));
  hipStream_t st = m->ctx->stream;
  const int din = m->dims[0], dout = m->dims[m->L];
  const long long chunk = kJacHostChunk;
  CHK(jac_stage(m, std::min<long long>(n, chunk)));
  CHK(jac_stage_host(m, std::min<long long>(n, chunk)));
  CHK(fit_out_reserve(m, std::min<long long>(n, chunk)));
  if (data && m->fdata_rows < n_data) {
    if (m->d_fdata) { HIPCHK(hipFree(m->d_fdata)); m->d_fdata = nullptr; }
    m->fdata_rows = 0;
    HIPCHK(hipMalloc((void**)&m->d_fdata, (size_t)n_data * dout * sizeof(float)));
    m->fdata_rows = n_data;
  }
  if (data) HIPCHK(hipMemcpyAsync(m->d_fdata, data, (size_t)n_data * dout * sizeof(float), hipMemcpyHostToDevice, st));
  const float* d_data = data ? m->d_fdata : m->d_lk_data;
  const long long ld = data ? dout : 0, rpd = data ? n / n_data : 1;
  const bool f64 = x_dtype == V21_DTYPE_F64;
  const size_t esz = f64 ? sizeof(double) : sizeof(float);
  // (counted once per call, as v21_mlp_fisher counts: the iterations, and the Fisher matrix at x_hat when asked for)
  const int route = fisher_route(m, flags & ~V21_FWD_IN_TRANSFORM);
  const int route_hat = fisher ? fisher_route(m, flags | V21_FWD_IN_TRANSFORM) : route;
  for (long long r0 = 0; r0 < n; r0 += chunk) {
    const long long rows = std::min<long long>(chunk, n - r0);
    const dim3 grid((unsigned)((rows + 255) / 256));
    CHK(stage_rows(m, x0, x_dtype, r0, rows, 1));
    CHK(fit_core(m, route, rows, d_data, ld, rpd, r0, o, precision, flags));
    float* dF = m->d_fout;
    float* dl = dF + rows * din * din;
    float* dl0 = dl + rows;
    int* ds = (int*)(dl0 + rows);
    if (f64)
      hipLaunchKernelGGL(fit_finish_kernel<double>, grid, dim3(256), 0, st, (const FitRow*)m->d_fit, (double*)m->d_jx64, dl, dl0, ds, rows,
                         din, m->tin);
    else
      hipLaunchKernelGGL(fit_finish_kernel<float>, grid, dim3(256), 0, st, (const FitRow*)m->d_fit, (float*)m->d_jx64, dl, dl0, ds, rows,
                         din, m->tin);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync((char*)x_hat + r0 * din * esz, m->d_jx64, (size_t)rows * din * esz, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(lnl + r0, dl, (size_t)rows * sizeof(float), hipMemcpyDeviceToHost, st));
    if (lnl_start) HIPCHK(hipMemcpyAsync(lnl_start + r0, dl0, (size_t)rows * sizeof(float), hipMemcpyDeviceToHost, st));
    if (status) HIPCHK(hipMemcpyAsync(status + r0, ds, (size_t)rows * sizeof(int), hipMemcpyDeviceToHost, st));
    if (fisher) {
      // the Fisher matrix at x_hat in raw units, from the rows as they were handed back (v21_mlp_fisher's input)
      const int fr = flags | V21_FWD_IN_TRANSFORM;
      CHK(jac_prep_rows(m, m->d_jx64, x_dtype, din, rows, 1));
      CHK(fisher_launch(m, route_hat, m->d_jxt, m->d_jfac, rows, dF, nullptr, nullptr, m->d_lk_data, 0, 1, 0, precision, fr));
      HIPCHK(hipMemcpyAsync(fisher + r0 * din * din, dF, (size_t)rows * din * din * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
  }
  return V21_OK;
}
