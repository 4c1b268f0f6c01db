// api_jacobian.hip -- the parameter Jacobian and the Gaussian log-likelihood with its gradient (include/v21.h:
// v21_mlp_jacobian[_dev], v21_mlp_set_likelihood, v21_mlp_loglike[_dev], v21_route_jacobian, v21_mlp_last_jac_route).
// The reference's Keras model is differentiated with tf.GradientTape; here one launch pushes the primal and the in_dim
// tangents through the stack together (forward mode: 7 inputs against 451 outputs).  Routes: csrc/routes.h
// (decide_jacobian) -- fused_jac<Arch, Prec> (fused_jac.h) for the stacks of archs.h, jac_generic_kernel
// (jac_generic.h) for every other.
#include "api_internal.h"
#include "fused_jac.h"
#include "jac_generic.h"

namespace v21 {
#define V21_DECL(a)                                                                \
  hipError_t launch_jac_##a##_F32(const JacArgs&, hipStream_t);              \
  hipError_t launch_jac_##a##_F16x2sp(const JacArgs&, hipStream_t);          \
  hipError_t launch_jac_##a##_BF16x2sp(const JacArgs&, hipStream_t);
V21_ARCH_LIST(V21_DECL)
#undef V21_DECL
}  // namespace v21

typedef hipError_t (*jac_launcher)(const JacArgs&, hipStream_t);
// in the order of V21_ARCH_LIST, i.e. of v21_mlp::fused_id (api_forward.hip: g_fused)
#define V21_ENTRY(a) {launch_jac_##a##_F32, launch_jac_##a##_F16x2sp, launch_jac_##a##_BF16x2sp},
static const jac_launcher g_jac[][3] = {V21_ARCH_LIST(V21_ENTRY)};
#undef V21_ENTRY

static bool jac_fused_compiled(int L, const int* dims, const int* act) {
#define V21_MATCH(a)                                                                              \
  if (L == Arch##a::L && std::equal(dims, dims + L + 1, Arch##a::dims) && std::equal(act, act + L, Arch##a::act)) \
    return true;
  V21_ARCH_LIST(V21_MATCH)
#undef V21_MATCH
  return false;
}

extern "C" int v21_route_jacobian(int n_layers, const int* dims, const int* act, int precision, int64_t n, int flags, int* route) {
  if (!dims || !act || !route) return fail(V21_ERR_ARG, "null argument");
  if (n_layers < 1 || n_layers > 16) return fail(V21_ERR_ARG, "n_layers %d out of range", n_layers);
  for (int l = 0; l <= n_layers; ++l)
    if (dims[l] < 1) return fail(V21_ERR_ARG, "dims[%d] = %d", l, dims[l]);
  if (precision < 0 || precision > 2) return fail(V21_ERR_ARG, "precision %d unknown", precision);
  (void)n;
  *route = decide_jacobian(jac_fused_compiled(n_layers, dims, act), dims[0], flags & 0xFF, dims[n_layers]);
  return V21_OK;
}
extern "C" int v21_mlp_last_jac_route(v21_mlp* m, int* route, long long counts[4]) {
  if (!m || !route) return fail(V21_ERR_ARG, "null argument");
  *route = m->last_jac_route;
  if (counts) for (int i = 0; i < 4; ++i) counts[i] = m->jac_route_count[i];
  return V21_OK;
}

extern "C" int v21_mlp_set_likelihood(v21_mlp* m, const float* data, const float* inv_var, int32_t n) {
  if (!m) return fail(V21_ERR_ARG, "null mlp");
  if (!data || !inv_var) { m->has_lk = false; return V21_OK; }
  const int dout = m->dims[m->L];
  if (n != dout) return fail(V21_ERR_ARG, "likelihood: %d bins, stack output = %d", (int)n, dout);
  for (int k = 0; k < n; ++k)
    if (!(inv_var[k] >= 0.f) || !std::isfinite(inv_var[k])) return fail(V21_ERR_ARG, "likelihood: inv_var[%d] = %g", k, (double)inv_var[k]);
  CHK(use(m->ctx));
  if (!m->d_lk_data) HIPCHK(hipMalloc((void**)&m->d_lk_data, (size_t)dout * sizeof(float)));
  if (!m->d_lk_w) HIPCHK(hipMalloc((void**)&m->d_lk_w, (size_t)dout * sizeof(float)));
  HIPCHK(hipMemcpyAsync(m->d_lk_data, data, (size_t)dout * sizeof(float), hipMemcpyHostToDevice, m->ctx->stream));
  HIPCHK(hipMemcpyAsync(m->d_lk_w, inv_var, (size_t)dout * sizeof(float), hipMemcpyHostToDevice, m->ctx->stream));
  HIPCHK(hipStreamSynchronize(m->ctx->stream));
  m->has_lk = true;
  return V21_OK;
}

// (re)size the staging of transformed rows and factors for `rows` rows (every route: a _dev call grows it to its n)
int jac_stage(v21_mlp* m, long long rows) {
  const int din = m->dims[0];
  if (m->jstage_rows >= rows) return V21_OK;
  for (float** p : {&m->d_jxt, &m->d_jfac}) if (*p) { HIPCHK(hipFree(*p)); *p = nullptr; }
  m->jstage_rows = 0;
  HIPCHK(hipMalloc((void**)&m->d_jxt, (size_t)rows * din * sizeof(float)));
  HIPCHK(hipMalloc((void**)&m->d_jfac, (size_t)rows * din * sizeof(float)));
  m->jstage_rows = rows;
  return V21_OK;
}
// ... and the host API's input and result staging, sized by its chunk (at most kJacHostChunk rows), apart from the above
int jac_stage_host(v21_mlp* m, long long rows) {
  const int din = m->dims[0], dout = m->dims[m->L];
  if (m->jhost_rows >= rows) return V21_OK;
  for (float** p : {&m->d_jy, &m->d_jout}) if (*p) { HIPCHK(hipFree(*p)); *p = nullptr; }
  if (m->d_jx64) { HIPCHK(hipFree(m->d_jx64)); m->d_jx64 = nullptr; }
  m->jhost_rows = 0;
  HIPCHK(hipMalloc((void**)&m->d_jx64, (size_t)rows * din * sizeof(double)));
  HIPCHK(hipMalloc((void**)&m->d_jy, (size_t)rows * dout * sizeof(float)));
  HIPCHK(hipMalloc((void**)&m->d_jout, (size_t)rows * din * std::max(dout, 2) * sizeof(float)));
  m->jhost_rows = rows;
  return V21_OK;
}

// the generic kernel's stack description, tangents per workgroup and LDS size (and its LDS attribute, once per device)
static int jac_gen_setup(v21_mlp* m, JacGenArgs& g, size_t* lds_out) {
  const int L = m->L, din = m->dims[0];
  g.L = L; g.in_dim = din;
  int maxw = 0;
  for (int l = 0; l <= L; ++l) { g.dims[l] = m->dims[l]; maxw = std::max(maxw, m->dims[l]); }
  for (int l = 0; l < L; ++l) { g.act[l] = m->act[l]; g.nw[l] = m->nw(l); g.w_off[l] = m->w_off[l]; g.b_off[l] = m->b_off[l]; }
  constexpr size_t kLdsMax = 160 * 1024;  // gfx950: LDS per workgroup
  int tc = std::min(din, kJacGenCols - 1);
  while (tc > 1 && (size_t)2 * (tc + 1) * maxw * sizeof(float) > kLdsMax) --tc;
  const size_t lds = std::max((size_t)2 * (tc + 1) * maxw, (size_t)256) * sizeof(float);
  if (lds > kLdsMax) return fail(V21_ERR_UNSUPPORTED, "Jacobian: a %d-wide layer does not fit the generic kernel's LDS", maxw);
  g.tc = tc; g.maxw = maxw;
  static bool attr_done[64] = {};
  if (!attr_done[m->ctx->device & 63]) {
    HIPCHK(hipFuncSetAttribute((const void*)jac_generic_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    attr_done[m->ctx->device & 63] = true;
  }
  *lds_out = lds;
  return V21_OK;
}

// the likelihood workspace (m->d_lk_ws): y and jac of up to `rows` rows, (1 + in_dim) out_dim floats each
int lk_ws_reserve(v21_mlp* m, long long rows) {
  const int din = m->dims[0], dout = m->dims[m->L];
  if (m->lk_ws_rows >= rows) return V21_OK;
  if (m->d_lk_ws) { HIPCHK(hipFree(m->d_lk_ws)); m->d_lk_ws = nullptr; }
  m->lk_ws_rows = 0;
  HIPCHK(hipMalloc((void**)&m->d_lk_ws, (size_t)rows * (din + 1) * dout * sizeof(float)));
  m->lk_ws_rows = rows;
  return V21_OK;
}

// Jacobian mode of `route` on rows (xt, fac) of pitch in_dim: y (n, out_dim) and jac (n, in_dim, out_dim), on the
// context's stream (api_fit.hip: one slice of the likelihood workspace; the caller counts the route)
int jac_eval_rows(v21_mlp* m, int route, const float* xt, const float* fac, long long n, float* y, float* jac, int prec, int flags) {
  hipStream_t st = m->ctx->stream;
  const int din = m->dims[0], dout = m->dims[m->L];
  const bool tout = (flags & V21_FWD_OUT_TRANSFORM) != 0;
  if (route == JAC_FUSED) {
    JacArgs a{};
    a.x = xt; a.ldx = din; a.fac = fac;
    a.y = y; a.ldy = dout; a.jac = jac; a.n_rows = n;
    CHK(mlp_fused_stream(m, prec, &a.stream));
    a.out_std = tout ? m->out_std : 1.0f;
    a.out_mean_scale = tout ? 1.0f : 0.0f;
    HIPCHK(g_jac[m->fused_id][prec](a, st));
    return V21_OK;
  }
  JacGenArgs g{};
  size_t lds = 0;
  CHK(jac_gen_setup(m, g, &lds));
  g.w = m->d_w; g.fac = fac; g.ldy = dout; g.like = 0;
  g.data = m->d_lk_data; g.wv = m->d_lk_w;
  g.out_std = tout ? m->out_std : 1.0f;
  g.mean = tout ? m->d_mean : nullptr;
  for (long long r0 = 0; r0 < n; r0 += 65535) {
    const long long rows = std::min<long long>(65535, n - r0);
    g.xt = xt + r0 * din; g.fac = fac + r0 * din; g.n_rows = rows;
    g.y = y ? y + r0 * dout : nullptr; g.jac = jac + r0 * din * dout;
    hipLaunchKernelGGL(jac_generic_kernel, dim3((unsigned)rows, (unsigned)((din + g.tc - 1) / g.tc)), dim3(256), lds, st, g);
    HIPCHK(hipGetLastError());
  }
  return V21_OK;
}

// device rows (float32 / float64, pitch ld) -> m->d_jxt / d_jfac (the caller has staged n rows), on the context's stream
int jac_prep_rows(v21_mlp* m, const void* d_src, int dtype, long long ld, long long n, int tin) {
  const int din = m->dims[0];
  const long long tot = n * din;
  const dim3 grid((unsigned)((tot + 255) / 256));
  if (dtype == V21_DTYPE_F64)
    hipLaunchKernelGGL(jac_prep_kernel<double>, grid, dim3(256), 0, m->ctx->stream, m->d_jxt, m->d_jfac, (const double*)d_src, ld, n, din,
                       tin, m->tin);
  else
    hipLaunchKernelGGL(jac_prep_kernel<float>, grid, dim3(256), 0, m->ctx->stream, m->d_jxt, m->d_jfac, (const float*)d_src, ld, n, din,
                       tin, m->tin);
  HIPCHK(hipGetLastError());
  return V21_OK;
}

// transformed rows + factors (m->d_jxt / d_jfac) -> y / jac or lnl / grad, on the context's stream
static int jac_launch(v21_mlp* m, long long n, float* d_y, long long ldy, float* d_jac, float* d_lnl, float* d_grad,
                      int prec, int flags, bool like) {
  hipStream_t st = m->ctx->stream;
  const int L = m->L, din = m->dims[0], dout = m->dims[L];
  const bool tout = (flags & V21_FWD_OUT_TRANSFORM) != 0;
  const int route = decide_jacobian(m->fused_id >= 0, din, flags, ldy);
  m->last_jac_route = route; m->jac_route_count[route] += 1;
  if (route == JAC_FUSED) {
    // likelihood: the Jacobian-mode kernel into a device workspace, reduced there (jac_loglike_kernel), in slices
    constexpr long long kSlice = kLkSlice;
    JacArgs a{};
    a.x = m->d_jxt; a.ldx = din; a.fac = m->d_jfac;
    a.y = d_y; a.ldy = ldy; a.jac = d_jac;
    CHK(mlp_fused_stream(m, prec, &a.stream));
    a.out_std = tout ? m->out_std : 1.0f;
    a.out_mean_scale = tout ? 1.0f : 0.0f;
    if (!like) {
      a.n_rows = n;
      HIPCHK(g_jac[m->fused_id][prec](a, st));
      return V21_OK;
    }
    const long long rows_ws = std::min(n, kSlice);
    CHK(lk_ws_reserve(m, rows_ws));
    for (long long r0 = 0; r0 < n; r0 += kSlice) {
      const long long rows = std::min(kSlice, n - r0);
      a.x = m->d_jxt + r0 * din; a.fac = m->d_jfac + r0 * din; a.n_rows = rows;
      a.y = m->d_lk_ws; a.ldy = dout; a.jac = m->d_lk_ws + rows_ws * dout;
      HIPCHK(g_jac[m->fused_id][prec](a, st));
      hipLaunchKernelGGL(jac_loglike_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, (const float*)a.y, (const float*)a.jac,
                         (const float*)m->d_lk_data, (const float*)m->d_lk_w, d_lnl + r0, d_grad ? d_grad + r0 * din : nullptr, rows,
                         din, dout);
      HIPCHK(hipGetLastError());
    }
    return V21_OK;
  }
  JacGenArgs g{};
  size_t lds = 0;
  CHK(jac_gen_setup(m, g, &lds));
  g.w = m->d_w; g.xt = m->d_jxt; g.fac = m->d_jfac; g.n_rows = n;
  g.y = d_y; g.ldy = ldy; g.jac = d_jac; g.lnl = d_lnl; g.grad = d_grad;
  g.data = m->d_lk_data; g.wv = m->d_lk_w; g.like = like ? 1 : 0;
  g.out_std = tout ? m->out_std : 1.0f;
  g.mean = tout ? m->d_mean : nullptr;
  const int tc = g.tc;
  for (long long r0 = 0; r0 < n; r0 += 65535) {  // (grid.x <= 65,535 rows per launch; the row offsets move the pointers)
    JacGenArgs gs = g;
    const long long rows = std::min<long long>(65535, n - r0);
    gs.xt += r0 * din; gs.fac += r0 * din; gs.n_rows = rows;
    if (gs.y) gs.y += r0 * ldy;
    if (like) { gs.lnl += r0; if (gs.grad) gs.grad += r0 * din; }
    else gs.jac += r0 * din * dout;
    hipLaunchKernelGGL(jac_generic_kernel, dim3((unsigned)rows, (unsigned)((din + tc - 1) / tc)), dim3(256), lds, st, gs);
    HIPCHK(hipGetLastError());
  }
  return V21_OK;
}

int jac_check(v21_mlp* m, int precision, int flags, bool like) {
  if (precision < 0 || precision > 2) return fail(V21_ERR_ARG, "precision %d unknown", precision);
  if ((flags & V21_FWD_IN_TRANSFORM) && !m->has_tin) return fail(V21_ERR_STATE, "input transform requested but not set");
  if ((flags & V21_FWD_OUT_TRANSFORM) && !m->has_tout) return fail(V21_ERR_STATE, "output transform requested but not set");
  if (like && !m->has_lk) return fail(V21_ERR_STATE, "log-likelihood requested but no data set (v21_mlp_set_likelihood)");
  return V21_OK;
}

// device-resident float32 rows -> staged transformed rows and factors
static int jac_prep_dev(v21_mlp* m, const float* d_x, long long ldx, long long n, int flags) {
  const int din = m->dims[0];
  CHK(jac_stage(m, n));
  const long long tot = n * din;
  hipLaunchKernelGGL(jac_prep_kernel<float>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, m->ctx->stream, m->d_jxt, m->d_jfac,
                     d_x, ldx, n, din, (flags & V21_FWD_IN_TRANSFORM) ? 1 : 0, m->tin);
  HIPCHK(hipGetLastError());
  return V21_OK;
}

extern "C" int v21_mlp_jacobian_dev(v21_mlp* m, const float* d_x, int64_t ldx, int64_t n, float* d_y, int64_t ldy, float* d_jac,
                                    int precision, int flags) {
  if (!m || !d_x || !d_jac) return fail(V21_ERR_ARG, "null argument");
  if (n < 0 || ldx < m->dims[0] || (d_y && ldy < m->dims[m->L])) return fail(V21_ERR_ARG, "bad shape: n=%lld ldx=%lld ldy=%lld", (long long)n, (long long)ldx, (long long)ldy);
  if (n == 0) return V21_OK;
  CHK(use(m->ctx));
  CHK(jac_check(m, precision, flags, false));
  CHK(jac_prep_dev(m, d_x, ldx, n, flags));
  return jac_launch(m, n, d_y, d_y ? ldy : m->dims[m->L], d_jac, nullptr, nullptr, precision, flags, false);
}
extern "C" int v21_mlp_loglike_dev(v21_mlp* m, const float* d_x, int64_t ldx, int64_t n, float* d_lnl, float* d_grad, int precision,
                                   int flags) {
  if (!m || !d_x || !d_lnl) return fail(V21_ERR_ARG, "null argument");
  if (n < 0 || ldx < m->dims[0]) return fail(V21_ERR_ARG, "bad shape: n=%lld ldx=%lld", (long long)n, (long long)ldx);
  if (n == 0) return V21_OK;
  CHK(use(m->ctx));
  CHK(jac_check(m, precision, flags, true));
  CHK(jac_prep_dev(m, d_x, ldx, n, flags));
  return jac_launch(m, n, nullptr, m->dims[m->L], nullptr, d_lnl, d_grad, precision, flags, true);
}

// host rows (float32 or float64) in chunks: stage, transform + factors on the device, launch, copy back
static int jac_host(v21_mlp* m, const void* x, int x_dtype, long long n, float* y, float* jac, float* lnl, float* grad,
                    int precision, int flags, bool like) {
  if (!m || !x || (like ? !lnl : !jac)) return fail(V21_ERR_ARG, "null argument");
  if (n < 0) return fail(V21_ERR_ARG, "negative row count");
  if (x_dtype != V21_DTYPE_F32 && x_dtype != V21_DTYPE_F64) return fail(V21_ERR_ARG, "x_dtype %d unknown", x_dtype);
  flags &= 0xFF;
  if (n == 0) return V21_OK;
  CHK(use(m->ctx));
  CHK(jac_check(m, precision, flags, like));
  hipStream_t st = m->ctx->stream;
  const int din = m->dims[0], dout = m->dims[m->L];
  const long long chunk = kJacHostChunk;
  CHK(jac_stage(m, std::min(n, chunk)));
  CHK(jac_stage_host(m, std::min(n, chunk)));
  const int tin = (flags & V21_FWD_IN_TRANSFORM) ? 1 : 0;
  for (long long r0 = 0; r0 < n; r0 += chunk) {
    const long long rows = std::min(chunk, n - r0), tot = rows * din;
    const dim3 grid((unsigned)((tot + 255) / 256));
    if (x_dtype == V21_DTYPE_F64) {
      HIPCHK(hipMemcpyAsync(m->d_jx64, (const double*)x + r0 * din, (size_t)tot * sizeof(double), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(jac_prep_kernel<double>, grid, dim3(256), 0, st, m->d_jxt, m->d_jfac, (const double*)m->d_jx64, (long long)din,
                         rows, din, tin, m->tin);
    } else {
      float* raw = m->d_jy;  // (the y staging holds the raw rows until the prep kernel has read them: dout >= 1 floats per row)
      if (dout < din) raw = m->d_jout;
      HIPCHK(hipMemcpyAsync(raw, (const float*)x + r0 * din, (size_t)tot * sizeof(float), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(jac_prep_kernel<float>, grid, dim3(256), 0, st, m->d_jxt, m->d_jfac, (const float*)raw, (long long)din, rows,
                         din, tin, m->tin);
    }
    HIPCHK(hipGetLastError());
    if (!like) {
      CHK(jac_launch(m, rows, y ? m->d_jy : nullptr, dout, m->d_jout, nullptr, nullptr, precision, flags, false));
      if (y) HIPCHK(hipMemcpyAsync(y + r0 * dout, m->d_jy, (size_t)rows * dout * sizeof(float), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(jac + r0 * din * dout, m->d_jout, (size_t)rows * din * dout * sizeof(float), hipMemcpyDeviceToHost, st));
    } else {
      float* d_lnl = m->d_jout;
      float* d_grad = grad ? m->d_jout + rows : nullptr;
      CHK(jac_launch(m, rows, nullptr, dout, nullptr, d_lnl, d_grad, precision, flags, true));
      HIPCHK(hipMemcpyAsync(lnl + r0, d_lnl, (size_t)rows * sizeof(float), hipMemcpyDeviceToHost, st));
      if (grad) HIPCHK(hipMemcpyAsync(grad + r0 * din, d_grad, (size_t)rows * din * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
  }
  return V21_OK;
}
extern "C" int v21_mlp_jacobian(v21_mlp* m, const void* x, int x_dtype, int64_t n, float* y, float* jac, int precision, int flags) {
  return jac_host(m, x, x_dtype, n, y, jac, nullptr, nullptr, precision, flags, false);
}
extern "C" int v21_mlp_loglike(v21_mlp* m, const void* x, int x_dtype, int64_t n, float* lnl, float* grad, int precision, int flags) {
  return jac_host(m, x, x_dtype, n, nullptr, nullptr, lnl, grad, precision, flags, true);
}
