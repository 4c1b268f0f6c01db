// api_jacobian.hip -- the parameter Jacobian and the Gaussian log-likelihood with its gradient (include/v21.h:
// v21_mlp_jacobian[_dev], v21_mlp_set_likelihood, v21_mlp_loglike[_dev], v21_route_jacobian, v21_mlp_last_jac_route).
// The reference's Keras model is differentiated with tf.GradientTape; here one launch pushes the primal and the in_dim
// tangents through the stack together (forward mode: 7 inputs against 451 outputs).  Routes: csrc/routes.h
// (decide_jacobian) -- fused_jac<Arch, Prec> (fused_jac.h) for the stacks of archs.h, jac_generic_kernel
// (jac_generic.h) for every other -- unless the handle asked for fused_jac instantiated for ITS stack at run time
// (v21_mlp_jit_jacobian; jit.hip: kJitJac; K18).  What leaves the device of a Jacobian that stays there -- ln L, its gradient, Fisher
// matrices, marginalised or not -- is reduced by jac_reduce_kernel (reduce_kernels.h; reduce_run).
#include "api_internal.h"
#include "fused_jac.h"
#include "jac_generic.h"
#include "reduce_kernels.h"

bool jac_fused_compiled(int L, const int* dims, const int* act) { return compiled_index(g_infer, L, dims, act) >= 0; }

extern "C" int v21_route_jacobian(int n_layers, const int* dims, const int* act, int precision, int64_t n, int flags, int* route) {
  CHK(route_query_args(route, n_layers, dims, act, precision));
  (void)n;
  *route = decide_jacobian(jac_fused_compiled(n_layers, dims, act), dims[0], flags & 0xFF, dims[n_layers], false);
  return V21_OK;
}
// ... and of a handle that asked for its run-time kernel and has it: JAC_FUSED_RT where the stack can have one
extern "C" int v21_route_jacobian_rt(int n_layers, const int* dims, const int* act, int precision, int flags, int* route) {
  CHK(route_query_args(route, n_layers, dims, act, precision));
  *route = decide_jacobian(jac_fused_compiled(n_layers, dims, act), dims[0], flags & 0xFF, dims[n_layers],
                           v21::jit_jac_eligible(n_layers, dims, act, nullptr));
  return V21_OK;
}

// the run-time Jacobian kernel of (stack, precision), requested at most once per handle; nullptr: the stack cannot have
// one, or V21_JIT=0 and nothing is cached
static v21::JitKernel* jac_jit_kernel(v21_mlp* m, int precision) {
  if (!m->jac_jit_asked[precision]) {
    m->jac_jit[precision] = v21::jit_request(m->L, m->dims.data(), m->act.data(), precision | v21::kJitJac);
    m->jac_jit_asked[precision] = true;
  }
  return m->jac_jit[precision];
}
extern "C" int v21_mlp_jit_jacobian(v21_mlp* m, int precision, int wait_ms, int* status) {
  if (!m || !status) return fail(V21_ERR_ARG, "null argument");
  if (precision < 0 || precision > 2) return fail(V21_ERR_ARG, "precision %d unknown", precision);
  *status = -1;
  if (m->fused_id >= 0) { *status = 1; return V21_OK; }  // compiled into the library (archs.h)
  std::string why;
  if (!v21::jit_jac_eligible(m->L, m->dims.data(), m->act.data(), &why))
    return fail(V21_ERR_UNSUPPORTED, "no fused Jacobian kernel for this stack: %s", why.c_str());
  v21::JitKernel* k = jac_jit_kernel(m, precision);
  if (!k) return fail(V21_ERR_UNSUPPORTED, "run-time compilation is switched off (V21_JIT=0) and no cached kernel exists");
  int s = v21::jit_state(k);
  if (s == v21::JIT_COMPILING && wait_ms != 0) s = v21::jit_wait(k, wait_ms);
  *status = s;
  if (s == v21::JIT_FAILED) {
    v21::jit_state(k, &why);
    return fail(V21_ERR_UNSUPPORTED, "fused Jacobian kernel of this stack: %s", why.c_str());
  }
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
  if (!data || !inv_var) { m->has_lk = false; m->nu_k = 0; return V21_OK; }
  const int dout = m->dims[m->L];
  if (n != dout) return fail(V21_ERR_ARG, "likelihood: %d bins, stack output = %d", (int)n, dout);
  for (int k = 0; k < n; ++k)
    if (!(inv_var[k] >= 0.f) || !std::isfinite(inv_var[k])) return fail(V21_ERR_ARG, "likelihood: inv_var[%d] = %g", k, (double)inv_var[k]);
  // (a nuisance record is re-whitened with the new weights first: a basis they make rank-deficient changes nothing)
  NuisRecord rec;
  if (m->nu_k) CHK(nuis_build(m->nu_basis.data(), inv_var, data, m->nu_k, dout, rec));
  CHK(use(m->ctx));
  CHK(m->lk_data.reserve((size_t)dout));
  CHK(m->lk_w.reserve((size_t)dout));
  HIPCHK(hipMemcpyAsync(m->lk_data.p, data, (size_t)dout * sizeof(float), hipMemcpyHostToDevice, m->ctx->stream));
  HIPCHK(hipMemcpyAsync(m->lk_w.p, inv_var, (size_t)dout * sizeof(float), hipMemcpyHostToDevice, m->ctx->stream));
  HIPCHK(hipStreamSynchronize(m->ctx->stream));
  m->lk_h_data.assign(data, data + dout);
  m->lk_h_w.assign(inv_var, inv_var + dout);
  m->has_lk = true;
  if (m->nu_k) {
    CHK(nuis_upload(m, rec));
    m->nu = std::move(rec);
  }
  return V21_OK;
}

int jac_args(v21_mlp* m, bool ptrs, long long n, long long ldx, long long ldy, int x_dtype, int precision, int& flags, const JacEntry& e) {
  if (!m || !ptrs) return fail(V21_ERR_ARG, "null argument");
  if (n < 0) return fail(V21_ERR_ARG, "negative row count");
  if (ldx < m->dims[0] || ldy < m->dims[m->L]) return fail(V21_ERR_ARG, "bad shape: ldx=%lld ldy=%lld", ldx, ldy);
  if (x_dtype != V21_DTYPE_F32 && x_dtype != V21_DTYPE_F64) return fail(V21_ERR_ARG, "x_dtype %d unknown", x_dtype);
  flags &= 0xFF;
  if (m->dims[0] > e.max_in) return fail(V21_ERR_UNSUPPORTED, "%s: %d inputs (at most %d)", e.name, m->dims[0], e.max_in);
  if (n == 0 && !e.fit) return V21_OK;
  if (e.fit && !m->has_tin) return fail(V21_ERR_STATE, "%s: no input transform (v21_mlp_set_input_transform): it defines the box", e.name);
  if (precision < 0 || precision > 2) return fail(V21_ERR_ARG, "precision %d unknown", precision);
  if ((flags & V21_FWD_IN_TRANSFORM) && !m->has_tin) return fail(V21_ERR_STATE, "input transform requested but not set");
  if ((flags & V21_FWD_OUT_TRANSFORM) && !m->has_tout) return fail(V21_ERR_STATE, "output transform requested but not set");
  if (e.like && !m->has_lk) return fail(V21_ERR_STATE, "%s requested but no likelihood set (v21_mlp_set_likelihood)", e.name);
  if (n == 0) return V21_OK;
  if ((flags & V21_FWD_FORCE_JIT) && !(flags & V21_FWD_FORCE_GENERIC)) {
    // diagnostics, as on the forward: the run-time kernel or an error -- for a stack of archs.h too; waits for the compiler
    std::string why;
    if (!v21::jit_jac_eligible(m->L, m->dims.data(), m->act.data(), &why))
      return fail(V21_ERR_UNSUPPORTED, "V21_FWD_FORCE_JIT: no run-time Jacobian kernel for this stack: %s", why.c_str());
    v21::JitKernel* k = jac_jit_kernel(m, precision);
    if (!k) return fail(V21_ERR_UNSUPPORTED, "V21_FWD_FORCE_JIT: run-time compilation is switched off (V21_JIT=0) and no cached kernel exists");
    if (v21::jit_wait(k, -1) != v21::JIT_READY) {
      v21::jit_state(k, &why);
      return fail(V21_ERR_UNSUPPORTED, "V21_FWD_FORCE_JIT: %s", why.c_str());
    }
    // route 3 or an error: what decide_jacobian would silently send to the generic kernel is refused here
    if (ldy != kNoPitch && ldy >= (1ll << 21))
      return fail(V21_ERR_UNSUPPORTED, "V21_FWD_FORCE_JIT: the fused Jacobian addresses y with a row pitch below 2^21 (ldy = %lld)", ldy);
    CHK(use(m->ctx));
    if (v21::jit_preload(k, m->ctx->device) != hipSuccess) {  // (a kernel that needs scratch memory, or cannot be loaded)
      (void)hipGetLastError();
      v21::jit_state(k, &why);
      return fail(V21_ERR_UNSUPPORTED, "V21_FWD_FORCE_JIT: %s", why.c_str());
    }
    return V21_OK;
  }
  return use(m->ctx);
}

int jac_route(v21_mlp* m, int precision, int flags, long long ldy) {
  // opt-in: only a kernel this handle asked for counts, and only once its code object is there (never waited for here)
  // AND loaded on this device: a code object that cannot be loaded or needs scratch memory is marked failed by the load, so
  // this call and every later one decide as a handle that never asked -- before anything of the call has run
  v21::JitKernel* k = m->jac_jit_asked[precision] ? m->jac_jit[precision] : nullptr;
  bool rt_ready = k && v21::jit_state(k) == v21::JIT_READY;
  if (rt_ready && v21::jit_preload(k, m->ctx->device) != hipSuccess) { (void)hipGetLastError(); rt_ready = false; }
  const int route = decide_jacobian(m->fused_id >= 0, m->dims[0], flags, ldy, rt_ready);
  m->last_jac_route = route;
  m->jac_route_count[route] += 1;
  return route;
}

int jac_prep(v21_mlp* m, const void* d_src, int dtype, long long ld, long long n, int tin) {
  const int din = m->dims[0];
  CHK(m->jxt.reserve((size_t)n * din));
  CHK(m->jfac.reserve((size_t)n * din));
  const long long tot = n * din;
  const dim3 grid((unsigned)((tot + 255) / 256));
  float *xt = m->jxt.get(), *fac = m->jfac.get();
  if (dtype == V21_DTYPE_F64)
    hipLaunchKernelGGL(jac_prep_kernel<double>, grid, dim3(256), 0, m->ctx->stream, xt, fac, (const double*)d_src, ld, n, din, tin, m->tin);
  else
    hipLaunchKernelGGL(jac_prep_kernel<float>, grid, dim3(256), 0, m->ctx->stream, xt, fac, (const float*)d_src, ld, n, din, tin, m->tin);
  HIPCHK(hipGetLastError());
  return V21_OK;
}

// Jacobian mode of `route` on the prepped rows [r0, r0 + n): y (nullable, pitch ldy) and jac (n, in_dim, out_dim); or,
// on the generic route with lnl given, the generic kernel's likelihood mode: lnl and grad (nullable).  On the
// context's stream.
static int jac_run(v21_mlp* m, int route, long long r0, long long n, float* y, long long ldy, float* jac, float* lnl, float* grad,
                   int prec, int flags) {
  hipStream_t st = m->ctx->stream;
  const int L = m->L, din = m->dims[0], dout = m->dims[L];
  const bool tout = (flags & V21_FWD_OUT_TRANSFORM) != 0;
  const float* xt = m->jxt.get() + r0 * din;
  const float* fac = m->jfac.get() + r0 * din;
  if (route == JAC_FUSED || route == JAC_FUSED_RT) {
    JacArgs a{};
    a.x = xt; a.ldx = din; a.fac = fac;
    a.y = y; a.ldy = ldy; a.jac = jac; a.n_rows = n;
    CHK(mlp_fused_stream(m, prec, &a.stream));
    a.out_std = tout ? m->out_std : 1.0f;
    a.out_mean_scale = tout ? 1.0f : 0.0f;
    if (route == JAC_FUSED) {
      HIPCHK(g_infer[m->fused_id].jac[prec](a, st));
      return V21_OK;
    }
    // (jac_route loaded the code object before it answered JAC_FUSED_RT: what is left to fail here is the launch itself)
    HIPCHK(v21::jit_launch_jac(m->jac_jit[prec], m->ctx->device, a, st));
    return V21_OK;
  }
  // the stack, tangents per workgroup and LDS size (and the kernel's LDS attribute, once per device)
  JacGenArgs g{};
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
    HIPCHK(hipFuncSetAttribute((const void*)jac_generic_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    HIPCHK(hipFuncSetAttribute((const void*)jac_generic_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    attr_done[m->ctx->device & 63] = true;
  }
  g.w = m->d_w; g.ldy = ldy;
  g.data = m->lk_data.get(); g.wv = m->lk_w.get(); g.like = lnl ? 1 : 0;
  g.out_std = tout ? m->out_std : 1.0f;
  g.mean = tout ? m->d_mean : nullptr;
  for (long long q = 0; q < n; q += 65535) {  // (grid.x <= 65,535 rows per launch; the row offsets move the pointers)
    const long long rows = std::min<long long>(65535, n - q);
    g.xt = xt + q * din; g.fac = fac + q * din; g.n_rows = rows;
    g.y = y ? y + q * ldy : nullptr;
    g.jac = jac ? jac + q * din * dout : nullptr;
    g.lnl = lnl ? lnl + q : nullptr;
    g.grad = grad ? grad + q * din : nullptr;
    const dim3 grid((unsigned)rows, (unsigned)((din + tc - 1) / tc));
    if (route_smooth(m->L, m->act.data())) hipLaunchKernelGGL(jac_generic_kernel<true>, grid, dim3(256), lds, st, g);
    else hipLaunchKernelGGL(jac_generic_kernel<false>, grid, dim3(256), lds, st, g);
    HIPCHK(hipGetLastError());
  }
  return V21_OK;
}

int jac_slices(v21_mlp* m, int route, long long n, bool want_y, int prec, int flags,
               const std::function<int(const float*, const float*, long long, long long)>& reduce) {
  const int din = m->dims[0], dout = m->dims[m->L];
  const long long rows_ws = std::min(n, kLkSlice);
  CHK(m->lk_ws.reserve((size_t)rows_ws * (din + 1) * dout));
  float* wy = want_y ? m->lk_ws.get() : nullptr;
  float* wj = m->lk_ws.get() + rows_ws * dout;
  for (long long r0 = 0; r0 < n; r0 += kLkSlice) {
    const long long rows = std::min(kLkSlice, n - r0);
    CHK(jac_run(m, route, r0, rows, wy, dout, wj, nullptr, nullptr, prec, flags));
    CHK(reduce(wy, wj, r0, rows));
    HIPCHK(hipGetLastError());
  }
  return V21_OK;
}

int jac_chunks(v21_mlp* m, const void* x, int x_dtype, long long n, int tin, ChunkStage& sg,
               const std::function<int(long long, long long)>& run, long long chunk_rows) {
  hipStream_t st = m->ctx->stream;
  const int din = m->dims[0];
  const long long chunk = std::min(n, chunk_rows);
  const size_t esz = x_dtype == V21_DTYPE_F64 ? sizeof(double) : sizeof(float);
  if (x) CHK(m->hin.reserve((size_t)chunk * din));
  CHK(sg.reserve(m, n, chunk));
  for (long long r0 = 0; r0 < n; r0 += chunk_rows) {
    const long long rows = std::min(chunk_rows, n - r0);
    if (x) {
      HIPCHK(hipMemcpyAsync(m->hin.p, (const char*)x + r0 * din * esz, (size_t)rows * din * esz, hipMemcpyHostToDevice, st));
      CHK(jac_prep(m, m->hin.p, x_dtype, din, rows, tin));
    }
    CHK(sg.place(m, r0, rows));
    CHK(run(r0, rows));
    CHK(sg.fetch(m, r0, rows));
    HIPCHK(hipStreamSynchronize(st));
  }
  return V21_OK;
}

// jac_reduce_kernel<NI, NK, FISHER> for din inputs, nk nuisance modes (0: no record) and F asked for or not
typedef void (*reduce_kernel)(const float*, const float*, const float*, long long, long long, long long, const float*, const float*, int,
                              float*, float*, float*, float*, long long, int, int);
static reduce_kernel reduce_pick(int din, int nk, bool fisher) {
#define V21_NK(NI, NK) {jac_reduce_kernel<NI, NK, false>, jac_reduce_kernel<NI, NK, true>}
#define V21_NI(NI) {V21_NK(NI, 0), V21_NK(NI, 4), V21_NK(NI, 8)}
  static const reduce_kernel table[2][3][2] = {V21_NI(8), V21_NI(kJacMaxIn)};
#undef V21_NI
#undef V21_NK
  return table[din > 8][(nk + 3) / 4][fisher];
}

int reduce_run(v21_mlp* m, int route, long long n, float* d_F, float* d_lnl, float* d_grad, float* d_b, const float* d_data,
               long long ld_data, long long rpd, long long row0, int prec, int flags) {
  const int din = m->dims[0], dout = m->dims[m->L], nk = m->nu_k;
  if (nk && din > kJacMaxIn) return fail(V21_ERR_UNSUPPORTED, "nuisance modes: %d inputs (at most %d)", din, kJacMaxIn);
  const reduce_kernel kern = reduce_pick(din, nk, d_F != nullptr);
  return jac_slices(m, route, n, d_lnl || d_grad || d_b, prec, flags, [&](const float* wy, const float* wj, long long r0, long long rows) {
    hipLaunchKernelGGL(kern, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, m->ctx->stream, wy, wj, d_data, ld_data, rpd, row0 + r0,
                       (const float*)m->lk_w.get(), (const float*)m->nu_qf.get(), nk, d_F ? d_F + r0 * din * din : nullptr,
                       d_lnl ? d_lnl + r0 : nullptr, d_grad ? d_grad + r0 * din : nullptr, d_b ? d_b + r0 * nk : nullptr, rows, din, dout);
    return V21_OK;
  });
}

// lnl / grad (nullable) of the n prepped rows: the generic kernel reduces in its own likelihood mode, the fused route's
// Jacobian -- and, with a nuisance record, either route's -- is reduced slice by slice (reduce_run)
static int loglike_run(v21_mlp* m, int route, long long n, float* d_lnl, float* d_grad, int prec, int flags) {
  if (!m->nu_k && route == JAC_GENERIC) return jac_run(m, route, 0, n, nullptr, m->dims[m->L], nullptr, d_lnl, d_grad, prec, flags);
  return reduce_run(m, route, n, nullptr, d_lnl, d_grad, nullptr, m->lk_read(), 0, 1, 0, prec, flags);
}

static constexpr JacEntry kJacobian{"Jacobian", INT_MAX, false, false}, kLoglike{"log-likelihood", INT_MAX, true, false};

extern "C" int v21_mlp_jacobian_dev(v21_mlp* m, const float* d_x, int64_t ldx, int64_t n, float* d_y, int64_t ldy, float* d_jac,
                                    int precision, int flags) {
  CHK(jac_args(m, d_x && d_jac, n, ldx, d_y ? ldy : kNoPitch, V21_DTYPE_F32, precision, flags, kJacobian));
  if (n == 0) return V21_OK;
  if (!d_y) ldy = m->dims[m->L];
  CHK(jac_prep(m, d_x, V21_DTYPE_F32, ldx, n, flags & V21_FWD_IN_TRANSFORM));
  return jac_run(m, jac_route(m, precision, flags, ldy), 0, n, d_y, ldy, d_jac, nullptr, nullptr, precision, flags);
}
extern "C" int v21_mlp_loglike_dev(v21_mlp* m, const float* d_x, int64_t ldx, int64_t n, float* d_lnl, float* d_grad, int precision,
                                   int flags) {
  CHK(jac_args(m, d_x && d_lnl, n, ldx, kNoPitch, V21_DTYPE_F32, precision, flags, kLoglike));
  if (n == 0) return V21_OK;
  CHK(jac_prep(m, d_x, V21_DTYPE_F32, ldx, n, flags & V21_FWD_IN_TRANSFORM));
  return loglike_run(m, jac_route(m, precision, flags, m->dims[m->L]), n, d_lnl, d_grad, precision, flags);
}

extern "C" int v21_mlp_jacobian(v21_mlp* m, const void* x, int x_dtype, int64_t n, float* y, float* jac, int precision, int flags) {
  CHK(jac_args(m, x && jac, n, kNoPitch, kNoPitch, x_dtype, precision, flags, kJacobian));
  if (n == 0) return V21_OK;
  const int din = m->dims[0], dout = m->dims[m->L];
  const int route = jac_route(m, precision, flags, dout);
  ChunkStage sg;
  float *dy, *dj;
  sg.add(y, &dy, dout * sizeof(float));
  sg.add(jac, &dj, (size_t)din * dout * sizeof(float));
  return jac_chunks(m, x, x_dtype, n, flags & V21_FWD_IN_TRANSFORM, sg, [&](long long, long long rows) {
    return jac_run(m, route, 0, rows, dy, dout, dj, nullptr, nullptr, precision, flags);
  });
}
extern "C" int v21_mlp_loglike(v21_mlp* m, const void* x, int x_dtype, int64_t n, float* lnl, float* grad, int precision, int flags) {
  CHK(jac_args(m, x && lnl, n, kNoPitch, kNoPitch, x_dtype, precision, flags, kLoglike));
  if (n == 0) return V21_OK;
  const int route = jac_route(m, precision, flags, m->dims[m->L]);
  ChunkStage sg;
  float *dl, *dg;
  sg.add(lnl, &dl, sizeof(float));
  sg.add(grad, &dg, m->dims[0] * sizeof(float));
  return jac_chunks(m, x, x_dtype, n, flags & V21_FWD_IN_TRANSFORM, sg, [&](long long, long long rows) {
    return loglike_run(m, route, rows, dl, dg, precision, flags);
  });
}
