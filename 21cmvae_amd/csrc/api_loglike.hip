// api_loglike.hip -- the forward-only Gaussian log-likelihood (include/v21.h: v21_mlp_loglike_fwd[_dev],
// v21_route_loglike_fwd, v21_mlp_last_lnl_route): ln L without its gradient, the call nested samplers, ensemble samplers
// and importance sampling make.  Routes: csrc/routes.h (decide_loglike_fwd) -- the ln L variant of fused_fwd<Arch, Prec>
// (compiled.h: the Lnl family), which reduces chi-square in the output layer's epilogue and writes 4 bytes per row, for the
// stacks of archs.h whose data are uniform per 128-row workgroup; for everything else the forward on its own route
// into the likelihood workspace, y only, then lnl_reduce_kernel (reduce_kernels.h) -- unless the handle asked for the
// ln L variant instantiated for ITS stack at run time (v21_mlp_jit_loglike; jit.hip: kJitLnl; K19): route 3, the same
// kernel template on the same FusedArgs.  The host path is the Jacobian
// side's: jac_args, call_data, jac_chunks with its ChunkStage and the lk_ws workspace (api_internal.h).
#include "api_internal.h"
#include "reduce_kernels.h"

extern "C" int v21_route_loglike_fwd(int n_layers, const int* dims, const int* act, int precision, int64_t n, int64_t n_data, int n_modes,
                                     int flags, int* route) {
  CHK(route_query_args(route, n_layers, dims, act, precision));
  if (n < 0 || n_data < 0 || n_modes < 0 || n_modes > 8) return fail(V21_ERR_ARG, "n = %lld, n_data = %lld, n_modes = %d", (long long)n, (long long)n_data, n_modes);
  CHK(call_data_args("loglike_fwd", n, n_data > 0, n_data));
  *route = decide_loglike_fwd(jac_fused_compiled(n_layers, dims, act), dims[0], n_modes, n_data > 0 ? n / n_data : 0, n, flags & 0xFF, false);
  return V21_OK;
}
// ... and of a handle that asked for its run-time kernel and has it: LNL_FUSED_RT where the stack can have one
extern "C" int v21_route_loglike_fwd_rt(int n_layers, const int* dims, const int* act, int precision, int64_t n, int64_t n_data, int n_modes,
                                        int flags, int* route) {
  CHK(v21_route_loglike_fwd(n_layers, dims, act, precision, n, n_data, n_modes, flags, route));
  *route = decide_loglike_fwd(jac_fused_compiled(n_layers, dims, act), dims[0], n_modes, n_data > 0 ? n / n_data : 0, n, flags & 0xFF,
                              v21::jit_lnl_eligible(n_layers, dims, act, nullptr));
  return V21_OK;
}

// the run-time ln L kernel of (stack, precision), requested at most once per handle; nullptr: the stack cannot have one, or
// V21_JIT=0 and nothing is cached
static v21::JitKernel* lnl_jit_kernel(v21_mlp* m, int precision) {
  if (!m->lnl_jit_asked[precision]) {
    m->lnl_jit[precision] = v21::jit_request(m->L, m->dims.data(), m->act.data(), precision | v21::kJitLnl);
    m->lnl_jit_asked[precision] = true;
  }
  return m->lnl_jit[precision];
}
extern "C" int v21_mlp_jit_loglike(v21_mlp* m, int precision, int wait_ms, int* status) {
  if (!m || !status) return fail(V21_ERR_ARG, "null argument");
  if (precision < 0 || precision > 2) return fail(V21_ERR_ARG, "precision %d unknown", precision);
  *status = -1;
  if (m->fused_id >= 0) { *status = 1; return V21_OK; }  // compiled into the library (archs.h)
  std::string why;
  if (!v21::jit_lnl_eligible(m->L, m->dims.data(), m->act.data(), &why))
    return fail(V21_ERR_UNSUPPORTED, "no fused ln L kernel for this stack: %s", why.c_str());
  v21::JitKernel* k = lnl_jit_kernel(m, precision);
  if (!k) return fail(V21_ERR_UNSUPPORTED, "run-time compilation is switched off (V21_JIT=0) and no cached kernel exists");
  int s = v21::jit_state(k);
  if (s == v21::JIT_COMPILING && wait_ms != 0) s = v21::jit_wait(k, wait_ms);
  *status = s;
  if (s == v21::JIT_FAILED) {
    v21::jit_state(k, &why);
    return fail(V21_ERR_UNSUPPORTED, "fused ln L kernel of this stack: %s", why.c_str());
  }
  return V21_OK;
}
bool lnl_rt_ready(v21_mlp* m, int precision) {
  v21::JitKernel* k = m->lnl_jit_asked[precision] ? m->lnl_jit[precision] : nullptr;
  if (!k || v21::jit_state(k) != v21::JIT_READY) return false;
  if (v21::jit_preload(k, m->ctx->device) != hipSuccess) { (void)hipGetLastError(); return false; }
  return true;
}
extern "C" int v21_mlp_last_lnl_route(v21_mlp* m, int* route, long long counts[4]) {
  if (!m || !route) return fail(V21_ERR_ARG, "null argument");
  *route = m->last_lnl_route;
  if (counts) for (int i = 0; i < 4; ++i) counts[i] = m->lnl_route_count[i];
  return V21_OK;
}

// the route of one entry-point call, counted once (rpd: 0 for the record)
static int lnl_route(v21_mlp* m, int precision, long long rpd, long long n, int flags) {
  const int route = decide_loglike_fwd(m->fused_id >= 0, m->dims[0], m->nu_k, rpd, n, flags, lnl_rt_ready(m, precision));
  m->last_lnl_route = route;
  m->lnl_route_count[route] += 1;
  return route;
}

typedef void (*lnl_reduce)(const float*, long long, const float*, long long, long long, long long, const float*, const float*, int, float*,
                           long long, int);

// lnl of the n device rows d_x (pitch ldx; raw, or transformed already with V21_FWD_IN_TRANSFORM cleared) that start at
// row0 of a call of n_call rows, on `route`, on the context's stream (api_internal.h: the ensemble sampler's evaluation too)
int lnl_run(v21_mlp* m, int route, const float* d_x, long long ldx, long long n, long long n_call, const CallData& cd, long long row0,
            float* d_lnl, int prec, int flags) {
  hipStream_t st = m->ctx->stream;
  const int dout = m->dims[m->L];
  if (route == LNL_FUSED || route == LNL_FUSED_RT) {
    FusedArgs a{};
    CHK(mlp_fused_stream(m, prec, &a.stream));
    a.x = d_x; a.ldx = ldx; a.y = d_lnl; a.ldy = 1; a.n_rows = n;
    const bool tout = (flags & V21_FWD_OUT_TRANSFORM) != 0;
    a.out_std = tout ? m->out_std : 1.0f;
    a.out_mean_scale = tout ? 1.0f : 0.0f;
    a.in_transform = (flags & V21_FWD_IN_TRANSFORM) ? 1 : 0;
    if (a.in_transform) a.tin = m->tin;
    a.lnl_d = cd.d; a.lnl_w = m->lk_w.get(); a.lnl_ld = cd.ld;
    a.lnl_wg0 = (unsigned)(row0 / kLnlWgRows);
    a.lnl_wgpd = cd.ld ? (unsigned)(cd.rpd / kLnlWgRows) : 1u;
    // (route 3: the entry point loaded the code object before it answered LNL_FUSED_RT -- what is left to fail is the launch)
    if (route == LNL_FUSED) HIPCHK(g_infer[m->fused_id].lnl[prec](a, st));
    else HIPCHK(v21::jit_launch_lnl(m->lnl_jit[prec], m->ctx->device, a, st));
    return V21_OK;
  }
  // the forward's own route for these rows and flags, slice by slice into the workspace (y only), each slice reduced
  // there.  A call of more rows than the few-row route serves keeps every slice and chunk off it: one result array
  // must not hold two summation orders.
  const int fl = flags | (n_call > V21_SMALL_BATCH_ROWS ? V21_FWD_NO_SMALL : 0);
  static const lnl_reduce table[3] = {lnl_reduce_kernel<0>, lnl_reduce_kernel<4>, lnl_reduce_kernel<8>};
  const lnl_reduce kern = table[(m->nu_k + 3) / 4];
  CHK(m->lk_ws.reserve((size_t)std::min(n, kLkSlice) * dout));
  float* wy = m->lk_ws.get();
  for (long long s0 = 0; s0 < n; s0 += kLkSlice) {
    const long long rows = std::min(kLkSlice, n - s0);
    CHK(v21_mlp_forward_dev(m, d_x + s0 * ldx, ldx, rows, wy, dout, prec, fl));
    hipLaunchKernelGGL(kern, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, (const float*)wy, (long long)dout, cd.d, cd.ld, cd.rpd,
                       row0 + s0, (const float*)m->lk_w.get(), (const float*)m->nu_qf.get(), m->nu_k, d_lnl + s0, rows, dout);
    HIPCHK(hipGetLastError());
  }
  return V21_OK;
}

static constexpr JacEntry kLoglikeFwd{"forward-only log-likelihood", INT_MAX, true, false};

extern "C" int v21_mlp_loglike_fwd_dev(v21_mlp* m, const float* d_x, int64_t ldx, int64_t n, const float* d_data, int64_t n_data,
                                       float* d_lnl, int precision, int flags) {
  CHK(jac_args(m, d_x && d_lnl, n, ldx, kNoPitch, V21_DTYPE_F32, precision, flags, kLoglikeFwd));
  CHK(call_data_args("loglike_fwd", n, d_data != nullptr, n_data));
  if (n == 0) return V21_OK;
  CallData cd;
  CHK(call_data(m, n, d_data, false, n_data, &cd));
  return lnl_run(m, lnl_route(m, precision, d_data ? cd.rpd : 0, n, flags), d_x, ldx, n, n, cd, 0, d_lnl, precision, flags);
}

extern "C" int v21_mlp_loglike_fwd(v21_mlp* m, const void* x, int x_dtype, int64_t n, const float* data, int64_t n_data, float* lnl,
                                   int precision, int flags) {
  CHK(jac_args(m, x && lnl, n, kNoPitch, kNoPitch, x_dtype, precision, flags, kLoglikeFwd));
  CHK(call_data_args("loglike_fwd", n, data != nullptr, n_data));
  if (n == 0) return V21_OK;
  CallData cd;
  CHK(call_data(m, n, data, true, n_data, &cd));
  const int route = lnl_route(m, precision, data ? cd.rpd : 0, n, flags);
  // chunks of kJacHostChunk rows, rounded down to whole spectra when a data matrix is given (routes.h: a fused call's
  // chunks then start on a workgroup boundary)
  static_assert(kJacHostChunk % kLnlWgRows == 0, "a chunk of the record's rows starts on a workgroup boundary");
  const long long chunk = lnl_host_chunk(kJacHostChunk, data ? cd.rpd : 0);
  // jac_chunks leaves a chunk's rows transformed in m->jxt (par_transform.h's own functions, float32 or float64 rows):
  // the kernels read those, without the input transform
  const int din = m->dims[0];
  ChunkStage sg;
  float* dl;
  sg.add(lnl, &dl, sizeof(float));
  return jac_chunks(m, x, x_dtype, n, flags & V21_FWD_IN_TRANSFORM, sg, [&](long long r0, long long rows) {
    return lnl_run(m, route, m->jxt.get(), din, rows, n, cd, r0, dl, precision, flags & ~V21_FWD_IN_TRANSFORM);
  }, chunk);
}
