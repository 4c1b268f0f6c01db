// api_ensemble.hip -- the affine-invariant ensemble sampler on the device (include/v21.h: v21_mlp_sample_ensemble[_dev],
// v21_route_ensemble): Goodman & Weare's stretch move (ensemble_kernels.h) on forward-only ln L.  The loop is the
// sampler's (api_sample.hip) with the Fisher evaluation replaced by lnl_run of api_loglike.hip: the walkers stay on the
// device, every half-move is one evaluation of the n / 2 pending proposals in their compacted layout (on u, without the
// input transform) and one ensemble_step_kernel launch, and the host only launches.  Routes: csrc/routes.h
// (decide_ensemble), decided once per call and counted once by v21_mlp_last_lnl_route.
#include "api_internal.h"
#include "ensemble_kernels.h"

static v21_ensemble_opts ensemble_defaults() {
  v21_ensemble_opts o;
  o.n_walkers = 64;
  o.a = 2.0;
  o.n_steps = 1000;
  o.n_warmup = 500;
  o.thin = 1;
  o.seed = 0;
  o.chain0 = 0;
  o.step0 = 0;
  return o;
}

// the stretch scale and the counts
static int ensemble_check(const v21_ensemble_opts& o) {
  if (!(o.a > 1.0) || !std::isfinite(o.a)) return fail(V21_ERR_ARG, "sample_ensemble: a = %g (above 1 and finite)", o.a);
  return sample_counts("sample_ensemble", o.n_steps, o.n_warmup, o.thin, o.chain0, o.step0);
}

// how the call's n rows (with data: the n / n_data rows of a spectrum) divide into ensembles of W walkers in din dimensions
static int ensemble_shape(int W, int din, long long n, bool has_data, long long n_data) {
  if (W < 2 || W % 2 != 0 || W < 2 * (din + 1) || W > kEnsMaxWalkers)
    return fail(V21_ERR_ARG, "sample_ensemble: n_walkers = %d (even, %d .. %d for %d parameters)", W, 2 * (din + 1), kEnsMaxWalkers, din);
  return whole_groups("sample_ensemble", "ensembles", n, W, has_data && n > 0, n_data);
}

int ens_route_query(const char* what, int n_layers, const int* dims, const int* act, int precision, long long n, long long n_data, int G,
                    int n_modes, int flags, int host_form, int* route, int64_t* chunk_rows, const std::function<int()>& shape, bool rt) {
  CHK(route_query_args(route, n_layers, dims, act, precision));
  if (n < 0 || n_data < 0 || n_modes < 0 || n_modes > 8) return fail(V21_ERR_ARG, "n = %lld, n_data = %lld, n_modes = %d", n, n_data, n_modes);
  if (dims[0] > kFitMaxIn) return fail(V21_ERR_UNSUPPORTED, "%s: %d inputs (at most %d)", what, dims[0], kFitMaxIn);
  CHK(call_data_args(what, n, n_data > 0, n_data));
  CHK(shape());
  const EnsRoute r = decide_ensemble(jac_fused_compiled(n_layers, dims, act), dims[0], n_modes, n_data > 0 ? n / n_data : 0, n, G, flags & 0xFF,
                                     host_form != 0, kJacHostChunk, rt && v21::jit_lnl_eligible(n_layers, dims, act, nullptr));
  *route = r.route;
  if (chunk_rows) *chunk_rows = r.chunk;
  return V21_OK;
}
extern "C" int v21_route_ensemble(int n_layers, const int* dims, const int* act, int precision, int64_t n, int64_t n_data, int n_walkers,
                                  int n_modes, int flags, int host_form, int* route, int64_t* chunk_rows) {
  return ens_route_query("sample_ensemble", n_layers, dims, act, precision, n, n_data, n_walkers, n_modes, flags, host_form, route, chunk_rows,
                         [&] { return ensemble_shape(n_walkers, dims[0], n, n_data > 0, n_data); });
}

// ... and of a handle that asked for its run-time ln L kernel and has it (v21_mlp_jit_loglike): route 3 where the stack can
// have one.  The nested sampler's query is this one with n_live in the place of n_walkers (decide_ensemble reads no more
// of G than the chunk arithmetic).
extern "C" int v21_route_ensemble_rt(int n_layers, const int* dims, const int* act, int precision, int64_t n, int64_t n_data, int n_walkers,
                                     int n_modes, int flags, int host_form, int* route, int64_t* chunk_rows) {
  return ens_route_query("sample_ensemble", n_layers, dims, act, precision, n, n_data, n_walkers, n_modes, flags, host_form, route, chunk_rows,
                         [&] { return ensemble_shape(n_walkers, dims[0], n, n_data > 0, n_data); }, true);
}

EnsRoute ens_route(v21_mlp* m, int precision, long long rpd, long long n, int G, int flags, bool host_form) {
  const EnsRoute r = decide_ensemble(m->fused_id >= 0, m->dims[0], m->nu_k, rpd, n, G, flags, host_form, kJacHostChunk,
                                     lnl_rt_ready(m, precision));
  m->last_lnl_route = r.route;
  m->lnl_route_count[r.route] += 1;
  return r;
}

int half_eval(v21_mlp* m, int route, long long n, long long n_call, const CallData& data, long long row0, int prec, int flags, HalfEval* ev) {
  const long long half = n / 2;
  CHK(m->ens_prop.reserve((size_t)half * m->dims[0]));
  CHK(m->ens_lnl.reserve((size_t)half));
  *ev = HalfEval{m->ens_prop.get(), m->ens_lnl.get(), half, n_call / 2, row0 / 2, CallData{data.d, data.ld, data.ld ? data.rpd / 2 : 1},
                 route, prec, flags & ~V21_FWD_IN_TRANSFORM};
  return V21_OK;
}

// the ensembles of n start rows prepped transformed in m->jxt; `out`: device pointers, samples and x_last of x_dtype; the
// call's first row is global chain `chain0`, its row `row0` of a call of n_call rows (data rows as in fit_run)
static int ensemble_run(v21_mlp* m, int route, long long n, long long n_call, const CallData& data, long long row0, const v21_ensemble_opts& o,
                        long long chain0, int prec, int flags, const v21_ensemble_out& out, int x_dtype) {
  hipStream_t st = m->ctx->stream;
  const int din = m->dims[0];
  CHK(m->ens.reserve((size_t)n));
  HalfEval ev;
  CHK(half_eval(m, route, n, n_call, data, row0, prec, flags, &ev));
  EnsRow* rows = m->ens.get();
  EnsArgs a{};
  a.n = n; a.din = din; a.W = o.n_walkers; a.H = o.n_walkers / 2; a.epw = 256 / a.H;
  a.total = (long long)o.n_warmup + o.n_steps; a.n_warmup = o.n_warmup;
  a.thin = o.thin; a.n_keep = sample_keep(o.n_steps, o.thin);
  a.a = o.a;
  a.seed = o.seed; a.chain0 = (uint64_t)chain0; a.step0 = (uint64_t)o.step0;
  a.samples = out.samples; a.samples_lnl = out.samples_lnl; a.last_prop_u = out.last_prop_u;
  a.t = m->tin;
  const long long ensembles = n / a.W;
  const dim3 grid((unsigned)((ensembles + a.epw - 1) / a.epw));
  // (samples and x_last are of x_dtype, the prior record (api_prior.hip) is there or not: one set of instantiations,
  // picked once)
  // ... and so is the hold record (api_hold.hip), which the HOLD instantiations take as their last argument
  const SamplerRecords rec = sampler_records(m);
  const bool f64 = x_dtype == V21_DTYPE_F64, pri = rec.pri;
  const auto step = pri ? (f64 ? ensemble_step_kernel<double, true, false> : ensemble_step_kernel<float, true, false>)
                        : (f64 ? ensemble_step_kernel<double, false, false> : ensemble_step_kernel<float, false, false>);
  const auto finish = f64 ? ensemble_finish_kernel<double, false> : ensemble_finish_kernel<float, false>;
  const auto step_h = pri ? (f64 ? ensemble_step_kernel<double, true, true, HoldArgs> : ensemble_step_kernel<float, true, true, HoldArgs>)
                          : (f64 ? ensemble_step_kernel<double, false, true, HoldArgs> : ensemble_step_kernel<float, false, true, HoldArgs>);
  const auto finish_h = f64 ? ensemble_finish_kernel<double, true, HoldArgs> : ensemble_finish_kernel<float, true, HoldArgs>;
  const long long last = 2 * a.total + 2;
  for (long long k = 0; k <= last; ++k) {
    if (k > 0) CHK(ev.run(m));
    if (rec.hold)
      hipLaunchKernelGGL(step_h, grid, dim3(256), 0, st, rows, (const float*)m->jxt.get(), ev.prop, (const float*)ev.lnl, k, a, rec.pr, rec.ho);
    else
      hipLaunchKernelGGL(step, grid, dim3(256), 0, st, rows, (const float*)m->jxt.get(), ev.prop, (const float*)ev.lnl, k, a, rec.pr);
    HIPCHK(hipGetLastError());
  }
  EnsOutDev od{out.x_last, out.lnl_last, out.accept_rate, out.mean_u, out.cov_u, out.last_log_alpha, out.last_partner};
  if (rec.hold)
    hipLaunchKernelGGL(finish_h, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const EnsRow*)rows, n, din, (long long)o.n_steps, m->tin,
                       od, rec.ho);
  else
    hipLaunchKernelGGL(finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const EnsRow*)rows, n, din, (long long)o.n_steps, m->tin, od);
  HIPCHK(hipGetLastError());
  return V21_OK;
}

static constexpr JacEntry kEnsemble{"sample_ensemble", kFitMaxIn, true, true};

extern "C" int v21_mlp_sample_ensemble_dev(v21_mlp* m, const float* d_x0, int64_t ldx, int64_t n, const float* d_data, int64_t n_data,
                                           const v21_ensemble_opts* opts, const v21_ensemble_out* out, int precision, int flags) {
  const v21_ensemble_opts o = opts ? *opts : ensemble_defaults();
  CHK(jac_args(m, d_x0 && out && out->x_last, n, ldx, kNoPitch, V21_DTYPE_F32, precision, flags, kEnsemble));
  CHK(call_data_args("sample_ensemble", n, d_data != nullptr, n_data));
  CHK(ensemble_check(o));
  CHK(ensemble_shape(o.n_walkers, m->dims[0], n, d_data != nullptr, n_data));
  if (n == 0) return V21_OK;
  CallData data;
  CHK(call_data(m, n, d_data, false, n_data, &data));
  const EnsRoute r = ens_route(m, precision, d_data ? data.rpd : 0, n, o.n_walkers, flags, false);
  CHK(jac_prep(m, d_x0, V21_DTYPE_F32, ldx, n, 1));
  return ensemble_run(m, r.route, n, n, data, 0, o, o.chain0, precision, flags, *out, V21_DTYPE_F32);
}

// the host form: chunks of whole ensembles (routes.h: decide_ensemble), each staged (ChunkStage), run by ensemble_run and
// copied back
extern "C" int v21_mlp_sample_ensemble(v21_mlp* m, const void* x0, int x_dtype, int64_t n, const float* data, int64_t n_data,
                                       const v21_ensemble_opts* opts, const v21_ensemble_out* out, int precision, int flags) {
  const v21_ensemble_opts o = opts ? *opts : ensemble_defaults();
  CHK(jac_args(m, x0 && out && out->x_last, n, kNoPitch, kNoPitch, x_dtype, precision, flags, kEnsemble));
  CHK(call_data_args("sample_ensemble", n, data != nullptr, n_data));
  CHK(ensemble_check(o));
  CHK(ensemble_shape(o.n_walkers, m->dims[0], n, data != nullptr, n_data));
  if (n == 0) return V21_OK;
  CallData cd;
  CHK(call_data(m, n, data, true, n_data, &cd));
  const EnsRoute r = ens_route(m, precision, data ? cd.rpd : 0, n, o.n_walkers, flags, true);
  ChunkStage sg;
  v21_ensemble_out d{};
  stage_sampler_out(sg, *out, d, sample_keep(o.n_steps, o.thin), m->dims[0], x_dtype == V21_DTYPE_F64 ? sizeof(double) : sizeof(float));
  sg.add(out->last_partner, &d.last_partner, sizeof(int));
  return jac_chunks(m, x0, x_dtype, n, 1, sg, [&](long long r0, long long rows) {
    return ensemble_run(m, r.route, rows, n, cd, r0, o, o.chain0 + r0, precision, flags, d, x_dtype);
  }, r.chunk);
}
