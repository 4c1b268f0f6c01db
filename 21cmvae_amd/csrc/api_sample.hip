// api_sample.hip -- posterior sampling on the device (include/v21.h: v21_mlp_sample[_dev]): n independent chains of a
// Fisher-preconditioned Metropolis-adjusted Langevin sampler (sample_kernels.h) in the fit's coordinates.  The loop is
// the fit's without its read-back: the chain state stays on the device, every transition is one Fisher evaluation of the
// pending proposals (reduce_run of api_jacobian.hip, on u without the input transform) and one sample_step_kernel launch,
// and the host only launches.  The tempered entries (v21_mlp_sample_tempered[_dev]) run the same loop with
// sample_step_tempered_kernel in the step kernel's place: T consecutive rows form a ladder of inverse temperatures whose
// rungs exchange their points inside that kernel.  A handle with a prior record (api_prior.hip) launches the PRIOR
// instantiations of both step kernels, one with a hold record (api_hold.hip) the HOLD instantiations of the init, step
// and finish kernels, which take the record as one further argument.
#include "api_internal.h"
#include "sample_kernels.h"

static v21_sample_opts sample_defaults() {
  v21_sample_opts o;
  o.n_steps = 1000;
  o.n_warmup = 200;
  o.thin = 1;
  o.eps0 = 1.0;
  o.ridge = 1.0;
  o.target_accept = 0.574;
  o.seed = 0;
  o.chain0 = 0;
  o.step0 = 0;
  return o;
}

// the chains of n start rows prepped transformed (their fac is overwritten); `out`: device pointers, samples and x_last
// of x_dtype; the call's first chain is global chain `chain0`, its row `row0` of the call (data rows as in fit_run).
// tp: the ladder of a tempered call (n a multiple of its n_temps) and its results `to`, device pointers; nullptr:
// independent chains
static int sample_run(v21_mlp* m, int route, long long n, const CallData& data, long long row0, const v21_sample_opts& o, long long chain0,
                      const double* d_eps_start, int prec, int flags, const v21_sample_out& out, int x_dtype,
                      const v21_temper_opts* tp = nullptr, const v21_temper_out* to = nullptr) {
  hipStream_t st = m->ctx->stream;
  const int din = m->dims[0];
  CHK(m->smp.reserve((size_t)n));
  CHK(m->fF.reserve((size_t)n * din * din));
  CHK(m->fl.reserve((size_t)n));
  CHK(m->fg.reserve((size_t)n * din));
  SampleRow* cs = m->smp.get();
  float *F = m->fF.get(), *l = m->fl.get(), *g = m->fg.get();
  const dim3 grid((unsigned)((n + 255) / 256));
  SampleArgs a{};
  a.n = n; a.din = din;
  a.total = (long long)o.n_warmup + o.n_steps; a.n_warmup = o.n_warmup;
  a.thin = o.thin; a.n_keep = sample_keep(o.n_steps, o.thin);
  a.ridge = o.ridge; a.target = o.target_accept;
  a.seed = o.seed; a.chain0 = (uint64_t)chain0; a.step0 = (uint64_t)o.step0;
  a.samples = out.samples; a.samples_lnl = out.samples_lnl;
  a.t = m->tin;
  // (samples and x_last are of x_dtype, the prior record is there or not, the hold record is there or not: one set of
  // instantiations, picked once; the HOLD ones take the record as their last argument)
  const SamplerRecords rec = sampler_records(m);
  const bool f64 = x_dtype == V21_DTYPE_F64, pri = rec.pri;
  if (rec.hold)
    hipLaunchKernelGGL((sample_init_kernel<true, HoldArgs>), grid, dim3(256), 0, st, cs, m->jxt.get(), m->jfac.get(), n, din, o.eps0, d_eps_start,
                       rec.ho);
  else
    hipLaunchKernelGGL(sample_init_kernel<false>, grid, dim3(256), 0, st, cs, m->jxt.get(), m->jfac.get(), n, din, o.eps0, d_eps_start);
  HIPCHK(hipGetLastError());
  const auto step = pri ? (f64 ? sample_step_kernel<double, true, false> : sample_step_kernel<float, true, false>)
                        : (f64 ? sample_step_kernel<double, false, false> : sample_step_kernel<float, false, false>);
  const auto tstep = pri ? (f64 ? sample_step_tempered_kernel<double, true, false> : sample_step_tempered_kernel<float, true, false>)
                         : (f64 ? sample_step_tempered_kernel<double, false, false> : sample_step_tempered_kernel<float, false, false>);
  const auto finish = f64 ? sample_finish_kernel<double, false> : sample_finish_kernel<float, false>;
  const auto step_h = pri ? (f64 ? sample_step_kernel<double, true, true, HoldArgs> : sample_step_kernel<float, true, true, HoldArgs>)
                          : (f64 ? sample_step_kernel<double, false, true, HoldArgs> : sample_step_kernel<float, false, true, HoldArgs>);
  const auto tstep_h = pri ? (f64 ? sample_step_tempered_kernel<double, true, true, HoldArgs> : sample_step_tempered_kernel<float, true, true, HoldArgs>)
                           : (f64 ? sample_step_tempered_kernel<double, false, true, HoldArgs>
                                  : sample_step_tempered_kernel<float, false, true, HoldArgs>);
  const auto finish_h = f64 ? sample_finish_kernel<double, true, HoldArgs> : sample_finish_kernel<float, true, HoldArgs>;
  TemperArgs ta{};
  TemperRow* tr = nullptr;
  dim3 tgrid(1);
  if (tp) {
    // whole ladders per workgroup; the rows' tempered sums start at zero
    ta.T = tp->n_temps; ta.swap_every = tp->swap_every; ta.rows_per_wg = 256 / tp->n_temps * tp->n_temps;
    for (int k = 0; k < tp->n_temps; ++k) ta.betas[k] = tp->betas[k];
    tgrid = dim3((unsigned)((n + ta.rows_per_wg - 1) / ta.rows_per_wg));
    CHK(m->tmp.reserve((size_t)n));
    tr = m->tmp.get();
    HIPCHK(hipMemsetAsync(tr, 0, (size_t)n * sizeof(TemperRow), st));
  }
  for (long long it = 0; it <= a.total; ++it) {
    CHK(reduce_run(m, route, n, F, l, g, nullptr, data.d, data.ld, data.rpd, row0, prec, flags & ~V21_FWD_IN_TRANSFORM));
    if (tp && rec.hold)
      hipLaunchKernelGGL(tstep_h, tgrid, dim3(256), 0, st, cs, tr, m->jxt.get(), (const float*)l, (const float*)g, (const float*)F, it, a, ta,
                         rec.pr, rec.ho);
    else if (tp)
      hipLaunchKernelGGL(tstep, tgrid, dim3(256), 0, st, cs, tr, m->jxt.get(), (const float*)l, (const float*)g, (const float*)F, it, a, ta,
                         rec.pr);
    else if (rec.hold)
      hipLaunchKernelGGL(step_h, grid, dim3(256), 0, st, cs, m->jxt.get(), (const float*)l, (const float*)g, (const float*)F, it, a, rec.pr,
                         rec.ho);
    else
      hipLaunchKernelGGL(step, grid, dim3(256), 0, st, cs, m->jxt.get(), (const float*)l, (const float*)g, (const float*)F, it, a, rec.pr);
    HIPCHK(hipGetLastError());
  }
  SampleOutDev od{out.x_last, out.lnl_last, out.eps_last, out.accept_rate, out.mean_u, out.cov_u, out.last_prop_u, out.last_log_alpha};
  if (rec.hold)
    hipLaunchKernelGGL(finish_h, grid, dim3(256), 0, st, (const SampleRow*)cs, (const float*)m->jxt.get(), n, din, (long long)o.n_steps,
                       m->tin, od, rec.ho);
  else
    hipLaunchKernelGGL(finish, grid, dim3(256), 0, st, (const SampleRow*)cs, (const float*)m->jxt.get(), n, din, (long long)o.n_steps, m->tin,
                       od);
  HIPCHK(hipGetLastError());
  if (tp && to && (to->mean_lnl || to->var_lnl || to->swap_accept)) {
    hipLaunchKernelGGL(sample_finish_tempered_kernel, grid, dim3(256), 0, st, (const SampleRow*)cs, (const TemperRow*)tr, n,
                       (long long)o.n_steps, TemperOutDev{to->mean_lnl, to->var_lnl, to->swap_accept});
    HIPCHK(hipGetLastError());
  }
  return V21_OK;
}

int sample_counts(const char* what, int n_steps, int n_warmup, int thin, long long chain0, long long step0) {
  if (n_steps < 0 || n_warmup < 0 || thin < 0)
    return fail(V21_ERR_ARG, "%s: options n_steps %d n_warmup %d thin %d", what, n_steps, n_warmup, thin);
  if (chain0 < 0 || step0 < 0 || step0 + (long long)n_warmup + n_steps >= (1LL << 32))
    return fail(V21_ERR_ARG, "%s: options chain0 %lld step0 %lld (step0 + n_warmup + n_steps < 2^32)", what, chain0, step0);
  return V21_OK;
}

static int sample_check(const v21_sample_opts& o) {
  CHK(sample_counts("sample", o.n_steps, o.n_warmup, o.thin, o.chain0, o.step0));
  if (!(o.eps0 > 0.0) || !std::isfinite(o.eps0) || !(o.ridge > 0.0) || !std::isfinite(o.ridge) || !(o.target_accept > 0.0 && o.target_accept < 1.0))
    return fail(V21_ERR_ARG, "sample: options eps0 %g ridge %g target_accept %g", o.eps0, o.ridge, o.target_accept);
  return V21_OK;
}

int whole_groups(const char* what, const char* noun, long long n, int G, bool per_data, long long n_data) {
  if (n % G != 0) return fail(V21_ERR_ARG, "%s: n = %lld rows are no whole %s of %d", what, n, noun, G);
  if (per_data && (n / n_data) % G != 0)
    return fail(V21_ERR_ARG, "%s: %lld rows per data row are no whole %s of %d", what, n / n_data, noun, G);
  return V21_OK;
}

static v21_temper_opts temper_defaults() {
  v21_temper_opts t{};
  t.n_temps = 1;
  t.betas[0] = 1.0;
  t.swap_every = 0;
  return t;
}

// the ladder, and how the call's n rows (with data: the n / n_data rows of a spectrum) divide into ladders
static int temper_check(const v21_temper_opts& t, long long n, bool has_data, long long n_data) {
  if (t.n_temps < 1 || t.n_temps > 32) return fail(V21_ERR_ARG, "sample_tempered: n_temps = %d (1 .. 32)", t.n_temps);
  for (int k = 0; k < t.n_temps; ++k)
    if (!(t.betas[k] >= 0.0 && t.betas[k] <= 1.0) || (k > 0 && !(t.betas[k] < t.betas[k - 1])))
      return fail(V21_ERR_ARG, "sample_tempered: betas[%d] = %g (inside [0, 1], strictly decreasing)", k, t.betas[k]);
  if (t.swap_every < 0) return fail(V21_ERR_ARG, "sample_tempered: swap_every = %d", t.swap_every);
  return whole_groups("sample_tempered", "ladders", n, t.n_temps, has_data, n_data);
}

static constexpr JacEntry kSample{"sample", kFitMaxIn, true, true}, kSampleTempered{"sample_tempered", kFitMaxIn, true, true};

// The four entries (sample and sample_tempered, temper: null for the first; on the device and from the host) share one
// body each.  What both forms check before any device work (ptrs, ldx: jac_args); o and t: the options in force
static int sample_args(v21_mlp* m, bool ptrs, long long ldx, int x_dtype, long long n, bool has_data, long long n_data,
                       const v21_sample_opts* opts, const v21_temper_opts* temper, bool tempered, int precision, int& flags,
                       v21_sample_opts* o, v21_temper_opts* t) {
  *o = opts ? *opts : sample_defaults();
  *t = temper ? *temper : temper_defaults();
  const JacEntry& entry = tempered ? kSampleTempered : kSample;
  CHK(jac_args(m, ptrs, n, ldx, kNoPitch, x_dtype, precision, flags, entry));
  CHK(call_data_args(entry.name, n, has_data, n_data));
  CHK(sample_check(*o));
  return tempered ? temper_check(*t, n, has_data, n_data) : V21_OK;
}

static int sample_dev(v21_mlp* m, const float* d_x0, long long ldx, long long n, const float* d_data, long long n_data,
                      const v21_sample_opts* opts, const v21_temper_opts* temper, bool tempered, const double* d_eps_start,
                      const v21_sample_out* out, const v21_temper_out* tout, int precision, int flags) {
  v21_sample_opts o;
  v21_temper_opts t;
  CHK(sample_args(m, d_x0 && out && out->x_last, ldx, V21_DTYPE_F32, n, d_data != nullptr, n_data, opts, temper, tempered, precision, flags, &o, &t));
  if (n == 0) return V21_OK;
  CallData data;
  CHK(call_data(m, n, d_data, false, n_data, &data));
  const int route = jac_route(m, precision, flags, m->dims[m->L]);
  CHK(jac_prep(m, d_x0, V21_DTYPE_F32, ldx, n, 1));
  return sample_run(m, route, n, data, 0, o, o.chain0, d_eps_start, precision, flags, *out, V21_DTYPE_F32, tempered ? &t : nullptr, tout);
}

// the host forms: chunks of kJacHostChunk chains -- of a tempered call the largest multiple of n_temps that is not above
// it: no ladder straddles two chunks --, each staged (ChunkStage), run by sample_run and copied back
static int sample_host(v21_mlp* m, const void* x0, int x_dtype, long long n, const float* data, long long n_data, const v21_sample_opts* opts,
                       const v21_temper_opts* temper, bool tempered, const double* eps_start, const v21_sample_out* out,
                       const v21_temper_out* tout, int precision, int flags) {
  v21_sample_opts o;
  v21_temper_opts tp;
  CHK(sample_args(m, x0 && out && out->x_last, kNoPitch, x_dtype, n, data != nullptr, n_data, opts, temper, tempered, precision, flags, &o, &tp));
  if (n == 0) return V21_OK;
  CallData cd;
  CHK(call_data(m, n, data, true, n_data, &cd));
  const int din = m->dims[0], dout = m->dims[m->L];
  const int route = jac_route(m, precision, flags, dout);
  ChunkStage sg;
  double* d_eps = nullptr;
  v21_sample_out d{};
  v21_temper_out t{};
  sg.add(eps_start, &d_eps, sizeof(double), true);
  stage_sampler_out(sg, *out, d, sample_keep(o.n_steps, o.thin), din, x_dtype == V21_DTYPE_F64 ? sizeof(double) : sizeof(float));
  sg.add(out->eps_last, &d.eps_last, sizeof(double));
  if (tempered && tout) {
    sg.add(tout->mean_lnl, &t.mean_lnl, sizeof(double));
    sg.add(tout->var_lnl, &t.var_lnl, sizeof(double));
    sg.add(tout->swap_accept, &t.swap_accept, sizeof(double));
  }
  return jac_chunks(m, x0, x_dtype, n, 1, sg, [&](long long r0, long long rows) {
    return sample_run(m, route, rows, cd, r0, o, o.chain0 + r0, d_eps, precision, flags, d, x_dtype, tempered ? &tp : nullptr, &t);
  }, tempered ? kJacHostChunk / tp.n_temps * tp.n_temps : kJacHostChunk);
}

extern "C" int v21_mlp_sample_dev(v21_mlp* m, const float* d_x0, int64_t ldx, int64_t n, const float* d_data, int64_t n_data,
                                  const v21_sample_opts* opts, const double* d_eps_start, const v21_sample_out* out, int precision, int flags) {
  return sample_dev(m, d_x0, ldx, n, d_data, n_data, opts, nullptr, false, d_eps_start, out, nullptr, precision, flags);
}

extern "C" int v21_mlp_sample(v21_mlp* m, const void* x0, int x_dtype, int64_t n, const float* data, int64_t n_data, const v21_sample_opts* opts,
                              const double* eps_start, const v21_sample_out* out, int precision, int flags) {
  return sample_host(m, x0, x_dtype, n, data, n_data, opts, nullptr, false, eps_start, out, nullptr, precision, flags);
}

// ---- parallel tempering (include/v21.h: v21_mlp_sample_tempered[_dev]; temper NULL: one rung at beta = 1)
extern "C" int v21_mlp_sample_tempered_dev(v21_mlp* m, const float* d_x0, int64_t ldx, int64_t n, const float* d_data, int64_t n_data,
                                           const v21_sample_opts* opts, const v21_temper_opts* temper, const double* d_eps_start,
                                           const v21_sample_out* out, const v21_temper_out* tout, int precision, int flags) {
  return sample_dev(m, d_x0, ldx, n, d_data, n_data, opts, temper, true, d_eps_start, out, tout, precision, flags);
}

extern "C" int v21_mlp_sample_tempered(v21_mlp* m, const void* x0, int x_dtype, int64_t n, const float* data, int64_t n_data,
                                       const v21_sample_opts* opts, const v21_temper_opts* temper, const double* eps_start,
                                       const v21_sample_out* out, const v21_temper_out* tout, int precision, int flags) {
  return sample_host(m, x0, x_dtype, n, data, n_data, opts, temper, true, eps_start, out, tout, precision, flags);
}
