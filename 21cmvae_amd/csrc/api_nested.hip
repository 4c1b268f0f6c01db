// api_nested.hip -- the nested sampler on the device (include/v21.h: v21_mlp_sample_nested[_dev], v21_route_nested):
// evidence and weighted posterior samples from forward-only ln L (nested_kernels.h).  The loop is the ensemble
// sampler's (api_ensemble.hip): the live points stay on the device, every move is one evaluation of the n / 2 pending
// proposals in their compacted layout by lnl_run of api_loglike.hip (on u, without the input transform) and one
// nested_step_kernel launch, and the host only launches.  Routes: csrc/routes.h (decide_ensemble with N in the place of
// W), decided once per call and counted once by v21_mlp_last_lnl_route.
#include "api_internal.h"
#include "nested_kernels.h"

static v21_nested_opts nested_defaults() {
  v21_nested_opts o;
  o.n_live = 256;
  o.n_repeats = 0;
  o.n_iter = 100;
  o.gamma = 0.0;
  o.seed = 0;
  o.iter0 = 0;
  o.chain0 = 0;
  return o;
}
static int nested_repeats(const v21_nested_opts& o, int din) { return o.n_repeats > 0 ? o.n_repeats : 3 * din; }

// the scale, the counts, and how the call's n rows (with data: the n / n_data rows of a spectrum) divide into runs of N
// live points in din dimensions
static int nested_check(const v21_nested_opts& o, int din, long long n, bool has_data, long long n_data) {
  const int N = o.n_live;
  if (N < kNestMinLive || N % 2 != 0 || N > kEnsMaxWalkers)
    return fail(V21_ERR_ARG, "sample_nested: n_live = %d (even, %d .. %d)", N, kNestMinLive, kEnsMaxWalkers);
  if (!(o.gamma >= 0.0 && o.gamma <= 1e6)) return fail(V21_ERR_ARG, "sample_nested: gamma = %g (0 .. 1e6; 0: the default)", o.gamma);
  if (o.n_repeats < 0 || o.n_iter < 0 || o.iter0 < 0 || o.chain0 < 0)
    return fail(V21_ERR_ARG, "sample_nested: n_repeats = %d, n_iter = %d, iter0 = %lld, chain0 = %lld (none negative)", o.n_repeats, o.n_iter,
                o.iter0, o.chain0);
  if (o.iter0 >= (1ll << 32) || (o.iter0 + o.n_iter) * (long long)nested_repeats(o, din) >= (1ll << 32))
    return fail(V21_ERR_ARG, "sample_nested: (iter0 + n_iter) n_repeats must stay below 2^32");
  return whole_groups("sample_nested", "runs", n, N, has_data && n > 0, n_data);
}

extern "C" int v21_route_nested(int n_layers, const int* dims, const int* act, int precision, int64_t n, int64_t n_data, int n_live,
                                int n_modes, int flags, int host_form, int* route, int64_t* chunk_rows) {
  return ens_route_query("sample_nested", n_layers, dims, act, precision, n, n_data, n_live, n_modes, flags, host_form, route, chunk_rows, [&] {
    v21_nested_opts o = nested_defaults();
    o.n_live = n_live;
    return nested_check(o, dims[0], n, n_data > 0, n_data);
  });
}

// the runs of n rows -- d_start: their start rows (n, din) in u, or nullptr (drawn) -- `out`: device pointers, dead_u and
// live_u of x_dtype, the dead record shaped for the n / N runs of THIS call; the call's first row is global row `chain0`,
// its row `row0` of a call of n_call rows (data rows as in fit_run)
static int nested_run(v21_mlp* m, int route, const float* d_start, long long n, long long n_call, const CallData& data, long long row0,
                      const v21_nested_opts& o, long long chain0, int prec, int flags, const v21_nested_out& out, int x_dtype) {
  hipStream_t st = m->ctx->stream;
  const int din = m->dims[0];
  CHK(m->nst.reserve((size_t)n));
  HalfEval ev;
  CHK(half_eval(m, route, n, n_call, data, row0, prec, flags, &ev));
  NestRow* rows = m->nst.get();
  NestArgs a{};
  a.runs = n / o.n_live; a.din = din; a.N = o.n_live; a.k = o.n_live / 2; a.rpw = 256 / a.k;
  a.R = nested_repeats(o, din);
  a.gamma = (float)(o.gamma > 0.0 ? o.gamma : 2.38 / std::sqrt(2.0 * din));
  a.seed = o.seed; a.chain0 = (uint64_t)chain0; a.iter0 = o.iter0;
  a.dead_u = out.dead_u; a.dead_lnl = out.dead_lnl; a.lstar = out.lstar;
  const dim3 grid((unsigned)((a.runs + a.rpw - 1) / a.rpw));
  // (dead_u and live_u are of x_dtype, the prior record (api_prior.hip) is there or not: one set of instantiations,
  // picked once)
  // ... and so is the hold record (api_hold.hip), which the HOLD instantiations take as their last argument
  const SamplerRecords rec = sampler_records(m);
  const bool f64 = x_dtype == V21_DTYPE_F64, pri = rec.pri;
  const auto step = pri ? (f64 ? nested_step_kernel<double, true, false> : nested_step_kernel<float, true, false>)
                        : (f64 ? nested_step_kernel<double, false, false> : nested_step_kernel<float, false, false>);
  const auto step_h = pri ? (f64 ? nested_step_kernel<double, true, true, HoldArgs> : nested_step_kernel<float, true, true, HoldArgs>)
                          : (f64 ? nested_step_kernel<double, false, true, HoldArgs> : nested_step_kernel<float, false, true, HoldArgs>);
  const auto finish = f64 ? nested_finish_kernel<double> : nested_finish_kernel<float>;
  const long long T = o.n_iter, moves = T * a.R;
  // launch 0 passes start half 0 on, 1 takes it and passes half 1 on, 2 takes that and opens iteration 0; launch 3 + mv
  // decides move mv, opens the next iteration after an iteration's last move, and draws move mv + 1
  for (long long q = 0; q < 3 + moves; ++q) {
    NestLaunch l{-1, 0, -1, 0, -1, -1};
    const long long dec = q >= 3 ? q - 3 : 0;  // the move a deciding launch decides (the prior's acceptance draw)
    if (q == 0) l.start = 0;
    else if (q == 1) { l.take = 0; l.start = 1; }
    else if (q == 2) { l.take = 1; if (T > 0) { l.bt = 0; l.dm = 0; } }
    else {
      const long long mv = q - 3;
      l.decide = 1;
      if (mv + 1 < moves) {
        l.dm = mv + 1;
        if ((mv + 1) % a.R == 0) l.bt = (mv + 1) / a.R;
      }
    }
    if (q > 0) CHK(ev.run(m));
    if (rec.hold)
      hipLaunchKernelGGL(step_h, grid, dim3(256), 0, st, rows, d_start, ev.prop, (const float*)ev.lnl, l, a, rec.pr, dec, rec.ho);
    else
      hipLaunchKernelGGL(step, grid, dim3(256), 0, st, rows, d_start, ev.prop, (const float*)ev.lnl, l, a, rec.pr, dec);
    HIPCHK(hipGetLastError());
  }
  NestOutDev od{out.live_u, out.live_lnl, out.accept_rate, out.last_partner, out.last_prop_u};
  hipLaunchKernelGGL(finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const NestRow*)rows, (const float*)ev.prop, n, din, a.N, moves, od);
  HIPCHK(hipGetLastError());
  return V21_OK;
}

static constexpr JacEntry kNested{"sample_nested", kFitMaxIn, true, false};

extern "C" int v21_mlp_sample_nested_dev(v21_mlp* m, const float* d_x0, int64_t ldx, int64_t n, const float* d_data, int64_t n_data,
                                         const v21_nested_opts* opts, const v21_nested_out* out, int precision, int flags) {
  const v21_nested_opts o = opts ? *opts : nested_defaults();
  CHK(jac_args(m, out && out->live_u, n, d_x0 ? ldx : kNoPitch, kNoPitch, V21_DTYPE_F32, precision, flags, kNested));
  CHK(call_data_args("sample_nested", n, d_data != nullptr, n_data));
  CHK(nested_check(o, m->dims[0], n, d_data != nullptr, n_data));
  if (n == 0) return V21_OK;
  CallData data;
  CHK(call_data(m, n, d_data, false, n_data, &data));
  const EnsRoute r = ens_route(m, precision, d_data ? data.rpd : 0, n, o.n_live, flags, false);
  if (d_x0) CHK(jac_prep(m, d_x0, V21_DTYPE_F32, ldx, n, 0));  // (the rows at pitch in_dim)
  return nested_run(m, r.route, d_x0 ? m->jxt.get() : nullptr, n, n, data, 0, o, o.chain0, precision, flags, *out, V21_DTYPE_F32);
}

// the host form: chunks of whole runs (routes.h: decide_ensemble), each staged (ChunkStage: a unit is a run, the dead
// record one copy per iteration), run by nested_run on the given starts -- x0 null: drawn -- and copied back
extern "C" int v21_mlp_sample_nested(v21_mlp* m, const void* x0, int x_dtype, int64_t n, const float* data, int64_t n_data,
                                     const v21_nested_opts* opts, const v21_nested_out* out, int precision, int flags) {
  const v21_nested_opts o = opts ? *opts : nested_defaults();
  CHK(jac_args(m, out && out->live_u, n, kNoPitch, kNoPitch, x_dtype, precision, flags, kNested));
  CHK(call_data_args("sample_nested", n, data != nullptr, n_data));
  CHK(nested_check(o, m->dims[0], n, data != nullptr, n_data));
  if (n == 0) return V21_OK;
  CallData cd;
  CHK(call_data(m, n, data, true, n_data, &cd));
  const EnsRoute r = ens_route(m, precision, data ? cd.rpd : 0, n, o.n_live, flags, true);
  const int din = m->dims[0], N = o.n_live, k = N / 2;
  const long long T = o.n_iter;
  const size_t esz = x_dtype == V21_DTYPE_F64 ? sizeof(double) : sizeof(float);
  ChunkStage sg;
  sg.unit = N;
  v21_nested_out d{};
  sg.add(out->dead_u, &d.dead_u, (size_t)k * din * esz, false, T);
  sg.add(out->dead_lnl, &d.dead_lnl, (size_t)k * sizeof(float), false, T);
  sg.add(out->lstar, &d.lstar, sizeof(float), false, T);
  sg.add(out->live_u, &d.live_u, (size_t)N * din * esz);
  sg.add(out->live_lnl, &d.live_lnl, (size_t)N * sizeof(float));
  sg.add(out->accept_rate, &d.accept_rate, (size_t)k * sizeof(double));
  sg.add(out->last_partner, &d.last_partner, (size_t)k * 2 * sizeof(int));
  sg.add(out->last_prop_u, &d.last_prop_u, (size_t)k * din * sizeof(float));
  return jac_chunks(m, x0, x_dtype, n, 0, sg, [&](long long r0, long long rows) {
    return nested_run(m, r.route, x0 ? m->jxt.get() : nullptr, rows, n, cd, r0, o, o.chain0 + r0, precision, flags, d, x_dtype);
  }, r.chunk);
}
