// api_sweep.hip -- v21_sweep_*: several models stepped in lock step with grouped launches (BASELINE configs[4]).
#include "api_internal.h"

// ---------------------------------------------------------------------------------
// sweep: G independent models, ONE shared batch stream, one launch per phase for all of them
// (BASELINE configs[4]: "64 concurrent latent-dim/hidden-width configs packed as batched
// GEMM", 8 per GPU; no reference code -- the reference trains one model at a time,
// emulator.py:739-747).  The models share depth, activations and in/out width; hidden and
// latent widths differ.  Phase k of a step is the same kind of kernel for every model, so it
// becomes one grouped launch (gemm_nt.h: NtGroup; train_kernels.h: *_group_kernel).
// ---------------------------------------------------------------------------------
struct v21_sweep {
  v21_ctx* ctx = nullptr;
  std::vector<v21_trainer*> tr;
  Dev<AdamArgs> d_adam;
  std::vector<AdamArgs> h_adam;  // what d_adam holds
  bool chain = false;            // every member runs the chain kernel: one grouped launch of it per step
  Dev<ChainModel> d_chain;
  std::vector<ChainModel> h_chain;
  Dev<DwAdamModel> d_dwadam;  // single rank: gradients + Adam in one grouped launch (dw_adam.h)
  std::vector<DwAdamModel> h_dwadam;
  // f32 members on the small-batch chain (train_chain32s.h): one grouped chain launch + one grouped gradient / Adam launch
  // (dw_adam32.h) per step on a single rank, steps of <= kDw32MaxRows rows
  bool chain32s = false;
  Dev<Dw32Model> d_dw32;
  std::vector<Dw32Model> h_dw32;
  // r5: TWO half-groups on two streams (one rank, grouped chain launches).  A group step is two launches of complementary
  // character -- every member's chain (latency-bound per workgroup, little HBM traffic) and every member's gradients + Adam
  // (bound by the optimizer state's bytes: 390 MB per step of 32 members at 3.85 TB/s) -- and the members are independent
  // models: half B's chain runs while half A's Adam launch waits for HBM.  Same kernels on the same data per member:
  // bit-identical results.  Measured (one MI355X, f16, batch 256; gpurun_out/r5_sweep_f16_c.txt against r5_b5.json): 16 members
  // 159-163 k -> 167 k model-steps/s, 64 members 170-173 k -> 180 k, 8 and 32 members within noise -- the two streams drift back
  // into lock step (two Adam launches that share the HBM end together, then both chains start together).  Forcing the
  // anti-phase order with events (A's Adam launch, then B's, then A's ...) was measured SLOWER (32 members: 183 against 168 us
  // per group step: every cross-stream dependency is a ~5-us hand-over); two host threads on two contexts reached 148 us
  // (scripts/diag/sweep_two_streams_probe.py) -- the kernels' own sum (44.6 + 101 us): what is left is enqueue jitter, not overlap.
  hipStream_t s2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_off = nullptr, ev_join = nullptr;
};

extern "C" int v21_sweep_create(v21_trainer** trainers, int count, v21_sweep** out) {
  if (!trainers || !out) return fail(V21_ERR_ARG, "null argument");
  if (count < 1 || count > kSweepMax) return fail(V21_ERR_ARG, "count %d not in [1,%d]", count, kSweepMax);
  v21_trainer* t0 = trainers[0];
  if (!t0) return fail(V21_ERR_ARG, "null trainer");
  const v21_mlp* m0 = t0->mlp;
  for (int k = 0; k < count; ++k) {
    v21_trainer* t = trainers[k];
    if (!t) return fail(V21_ERR_ARG, "null trainer");
    const v21_mlp* m = t->mlp;
    if (t->ctx != t0->ctx || t->prec != t0->prec || t->max_batch != t0->max_batch)
      return fail(V21_ERR_ARG, "model %d: context, precision and max_batch must match model 0", k);
    if (m->L != m0->L || m->act != m0->act || m->dims[0] != m0->dims[0] || m->dims[m->L] != m0->dims[m0->L])
      return fail(V21_ERR_ARG, "model %d: depth, activations and in/out width must match model 0", k);
    if (t->kind.gl >= 0 && !t->kind.chain && !(t->kind.chain32 && t->kind.chain32s))
      return fail(V21_ERR_UNSUPPORTED, "variational stacks are swept on the chain kernels only (f16 / bf16, or f32 with max_batch <= %d; latent <= %d)",
                  kC32sMaxBatch, kChainMaxLatent);
    for (int j = 0; j < k; ++j)
      if (trainers[j] == t) return fail(V21_ERR_ARG, "trainer %d listed twice", k);
  }
  CHK(use(t0->ctx));
  std::unique_ptr<v21_sweep> s(new v21_sweep());
  s->ctx = t0->ctx;
  s->tr.assign(trainers, trainers + count);
  CHK(s->d_adam.reserve(count));
  s->chain = true;
  for (int k = 0; k < count; ++k) s->chain = s->chain && trainers[k]->kind.chain;
  for (int k = 0; k < count; ++k) s->h_adam.push_back(adam_args(trainers[k], true, 0.f, s->chain));
  HIPCHK(hipMemcpyAsync(s->d_adam, s->h_adam.data(), s->h_adam.size() * sizeof(AdamArgs), hipMemcpyHostToDevice, s->ctx->stream));
  s->chain32s = !s->chain;
  for (int k = 0; k < count; ++k) s->chain32s = s->chain32s && trainers[k]->kind.chain32s && trainers[k]->mlp->L <= kNtMaxGroup;
  if (s->chain || s->chain32s) CHK(s->d_chain.reserve(count));
  if (s->chain32s) CHK(s->d_dw32.reserve(count));
  HIPCHK(hipStreamSynchronize(s->ctx->stream));
  *out = s.release();
  return V21_OK;
}
extern "C" int v21_sweep_destroy(v21_sweep* s) {
  if (!s) return V21_OK;
  hipSetDevice(s->ctx->device);
  hipStreamSynchronize(s->ctx->stream);
  if (s->s2) { hipStreamSynchronize(s->s2); hipStreamDestroy(s->s2); }
  for (hipEvent_t e : {s->ev_fork, s->ev_off, s->ev_join}) if (e) hipEventDestroy(e);
  delete s;
  return V21_OK;
}

// the end of a sweep step that did not take a one-launch update: every model's gradients summed over the ranks (its loss
// then into the epoch's table: a rank without rows takes part, so this is the only writer), Adam of every model in one
// launch, the packed copies (nt_ok: the fp32 NT copies too)
static int sweep_adam(v21_sweep* s, long long step_index, bool nt_ok) {
  hipStream_t st = s->ctx->stream;
  const int G = (int)s->tr.size();
  AlphaGroup al{};
  size_t maxP = 0;
  for (int k = 0; k < G; ++k) {
    v21_trainer* t = s->tr[k];
    CHK(v21_comm_allreduce_f32(t->ctx, t->d_g, t->P + 1));
    if (s->ctx->nranks > 1 && step_index >= 0)
      HIPCHK(hipMemcpyAsync(t->d_steploss + step_index, t->d_g + t->P, sizeof(float), hipMemcpyDeviceToDevice, st));
    t->iter += 1;
    al.a[k] = adam_alpha(t->adam, t->iter);
    maxP = std::max(maxP, t->P);
  }
  hipLaunchKernelGGL(adam_repack_group_kernel, dim3((unsigned)((maxP + 255) / 256), G), dim3(256), 0, st,
                     (const AdamArgs*)s->d_adam, al);
  HIPCHK(hipGetLastError());
  for (v21_trainer* t : s->tr) weights_updated(t, nt_ok);
  return V21_OK;
}
// one optimizer step of every model on the batch gathered into model 0's h[0]/ht[0]/yb/wb
static int sweep_step(v21_sweep* s, const float* yb, long long ldy, int rows, int brows, long long step_index) {
  v21_trainer* t0 = s->tr[0];
  hipStream_t st = s->ctx->stream;
  const int G = (int)s->tr.size(), L = t0->mlp->L, dout = t0->mlp->dims[L];
  if (rows > t0->max_batch) return fail(V21_ERR_ARG, "batch of %d rows exceeds max_batch %d", rows, t0->max_batch);
  if (rows > 0) {
    for (v21_trainer* t : s->tr) CHK(ensure_copies(t));
    std::vector<NtArgs> probs;
    for (int l = 0; l < L; ++l) {  // forward, layer l of every model
      probs.clear();
      for (v21_trainer* t : s->tr) probs.push_back(nt_forward(t, l, l == 0 ? t0->d_h[0] : t->d_h[l], rows, true));
      CHK(launch_nt_many(t0->prec, probs, st));
    }
    LossGroup lg{};
    SumGroup sg{};
    for (int k = 0; k < G; ++k) {
      v21_trainer* t = s->tr[k];
      lg.p[k] = t->d_h[L]; lg.ldp[k] = p16(dout);
      lg.dz[k] = t->d_dz[L]; lg.lddz[k] = p16(dout);
      lg.dzt[k] = t->d_dzt[L]; lg.rowloss[k] = t->d_rowloss;
      sg.v[k] = t->d_rowloss; sg.out[k] = t->d_g + t->P;
      sg.out2[k] = (s->ctx->nranks == 1 && step_index >= 0) ? t->d_steploss + step_index : nullptr;
    }
    lg.y = yb; lg.ldy = ldy; lg.w = t0->d_wb; lg.ldt = t0->Bp; lg.n = rows; lg.d = dout;
    lg.scale = 2.0f / (float)brows;
    sg.n = rows;
    hipLaunchKernelGGL(loss_grad_t_group_kernel, dim3((rows + 3) / 4, G), dim3(256), 0, st, lg);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(sum_group_kernel, dim3(G), dim3(256), 0, st, sg);
    HIPCHK(hipGetLastError());
    const NtSlices sl = nt_slices(rows, false);
    const float gs = grad_opscale(brows, dout);
    for (int l = L - 1; l >= 0; --l) {  // backward, layer l of every model: dW (and dX below the top)
      probs.clear();
      for (v21_trainer* t : s->tr) {
        probs.push_back(nt_dw(t, l, l == 0 ? t0->d_ht[0] : t->d_ht[l], t->d_dzt[l + 1], rows, sl, gs));
        if (l > 0) probs.push_back(nt_dx(t, l, t->d_dz[l + 1], rows, gs));
      }
      CHK(launch_nt_many(t0->prec, probs, st));
    }
    if (sl.nslice > 1)
      for (v21_trainer* t : s->tr) CHK(reduce_slabs(t, sl.nslice));
  } else {
    for (v21_trainer* t : s->tr) CHK(zero_grad(t));
  }
  return sweep_adam(s, step_index, true);
}

// chain form of a sweep step: ONE launch carries every model's rows through forward, loss and the
// activation-gradient chain (blockIdx.y = model); then all weight gradients, then all Adam updates
// members [g0, g1) of the group on stream `st`: the chain of each, and (one rank) their gradients + Adam
static int sweep_chain_launch(v21_sweep* s, const ChainStep& csp, int g0, int g1, hipStream_t st) {
  v21_trainer* t0 = s->tr[0];
  const int G = g1 - g0;
  // one-dimensional grid: a model's row blocks share an XCD label (train_chain.h: train_chain_group_kernel)
  const dim3 grid(8 * csp.ncons * ((G + 7) / 8)), block(64 * kChainWaves);
  bool gauss = false;  // (train_chain.h: FEAT)
  for (int k = g0; k < g1; ++k) gauss = gauss || s->tr[k]->kind.gl >= 0;
  const ChainModel* tab = (const ChainModel*)s->d_chain + g0;
  V21_CHAIN_LAUNCH(train_chain_group_kernel, PrecF16, PrecBF16, t0->prec == V21_PREC_F16, gauss, kChainLdsBytes, grid, block, st, tab, csp, G);
  HIPCHK(hipGetLastError());
  return V21_OK;
}
// two streams, the epoch's first step: half B starts after half A's chain launch -- the offset that makes B's chain meet
// A's Adam launch, not A's chain
static int sweep_offset(v21_sweep* s) {
  HIPCHK(hipEventRecord(s->ev_off, s->ctx->stream));
  HIPCHK(hipStreamWaitEvent(s->s2, s->ev_off, 0));
  return V21_OK;
}
static int sweep_dwadam_launch(v21_sweep* s, int g0, int g1, int rows, int brows, long long step_index, hipStream_t st) {
  const std::vector<v21_trainer*> part(s->tr.begin() + g0, s->tr.begin() + g1);
  const std::vector<DwAdamModel> hpart(s->h_dwadam.begin() + g0, s->h_dwadam.begin() + g1);
  return launch_dw_adam_group(part, s->d_dwadam + g0, hpart, rows, brows, step_index, st);
}
static int sweep_step_chain(v21_sweep* s, const ChainStep& cs, int brows, long long step_index, const SweepShape& sh, const RouteEnv& env) {
  v21_trainer* t0 = s->tr[0];
  hipStream_t st = s->ctx->stream;
  const int G = (int)s->tr.size(), rows = cs.rows;
  if (rows > t0->max_batch) return fail(V21_ERR_ARG, "batch of %d rows exceeds max_batch %d", rows, t0->max_batch);
  if (rows > 0) {
    for (v21_trainer* t : s->tr) CHK(ensure_copies(t, false));
    CHK(chain_attr(t0->prec));
    ChainStep csp = cs;
    const ChainLaunch p = plan_chain16(rows, 0, env);  // (no prefetcher workgroups in a sweep)
    csp.ncons = p.ncons; csp.npref = p.npref;
    if (sh.two_streams) {  // one rank: half A on the context's stream, half B on the second one, B one launch behind A
      const int GA = (G + 1) / 2;
      CHK(sweep_chain_launch(s, csp, 0, GA, st));
      if (step_index == 0) CHK(sweep_offset(s));
      CHK(sweep_chain_launch(s, csp, GA, G, s->s2));
      CHK(sweep_dwadam_launch(s, 0, GA, rows, brows, step_index, st));
      return sweep_dwadam_launch(s, GA, G, rows, brows, step_index, s->s2);
    }
    CHK(sweep_chain_launch(s, csp, 0, G, st));
    if (s->ctx->nranks == 1)  // nothing to exchange: all gradients, all Adam updates, all packed copies in one launch
      return launch_dw_adam_group(s->tr, s->d_dwadam, s->h_dwadam, rows, brows, step_index, st);
    int nslice = 1;  // data-parallel ranks: every model's gradients in one launch, the exchange, Adam
    std::vector<Dw16Args> probs;
    for (v21_trainer* t : s->tr) dw16_problems(t, rows, brows, &nslice, probs);
    CHK(launch_dw16(t0->prec, probs, st));
    if (nslice > 1)
      for (v21_trainer* t : s->tr) CHK(reduce_slabs(t, nslice));
  } else {
    for (v21_trainer* t : s->tr) CHK(zero_grad(t));
  }
  return sweep_adam(s, step_index, false);
}

// f32 members (train_chain32s.h): the problem and Adam blocks of one model's gradient launch, as a step of the trainer
// builds them (dw32_model) -- without what changes from step to step (contraction length, step size, loss slot: Dw32Step).
// false: this model's gradient launch would take 64 x 64 tiles (routes.h: dw32_tile; gemm_nt_dwadam_kernel<2>): the sweep
// then keeps the per-layer path, so that a member trains bit for bit as it would on its own.
static bool build_dw32_model(v21_trainer* t, Dw32Model& md, int& blocks) {
  const v21_mlp* m = t->mlp;
  md = Dw32Model{};
  blocks = 0;
  if (m->L > kNtMaxGroup || dw32_tile(m->L, m->dims.data(), m->act.data()) != 32) return false;
  blocks = dw32_model(t, 32, md);
  return true;
}
// every weight gradient + Adam + packed streams + batch loss of several f32 models in one launch (dw_adam32.h)
// small_slabs: the 128-row instantiation (dw_adam32.h: SLAB) -- decided by the caller for the WHOLE sweep, not per launch: a
// member must see the same sums whether its half-group or the whole group is launched
int launch_dw32_group(const std::vector<v21_trainer*>& trs, const Dw32Model* d_tab, int rows, long long step_index, int max_blocks,
                             hipStream_t st, bool small_slabs) {
  const int G = (int)trs.size();
  Dw32Step ds{};
  ds.rows = rows; ds.slot = (int)step_index;
  for (int k = 0; k < G; ++k) {
    v21_trainer* t = trs[k];
    t->iter += 1;
    ds.alpha[k] = adam_alpha(t->adam, t->iter);
  }
  if (small_slabs) hipLaunchKernelGGL(dwadam32_group_kernel<128>, dim3(max_blocks, G), dim3(256), 0, st, d_tab, ds);
  else hipLaunchKernelGGL(dwadam32_group_kernel<256>, dim3(max_blocks, G), dim3(256), 0, st, d_tab, ds);
  HIPCHK(hipGetLastError());
  for (v21_trainer* t : trs) weights_updated(t, false);
  return V21_OK;
}
// builds / refreshes the device table of launch_dw32_group; *ok = false: a member's gradient launch takes 64 x 64 tiles
int refresh_dw32_table(const std::vector<v21_trainer*>& trs, Dw32Model* d_tab, std::vector<Dw32Model>& h_tab, int* max_blocks, bool* ok,
                              hipStream_t st) {
  std::vector<Dw32Model> dtab(trs.size());
  *max_blocks = 0; *ok = true;
  for (size_t k = 0; k < trs.size(); ++k) {
    int blocks = 0;
    *ok = *ok && build_dw32_model(trs[k], dtab[k], blocks);
    *max_blocks = std::max(*max_blocks, blocks);
  }
  if (!*ok) return V21_OK;
  return upload_if_changed(dtab, h_tab, d_tab, st);
}
// one optimizer step of every f32 member in TWO launches: the chain of every model (blockIdx.y = model), then every
// weight gradient + Adam + packed streams + batch loss
static int sweep_chain32_launch(v21_sweep* s, const ChainStep& csp, int rpw, int g0, int g1, hipStream_t st) {
  const int G = g1 - g0;
  const dim3 grid(csp.ncons * G), block(64 * kC32sWaves);
  bool gauss = false;
  for (int k = g0; k < g1; ++k) gauss = gauss || s->tr[k]->kind.gl >= 0;
  const ChainModel* tab = (const ChainModel*)s->d_chain + g0;
  V21_CHAIN_LAUNCH(train_chain32s_group_kernel, 4, 8, rpw == 4, gauss, kC32sLdsBytes, grid, block, st, tab, csp, G);
  HIPCHK(hipGetLastError());
  return V21_OK;
}
static int sweep_step_chain32(v21_sweep* s, const ChainStep& cs, long long step_index, int max_blocks, const SweepShape& sh, const RouteEnv& env) {
  hipStream_t st = s->ctx->stream;
  const int G = (int)s->tr.size(), rows = cs.rows;
  for (v21_trainer* t : s->tr) CHK(ensure_copies(t, false));
  CHK(chain_attr(V21_PREC_F32));
  // 4 rows per workgroup while every model's row blocks fit the chip in one round (routes.h: c32s_rows)
  const ChainLaunch p = plan_chain32s(rows, G, 0, env);
  const int rpw = p.rows_per_wg;
  ChainStep csp = cs;
  csp.ncons = p.ncons; csp.npref = p.npref;
  if (sh.two_streams) {  // (as sweep_step_chain: half B one launch behind half A)
    const int GA = (G + 1) / 2;
    const std::vector<v21_trainer*> pa(s->tr.begin(), s->tr.begin() + GA), pb(s->tr.begin() + GA, s->tr.end());
    CHK(sweep_chain32_launch(s, csp, rpw, 0, GA, st));
    if (step_index == 0) CHK(sweep_offset(s));
    CHK(sweep_chain32_launch(s, csp, rpw, GA, G, s->s2));
    CHK(launch_dw32_group(pa, s->d_dw32, rows, step_index, max_blocks, st, sh.small_slabs));
    return launch_dw32_group(pb, s->d_dw32 + GA, rows, step_index, max_blocks, s->s2, sh.small_slabs);
  }
  CHK(sweep_chain32_launch(s, csp, rpw, 0, G, st));
  return launch_dw32_group(s->tr, s->d_dw32, rows, step_index, max_blocks, st, sh.small_slabs);
}

extern "C" int v21_sweep_run_epoch(v21_sweep* s, const int32_t* perm, int batch, double* losses) {
  if (!s || !losses) return fail(V21_ERR_ARG, "null argument");
  v21_trainer* t0 = s->tr[0];
  if (t0->n[0] < 1) return fail(V21_ERR_STATE, "model 0 holds the training set of the sweep: none set");
  CHK(use(s->ctx));
  hipStream_t st = s->ctx->stream;
  v21_mlp* m = t0->mlp;
  const long long n = t0->n[0];
  const int R = s->ctx->nranks;
  if (batch < 1) return fail(V21_ERR_ARG, "batch must be >= 1");
  if ((batch + R - 1) / R > t0->max_batch) return fail(V21_ERR_ARG, "per-rank batch %d exceeds max_batch %d", (batch + R - 1) / R, t0->max_batch);
  const int* d_idx = nullptr;
  CHK(upload_rows(t0, perm, &d_idx));
  const long long steps = (n + batch - 1) / batch;
  for (v21_trainer* t : s->tr) CHK(ensure_steploss(t, steps));
  // the Adam hyper-parameters may have changed since create (set_adam / set_lr): refresh the device table
  std::vector<AdamArgs> tab;
  for (v21_trainer* t : s->tr) tab.push_back(adam_args(t, true, 0.f, s->chain));
  CHK(upload_if_changed(tab, s->h_adam, s->d_adam.get(), st));
  const int din = m->dims[0], dout = m->dims[m->L];
  if (s->chain) {
    std::vector<ChainModel> tab;
    for (v21_trainer* t : s->tr) tab.push_back(chain_model(t));
    CHK(upload_if_changed(tab, s->h_chain, s->d_chain.get(), st));
    if (R == 1) CHK(refresh_dw_adam_table(s->tr, s->d_dwadam, s->h_dwadam, st));
  }
  const RouteEnv env = RouteEnv::read();  // the epoch's shape (routes.h); the tile check in between needs the models
  bool group32 = decide_group32(s->chain32s, R, batch, env.sweep32_group);
  int max_blocks32 = 0;
  if (group32) CHK(refresh_dw32_table(s->tr, s->d_dw32, s->h_dw32, &max_blocks32, &group32, st));
  const SweepShape sh = decide_sweep(s->chain || group32, (int)s->tr.size(), R, env);
  if (!s->chain && !group32)
    for (v21_trainer* t : s->tr)
      if (t->kind.gl >= 0)
        return fail(V21_ERR_UNSUPPORTED, "a sweep of variational f32 models takes the grouped chain launches only: one rank, batches of <= %d rows",
                    kDw32MaxRows);
  if (group32) {
    std::vector<ChainModel> tab;
    for (v21_trainer* t : s->tr) {
      tab.push_back(chain_model32(t));
      tab.back().stamps = nullptr;
    }
    CHK(upload_if_changed(tab, s->h_chain, s->d_chain.get(), st));
  }
  // r5: two half-groups on two streams (v21_sweep: s2) for the grouped chain launches of one rank; V21_SWEEP_STREAMS=1: one stream
  if (sh.two_streams) {
    if (!s->s2) {
      HIPCHK(hipStreamCreateWithFlags(&s->s2, hipStreamNonBlocking));
      for (hipEvent_t* e : {&s->ev_fork, &s->ev_off, &s->ev_join}) HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    for (v21_trainer* t : s->tr) CHK(ensure_copies(t, false));  // (a stale member's refresh runs on the context's stream: before the fork)
    HIPCHK(hipEventRecord(s->ev_fork, st));                        // the row table, the tables and the copies are in place
    HIPCHK(hipStreamWaitEvent(s->s2, s->ev_fork, 0));
  }
  for (long long sidx = 0; sidx < steps; ++sidx) {
    const EpochBatch b = epoch_batch(s->ctx, n, batch, sidx);
    const long long lo = b.lo, first = b.first;
    const int rows = b.rows, brows = b.brows;
    if (s->chain) {
      ChainStep cs = chain_step(t0->d_x[0], din, t0->y_is_x[0] ? nullptr : t0->d_y[0], dout, t0->d_rw[0], d_idx, lo, rows,
                                brows, dout, nullptr, lo - first);
      cs.step_off = (unsigned long long)sidx;  // the table holds every model's step counter as of the epoch's start
      CHK(sweep_step_chain(s, cs, brows, sidx, sh, env));
      continue;
    }
    if (group32) {
      ChainStep cs = chain_step(t0->d_x[0], din, t0->y_is_x[0] ? nullptr : t0->d_y[0], dout, t0->d_rw[0], d_idx, lo, rows,
                                brows, dout, nullptr, lo - first);
      cs.gs = 1.0f;  // fp32 operands: no scaling of the gradients
      cs.step_off = (unsigned long long)sidx;  // the table holds every model's step counter as of the epoch's start (noise key)
      CHK(sweep_step_chain32(s, cs, sidx, max_blocks32, sh, env));
      continue;
    }
    if (rows > 0)
      CHK(gather_batch(t0, t0->d_x[0], din, t0->y_is_x[0] ? nullptr : t0->d_y[0], dout, t0->d_rw[0], d_idx, lo, rows));
    const float* yb = t0->y_is_x[0] ? t0->d_h[0] : t0->d_yb;
    CHK(sweep_step(s, yb, t0->y_is_x[0] ? p16(din) : p16(dout), rows, brows, sidx));
  }
  if (sh.two_streams) {  // half B's launches end before the losses are read (and before anything else touches its members)
    HIPCHK(hipEventRecord(s->ev_join, s->s2));
    HIPCHK(hipStreamWaitEvent(st, s->ev_join, 0));
  }
  return epoch_losses(s->tr, steps, n, losses);
}
