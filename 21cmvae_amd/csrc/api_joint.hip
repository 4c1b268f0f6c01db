// api_joint.hip -- v21_joint_*: autoencoder and latent emulator stepping on the same rows (BASELINE configs[2]).
#include "api_internal.h"

// ---------------------------------------------------------------------------------
// joint step (BASELINE configs[2]: "encoder+decoder+emulator joint train"): the autoencoder
// (signals -> signals, emulator.py:739-747) and the latent emulator (parameters -> latent, :756-764) take one
// optimizer step each on the SAME rows of every batch, and the emulator's targets are the latents the
// encoder produces for those rows in that very step (stop-gradient) instead of the reference's
// encoder.predict() of the finished autoencoder (:753-754).  With the autoencoder frozen (lr = 0) it is
// exactly the reference's phase 2.  One launch carries a row block through both models
// (train_chain_joint_kernel), one grouped launch forms all weight gradients and applies Adam to both models (dw_adam.h).
// ---------------------------------------------------------------------------------
struct v21_joint {
  v21_trainer *ae = nullptr, *em = nullptr;
  v21_ctx* ctx = nullptr;  // (kept: destroying the joint object must not look into trainers that may already be gone)
  int latent_layer = 0;
  Dev<ChainModel> d_tab;
  std::vector<ChainModel> h_tab;
  Dev<DwAdamModel> d_dwadam;  // gradients + Adam of both models in one grouped launch (dw_adam.h)
  std::vector<DwAdamModel> h_dwadam;
  bool f32 = false;  // both trainers on the small-batch f32 chain (train_chain32s.h: train_chain32s_joint_kernel)
  Dev<Dw32Model> d_dw32;  // ... and, on a single rank with steps of <= kDw32MaxRows rows, both models' gradients + Adam in one launch
  std::vector<Dw32Model> h_dw32;
};
extern "C" int v21_joint_create(v21_trainer* ae, v21_trainer* em, int latent_layer, v21_joint** out) {
  if (!ae || !em || !out) return fail(V21_ERR_ARG, "null argument");
  if (ae == em || ae->ctx != em->ctx || ae->prec != em->prec || ae->max_batch != em->max_batch)
    return fail(V21_ERR_ARG, "the two trainers must be distinct and share context, precision and max_batch");
  const bool f32 = ae->kind.chain32s && em->kind.chain32s && em->kind.gl < 0;
  for (const v21_trainer* t : {ae, em})  // (routes.h: route_smooth -- such trainers are per-layer trainers)
    for (int l = 0; l < t->mlp->L; ++l)
      if (act_is_smooth(t->mlp->act[l]))
        return fail(V21_ERR_UNSUPPORTED, "the joint step runs on the chain kernels, which have no %s activation (layer %d of the %s): train the "
                    "two models with their own trainers", act_name(t->mlp->act[l]), l, t == ae ? "autoencoder" : "emulator");
  if (!f32 && (!ae->kind.chain || !em->kind.chain || em->kind.gl >= 0))
    return fail(V21_ERR_UNSUPPORTED, "the joint step runs on the chain kernels: f16 / bf16 (widths <= %d, no variational layer in the emulator), or "
                "f32 with max_batch <= %d (variational head: latent <= %d)", kChainMaxDim, kC32sMaxBatch, kChainMaxLatent);
  const v21_mlp* ma = ae->mlp;
  const v21_mlp* me = em->mlp;
  // the latent layer: linear, or the variational head (V21_ACT_GAUSS) -- the emulator then learns z_mean, what
  // encoder.predict returns (emulator.py:753-754)
  if (latent_layer < 0 || latent_layer >= ma->L - 1 || ma->act[latent_layer] == V21_ACT_RELU || (ae->kind.gl >= 0 && ae->kind.gl != latent_layer))
    return fail(V21_ERR_ARG, "latent_layer %d must be the linear (or variational) layer below the autoencoder's output", latent_layer);
  if (ma->dims[latent_layer + 1] != me->dims[me->L] || ma->dims[latent_layer + 1] > 2 * kChainMaxLatent)
    return fail(V21_ERR_ARG, "latent width %d (autoencoder) vs emulator output %d (at most %d)", ma->dims[latent_layer + 1],
                me->dims[me->L], 2 * kChainMaxLatent);
  if (ma->dims[0] != ma->dims[ma->L]) return fail(V21_ERR_ARG, "the first trainer must be an autoencoder (in == out width)");
  CHK(use(ae->ctx));
  std::unique_ptr<v21_joint> j(new v21_joint());
  j->ae = ae; j->em = em; j->ctx = ae->ctx; j->latent_layer = latent_layer; j->f32 = f32;
  CHK(j->d_tab.reserve(2));
  *out = j.release();
  return V21_OK;
}
extern "C" int v21_joint_destroy(v21_joint* j) {
  if (!j) return V21_OK;
  hipSetDevice(j->ctx->device);
  hipStreamSynchronize(j->ctx->stream);
  delete j;
  return V21_OK;
}
// the chain table of the joint launches: both models, the autoencoder's latent captured; `sample` = 0: no noise drawn
static std::vector<ChainModel> joint_table(const v21_joint* j, int sample) {
  std::vector<ChainModel> tab = j->f32 ? std::vector<ChainModel>{chain_model32(j->ae), chain_model32(j->em)}
                                       : std::vector<ChainModel>{chain_model(j->ae), chain_model(j->em)};
  tab[0].zcap_layer = j->latent_layer;
  if (j->f32) tab[0].stamps = tab[1].stamps = nullptr;
  if (!sample) tab[0].sample = 0;
  return tab;
}
// ONE launch carries `rows` rows through both models (train_chain_joint_kernel / train_chain32s_joint_kernel) in the shape
// routes.h plans; models: what c32s_rows counts (2, or 1 to meet the row blocks of a trainer's own launch)
static int joint_launch(const v21_joint* j, ChainStep& sa, ChainStep& sb, long long rows, int models, const RouteEnv& env) {
  const v21_trainer* ta = j->ae;
  hipStream_t st = ta->ctx->stream;
  const ChainLaunch p = j->f32 ? plan_chain32s(rows, models, 0, env) : plan_chain16(rows, 2, env);
  sa.ncons = sb.ncons = p.ncons; sa.npref = sb.npref = p.npref;
  sb.y_from_lds = 1;
  if (j->f32) {
    sa.gs = sb.gs = 1.0f;  // fp32 operands: no scaling of the gradients
    launch_joint32_kernel(p.rows_per_wg, ta->kind.gl >= 0, dim3(2 * p.ncons), dim3(64 * kC32sWaves), st, (const ChainModel*)j->d_tab, sa, sb);
  } else {
    sb.blk0 = p.ncons;  // the emulator's row blocks follow the autoencoder's in the grid
    launch_joint_kernel(ta->prec, ta->kind.gl >= 0, dim3(2 * p.ncons + 8 * p.npref), dim3(64 * kChainWaves), st, (const ChainModel*)j->d_tab, sa, sb);
  }
  HIPCHK(hipGetLastError());
  return V21_OK;
}
// one epoch: the autoencoder trainer holds the signals (set_data(0, signals, NULL, w)), the emulator trainer the
// parameters of the SAME rows (set_data(0, params, any (n, latent) array, w_mse)); losses[0] = autoencoder,
// losses[1] = emulator (Keras epoch losses)
extern "C" int v21_joint_run_epoch(v21_joint* j, const int32_t* perm, int batch, double* losses) {
  if (!j || !losses) return fail(V21_ERR_ARG, "null argument");
  v21_trainer *ta = j->ae, *te = j->em;
  if (ta->n[0] < 1 || te->n[0] != ta->n[0]) return fail(V21_ERR_STATE, "both trainers need training sets of the same row count");
  if (!ta->y_is_x[0]) return fail(V21_ERR_STATE, "the autoencoder's targets must be its inputs (y == NULL)");
  CHK(use(ta->ctx));
  hipStream_t st = ta->ctx->stream;
  const long long n = ta->n[0];
  const int R = ta->ctx->nranks;
  if (batch < 1 || (batch + R - 1) / R > ta->max_batch) return fail(V21_ERR_ARG, "per-rank batch %d not in [1, max_batch %d]", (batch + R - 1) / R, ta->max_batch);
  const int* d_idx = nullptr;
  CHK(upload_rows(ta, perm, &d_idx));
  const long long steps = (n + batch - 1) / batch;
  for (v21_trainer* t : {ta, te}) CHK(ensure_steploss(t, steps));
  CHK(upload_if_changed(joint_table(j, 1), j->h_tab, j->d_tab.get(), st));
  if (R == 1 && !j->f32) CHK(refresh_dw_adam_table({ta, te}, j->d_dwadam, j->h_dwadam, st));
  const RouteEnv env = RouteEnv::read();
  bool group32 = decide_group32(j->f32, R, batch);  // (routes.h; then the tile check that needs the models)
  int max_blocks32 = 0;
  if (group32) {
    CHK(j->d_dw32.reserve(2));
    CHK(refresh_dw32_table({ta, te}, j->d_dw32, j->h_dw32, &max_blocks32, &group32, st));
  }
  CHK(chain_attr(ta->prec));
  const int dsig = ta->mlp->dims[0], dpar = te->mlp->dims[0], dlat = te->mlp->dims[te->mlp->L];
  for (long long s = 0; s < steps; ++s) {
    const EpochBatch b = epoch_batch(ta->ctx, n, batch, s);  // this rank's share of the global batch (data parallel: SURVEY 8e)
    const long long lo = b.lo, first = b.first;
    const int rows = b.rows, brows = b.brows;
    for (v21_trainer* t : {ta, te}) CHK(ensure_copies(t, false));
    if (rows > 0) {  // the reference's arithmetic: one joint chain launch (train_chain_joint_kernel / train_chain32s_joint_kernel)
      ChainStep sa = chain_step(ta->d_x[0], dsig, nullptr, dsig, ta->d_rw[0], d_idx, lo, rows, brows, dsig, nullptr, lo - first);
      ChainStep sb = chain_step(te->d_x[0], dpar, nullptr, dlat, te->d_rw[0], d_idx, lo, rows, brows, dlat, nullptr, lo - first);
      sa.step_off = (unsigned long long)s;  // the table holds the autoencoder's step counter as of the epoch's start (noise key)
      CHK(joint_launch(j, sa, sb, rows, 2, env));  // (both models' row blocks share the chip)
    }
    // then each model's gradients and Adam as after a chain step of its own: both models in one launch on a single rank
    if (group32) {
      CHK(launch_dw32_group({ta, te}, j->d_dw32, rows, s, max_blocks32, st));
      continue;
    }
    if (j->f32) {  // (chain32_update: one launch on a single rank, the exchange otherwise)
      for (v21_trainer* t : {ta, te}) CHK(chain32_update(t, rows, t->d_steploss + s));
      continue;
    }
    if (R == 1) {
      CHK(launch_dw_adam_group({ta, te}, j->d_dwadam, j->h_dwadam, rows, brows, s, st));
      continue;
    }
    // data parallel: each model's weight gradients (this rank's rows), summed over the ranks, then Adam -- the same
    // exchange as a plain step (reduce_and_update: all-reduce, or reduce-scatter + sharded Adam + all-gather)
    for (v21_trainer* t : {ta, te}) {
      if (rows > 0) {
        int nslice = 1;
        std::vector<Dw16Args> probs;
        dw16_problems(t, rows, brows, &nslice, probs);
        CHK(launch_dw16(t->prec, probs, st));
        if (nslice > 1) CHK(reduce_slabs(t, nslice));
      } else {
        CHK(zero_grad(t));
      }
      CHK(reduce_and_update(t, 1));
      CHK(step_tail(t, StepLoss{t->d_steploss + s, -1}));
    }
  }
  return epoch_losses({ta, te}, steps, n, losses);
}

// validation of both models in ONE launch: the autoencoder's loss on its validation signals, and the emulator's loss on
// the validation parameters against the latents the CURRENT encoder produces for the validation signals (what the
// reference gets from encoder.predict(signal_val), emulator.py:754) -- no host round trip for the latents
extern "C" int v21_joint_eval(v21_joint* j, double* losses) {
  if (!j || !losses) return fail(V21_ERR_ARG, "null argument");
  v21_trainer *ta = j->ae, *te = j->em;
  if (ta->n[1] < 1 || te->n[1] != ta->n[1]) return fail(V21_ERR_STATE, "both trainers need validation sets of the same row count");
  if (!ta->y_is_x[1]) return fail(V21_ERR_STATE, "the autoencoder's validation targets must be its inputs (y == NULL)");
  CHK(use(ta->ctx));
  hipStream_t st = ta->ctx->stream;
  const long long n = ta->n[1];
  if (n > (1ll << 30)) return fail(V21_ERR_ARG, "too many rows for one validation launch");
  for (v21_trainer* t : {ta, te}) CHK(ensure_copies(t, false));
  CHK(upload_if_changed(joint_table(j, 0), j->h_tab, j->d_tab.get(), st));  // (evaluation passes draw no noise)
  CHK(chain_attr(ta->prec));
  const int dsig = ta->mlp->dims[0], dpar = te->mlp->dims[0], dlat = te->mlp->dims[te->mlp->L];
  ChainStep sa = chain_step(ta->d_x[1], dsig, nullptr, dsig, ta->d_rw[1], nullptr, 0, (int)n, (int)n, dsig);
  ChainStep sb = chain_step(te->d_x[1], dpar, nullptr, dlat, te->d_rw[1], nullptr, 0, (int)n, (int)n, dlat);
  sa.fwd_only = sb.fwd_only = 1;
  // models = 1, not 2: the row blocks v21_trainer_eval's launch takes for n rows -- the same rows meet in the same partial
  // sums, and the autoencoder's validation loss is bit for bit the one it reports alone
  CHK(joint_launch(j, sa, sb, n, 1, RouteEnv::read()));
  return read_tickets({ta, te}, n, losses);
}
