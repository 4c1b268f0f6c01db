/* v21.h -- C ABI of libv21.so: the MI355X (gfx950) engine behind the 21cmVAE
 * predict()/train() hot path.
 *
 * The reference (christianhbye/21cmVAE) has no FFI of its own: its numeric engine is
 * TensorFlow/Keras, reached through eight call sites in
 * VeryAccurateEmulator/emulator.py (:369, :402, :739, :753-754, :756, :789, :790, :827).
 * Every entry point below names the reference call site it replaces.  The Python
 * shim (21cmvae_amd/engine.py) binds these with ctypes; INTEGRATION.md shows the
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C, opaque handles, no exceptions cross the boundary;
 *   - every function returns 0 on success or a negative V21_ERR_* code;
 *     v21_last_error() returns a thread-local human-readable message;
 *   - host buffers are caller-owned, C-contiguous, alive for the call only;
 *     device memory is owned by the library (or, for *_dev entry points, by the
 *     caller, who passes raw device pointers on the context's stream);
 *   - weights travel in Keras get_weights() order: W0 (in,out) row-major, b0, W1, ...
 *     (layout confirmed by the reference's shipped .h5 files);
 *   - one context per device; calls on one context must be serialised by the caller.
 */
#ifndef V21_H
#define V21_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct v21_ctx v21_ctx;
typedef struct v21_mlp v21_mlp;
typedef struct v21_trainer v21_trainer;

enum {
  V21_OK = 0,
  V21_ERR_ARG = -1,         /* bad argument (null, shape, range)              */
  V21_ERR_HIP = -2,         /* a HIP runtime call failed                      */
  V21_ERR_UNSUPPORTED = -3, /* valid request this build cannot serve          */
  V21_ERR_STATE = -4,       /* call order violated (e.g. no data set)         */
  V21_ERR_COMM = -5         /* RCCL failure                                   */
};

/* arithmetic of the dense contractions (accumulation is always fp32) */
enum { V21_PREC_F32 = 0, V21_PREC_F16 = 1, V21_PREC_BF16 = 2 };
/* V21_ACT_GAUSS: the variational latent layer (the KL/ELBO mode the
 * north star names; the reference snapshot has only its `z_mean` layer name,
 * models/autoencoder_based_emulator/encoder.h5).  A layer with this activation is
 * Dense(dims[l] -> 2*dims[l+1]) whose output is [z_mean | z_log_var]; what the next
 * layer sees is z = z_mean + exp(z_log_var / 2) * eps (dims[l+1] wide).  forward()
 * is deterministic (z = z_mean); the trainer samples eps and adds
 * kl_weight * KL(N(z_mean, exp z_log_var) || N(0, 1)) to every row's loss. */
enum { V21_ACT_LINEAR = 0, V21_ACT_RELU = 1, V21_ACT_GAUSS = 2,
       V21_ACT_TANH = 3, V21_ACT_SIGMOID = 4, V21_ACT_ELU = 5, V21_ACT_SOFTPLUS = 6 };
/* V21_ACT_TANH .. V21_ACT_SOFTPLUS: the smooth activations, Keras' definitions (the reference's `activation_func`:
 * "str or instance of tf.keras.activations"), evaluated in float32 whatever the precision of the contractions
 * (csrc/act.h: formulas that neither overflow nor give NaN for any finite z; expf / expm1f / log1pf at 1 ulp):
 *   code                  h = act(z)                  dh/dz, from the stored output h
 *   V21_ACT_TANH     = 3  tanh z                      1 - h^2
 *   V21_ACT_SIGMOID  = 4  1 / (1 + exp(-z))           h (1 - h)
 *   V21_ACT_ELU      = 5  z > 0 ? z : exp(z) - 1      h > 0 ? 1 : h + 1      (alpha = 1)
 *   V21_ACT_SOFTPLUS = 6  ln(1 + exp(z))              1 - exp(-h)
 * Who takes them:
 *   v21_mlp_create          on any layer (as it takes a ReLU output layer);
 *   v21_mlp_forward[_dev]   fused_fwd instantiated at run time once its code object is ready (hidden layers only; linear
 *                           output layer), before that and with V21_FWD_FORCE_GENERIC / V21_FWD_FORCE_CHAIN the generic
 *                           per-layer route, few rows the small route; never the table-driven chain kernels;
 *   v21_mlp_jacobian / _loglike / _fisher / _fit / _fit_map / the samplers: the generic Jacobian kernel and the two-launch
 *                           ln L (the fused Jacobian and the fused ln L variant exist for the stacks of csrc/archs.h only);
 *   v21_trainer_create      the per-layer route for every precision and batch; V21_ERR_UNSUPPORTED (the message names the
 *                           layer) when the LAST layer has one: the loss is taken on a linear output layer;
 *   v21_sweep_create        as for any per-layer trainer: works, every member equals its solo trainer;
 *   v21_joint_create        V21_ERR_UNSUPPORTED (the message names the activation): the joint step runs on the chain kernels;
 *   v21_mlp_jit             V21_ERR_UNSUPPORTED "no fused kernel for this stack" when the OUTPUT layer has one;
 *   v21_trainer_jit (fused training kernels): never eligible. */
enum { V21_DTYPE_F32 = 0, V21_DTYPE_F64 = 1 };

/* Fused prologue = preprocess.par_transform (preprocess.py:49-110) with the training-set statistics cached:
 *   t = x_j;  if (zero_floor_j > 0 && t == 0) t = zero_floor_j      (fx == 0 -> 1e-6, preprocess.py:76)
 *   if (log_mask_j) t = log10(t)                                     (preprocess.py:77-78)
 *   y_j = (t - lo_j) / span_j * 2 - 1,  span_j = hi_j - lo_j         (preprocess.py:105-108, float64)
 * and the float32 cast Keras applies to the float64 result [K].  lo / hi are the column minima / maxima of the
 * log-transformed TRAINING parameters (float64, computed by the host as the reference computes them, :89-101).
 * The reference floors and takes log10 IN THE DTYPE OF THE ARRAY IT IS HANDED (:74-78) and does the affine map in
 * float64 (:81-85, :105-108); the library keeps both branches:
 *   float64 rows (v21_mlp_forward with V21_DTYPE_F64): floor, log10 and map in float64 on the device;
 *   float32 rows (V21_DTYPE_F32, and every device-resident input): floor = (float)zero_floor_j, log10 rounded to
 *     float32 (the correctly rounded log10f), then the float64 map -- numpy's float32 branch up to log10f's last bit.
 * n <= 8. */
#include "v21_types.h" /* v21_affine_in */

/* Fused epilogue = preprocess.unpreproc (preprocess.py:27-46): y*std + mean_j. */
typedef struct {
  float std;
  const float* mean; /* host pointer, out_dim floats */
  int32_t n;
} v21_affine_out;

const char* v21_last_error(void);
int v21_version(void);
int v21_device_count(int* n);

/* ---- context: one per device; owns a HIP stream ------------------------------ */
int v21_ctx_create(int device, v21_ctx** out);
int v21_ctx_destroy(v21_ctx* ctx);
int v21_ctx_sync(v21_ctx* ctx);
/* adopt an external hipStream_t (e.g. torch's current stream); NULL restores own */
int v21_ctx_set_stream(v21_ctx* ctx, void* hip_stream);
int v21_ctx_get_stream(v21_ctx* ctx, void** hip_stream);

/* device memory + copies + event timing, so a host program needs nothing else */
int v21_malloc(v21_ctx* ctx, size_t bytes, void** dptr);
int v21_free(v21_ctx* ctx, void* dptr);
/* page-locked host memory: a result buffer of this kind is filled by the device over PCIe
 * directly (no staging copy) -- the Python shim hands out numpy arrays backed by a pool of
 * them for large predict() results */
int v21_host_alloc(v21_ctx* ctx, size_t bytes, void** hptr);
int v21_host_free(v21_ctx* ctx, void* hptr);
int v21_memcpy_h2d(v21_ctx* ctx, void* dst, const void* src, size_t bytes);
int v21_memcpy_d2h(v21_ctx* ctx, void* dst, const void* src, size_t bytes);
int v21_memset(v21_ctx* ctx, void* dst, int value, size_t bytes);
int v21_event_create(v21_ctx* ctx, void** ev);
int v21_event_destroy(v21_ctx* ctx, void* ev);
int v21_event_record(v21_ctx* ctx, void* ev);               /* on the ctx stream */
int v21_event_elapsed_ms(v21_ctx* ctx, void* start, void* stop, float* ms); /* syncs stop */

/* ---- dense stack: replaces emulator._gen_model (emulator.py:12-48) + the Keras
 * Model object it returns.  A chain of models (emulator -> decoder,
 * emulator.py:789-790; encoder -> decoder, emulator.py:517) is ONE stack whose
 * `act` array has a linear layer in the middle. ----------------------------------- */
int v21_mlp_create(v21_ctx* ctx, int n_layers, const int* dims /* n_layers+1 */,
                   const int* act /* n_layers */, v21_mlp** out);
int v21_mlp_destroy(v21_mlp* mlp);
int v21_mlp_num_params(const v21_mlp* mlp, size_t* n);
/* Keras Model.set_weights / get_weights (flat fp32 arena, Keras order) */
int v21_mlp_set_weights(v21_mlp* mlp, const float* flat, size_t n);
int v21_mlp_get_weights(v21_mlp* mlp, float* flat, size_t n);
/* NULL clears the transform.  Both are copied. */
int v21_mlp_set_input_transform(v21_mlp* mlp, const v21_affine_in* t);
int v21_mlp_set_output_transform(v21_mlp* mlp, const v21_affine_out* t);
/* 1 if (dims, act) has a fully fused register-resident kernel, else 0 */
int v21_mlp_has_fused(const v21_mlp* mlp, int precision, int* yes);

/* Model.predict (emulator.py:402, :753-754, :789-790) and Model.__call__ (:517, :827):
 * host (n, in_dim) f32/f64 -> host (n, out_dim) f32.  flags: bit0 = apply input
 * transform, bit1 = apply output transform, bit2 = force the generic per-layer path,
 * bit3 = never take the small-batch latency path.
 * Path selection (results agree within fp32 rounding of the summation order): the fused
 * one-launch kernel for the shipped stack shapes; for up to V21_SMALL_BATCH_ROWS rows in
 * f32 (and for any stack without a fused kernel) one latency-oriented launch per layer
 * that spreads a layer's output tiles over the chip -- a sampler that calls
 * predict() row by row (the reference's use case: README "40 ms" per call) waits for one
 * memory round trip per layer instead of for one wave walking the whole stack. */
int v21_mlp_forward(v21_mlp* mlp, const void* x, int x_dtype, int64_t n, float* y,
                    int precision, int flags);
/* Same, device-resident, asynchronous on the context stream.  ldx/ldy = row pitch
 * in floats (>= in_dim / out_dim). */
int v21_mlp_forward_dev(v21_mlp* mlp, const float* d_x, int64_t ldx, int64_t n,
                        float* d_y, int64_t ldy, int precision, int flags);
/* The fully fused register-resident kernel (csrc/fused_fwd.h) is straight-line code per (stack, precision): the stacks of
 * csrc/archs.h are compiled into the library, every other `_gen_model` output (emulator.py:12-48: any `hidden_dims`)
 * gets it instantiated AT RUN TIME by hiprtc (csrc/jit.h), in a background thread started by the first
 * v21_mlp_forward[_dev] call above V21_SMALL_BATCH_ROWS rows; calls that arrive earlier take the table-driven one-launch
 * kernel (same results to operand rounding).  Code objects are cached under $V21_KERNEL_CACHE (default
 * ~/.cache/21cmvae_amd/kernels) and looked up in `kernel_cache/` next to libv21.so first; V21_JIT=0 switches the
 * compilation off (cached kernels are still used).
 * v21_mlp_jit: ask for the kernel now and wait up to wait_ms milliseconds (< 0: until the compilation has ended, 0: do
 *   not wait); *status = 1 ready (also for the compiled-in stacks), 0 compiling; V21_ERR_UNSUPPORTED (status -1) when
 *   the stack cannot have one (non-linear output layer, variational head, too wide for the register budget, no
 *   libhiprtc) -- v21_last_error says which.
 * v21_jit_prebuild: compile (stack, precision) into `dir` (NULL: kernel_cache/ next to the library) without touching a
 *   GPU -- a build step for deployments that know their stacks. */
int v21_mlp_jit(v21_mlp* mlp, int precision, int wait_ms, int* status);
/* r5: the same for the fused TRAINING kernel (csrc/fused_train16.h: forward + loss + activation gradients of steps of
 * >= 8,193 rows in one launch, 64-row workgroups).  `_gen_model` takes any hidden_dims (emulator.py:12-48); four stacks
 * have the kernel compiled in (archs.h T1-T4), every other f16 / bf16 trainer of >= 8,193 rows per step whose stack the
 * template can express (linear output, no variational head, 2-8 layers up to 512 wide) has it instantiated at run time:
 * asked for when the trainer is created, taken once the code object is there (until then, and if it never comes, the
 * chain kernel serves).  v21_trainer_jit waits up to wait_ms (< 0: until compiled): *status 1 ready, 0 compiling;
 * V21_ERR_UNSUPPORTED (status -1) when this trainer cannot have one.  v21_jit_prebuild(..., precision | 16, dir) compiles
 * it ahead of time. */
int v21_trainer_jit(v21_trainer* tr, int wait_ms, int* status);
int v21_jit_prebuild(int n_layers, const int* dims, const int* act, int precision, const char* dir);
#define V21_FWD_IN_TRANSFORM 1
#define V21_FWD_OUT_TRANSFORM 2
#define V21_FWD_FORCE_GENERIC 4
#define V21_FWD_NO_SMALL 8
/* diagnostics / benchmarks: the table-driven one-launch forward (csrc/train_chain.h, FORWARD mode: any stack up to 512
 * wide, f16 / bf16) even where a compiled fused kernel exists -- what every other stack gets by default */
#define V21_FWD_FORCE_CHAIN 16
/* diagnostics / benchmarks: the run-time-instantiated fused kernel (v21_mlp_jit) even for a stack that has a
 * compiled-in one; waits for the compilation, V21_ERR_UNSUPPORTED if the stack cannot have one */
#define V21_FWD_FORCE_JIT 32
#define V21_SMALL_BATCH_ROWS 4096

/* ---- parameter Jacobian and Gaussian log-likelihood (forward mode: the primal and its in_dim tangents pushed through
 * the stack in one launch; the reference differentiates its Keras model with tf.GradientTape).
 *   v21_mlp_jacobian[_dev]  y[n, :] = the forward's output (nullable) and jac[n, j, :] = d y[n, :] / d x[n, j], layout
 *     (n, in_dim, out_dim), float32.  flags: V21_FWD_IN_TRANSFORM / V21_FWD_OUT_TRANSFORM as for the forward; with the
 *     input transform the derivative is with respect to the RAW parameter, taken at the value after the zero floor
 *     (the two input branches of v21_affine_in: float32 and float64 rows); the output transform contributes std.
 *   v21_mlp_set_likelihood  the data vector d and the inverse variances w = 1 / sigma^2 (out_dim floats each, copied;
 *     NULL clears).  Bins with w == 0 do not influence any result.
 *   v21_mlp_loglike[_dev]   lnl[n] = -1/2 sum_k w_k (d_k - y_k)^2 and grad[n, j] = d lnl / d x[n, j] (nullable), reduced
 *     on the device (4 (1 + in_dim) bytes per row leave it instead of the whole Jacobian).
 * Routes (v21_route_jacobian; csrc/routes.h: 1 = fused, 2 = generic, 3 = fused_rt): the stacks of archs.h (S1-S4, up to
 * 15 inputs) take fused_jac<Arch, Prec>, whose primal is bit-identical to the forward's fused route in the same
 * precision; every other stack (any hidden_dims, any in_dim, wider than 512, V21_ACT_GAUSS evaluated as z = z_mean)
 * takes a generic kernel in f32 arithmetic whatever the precision -- unless the handle ASKED for route 3:
 *   v21_mlp_jit_jacobian  fused_jac instantiated for THIS stack at run time (csrc/jit.h; ReLU, linear and the smooth
 *     activations 3 .. 6 on hidden layers; 1 .. 15 inputs, a linear output layer, widths up to 1,024 where the registers
 *     hold them), semantics as v21_mlp_jit: *status 1 ready (also for a compiled-in stack), 0 compiling,
 *     V21_ERR_UNSUPPORTED (status -1) with the reason in v21_last_error.  It marks the handle as asked for that
 *     precision: from the first call that starts with the code object in place, every Jacobian-side call of the handle
 *     (Jacobian, ln L + gradient, Fisher, fits, MAP, both samplers) takes route 3.  A call decides its route once, for all
 *     its slices, chunks and iterations; a kernel that arrives mid-call serves the next call; one that cannot be loaded
 *     or needs scratch memory (found when the first call after its arrival decides its route) leaves the handle on
 *     route 2, without an error.  Its primal is bit-identical to the
 *     forward's run-time route (v21_mlp_jit) in the same precision.  Without the call nothing changes.
 *   v21_route_jacobian_rt  the route of a handle that asked and has its kernel: 3 where the stack can have one and the
 *     flags allow it, else v21_route_jacobian's answer (which never says 3: it knows no handle).  Pure host logic.
 *   V21_FWD_FORCE_JIT on any Jacobian-side call (diagnostics): route 3 or V21_ERR_UNSUPPORTED (an ineligible stack, a
 *     kernel that needs scratch memory, a y pitch of 2^21 floats or more) -- asks, waits for the compilation, and works
 *     on S1-S4 too.  A forced call ASKS: it opts the handle in for that precision like v21_mlp_jit_jacobian, for good.  v21_jit_prebuild(..., precision | 32, dir) compiles the kernel ahead of time.
 * n = 0 is a no-op.  The _dev forms are asynchronous on the
 * context's stream; the host forms return when the results are in place.  v21_mlp_last_jac_route: the route of the
 * last call and the calls per route (counts[4], indexed by route). */
int v21_mlp_jacobian(v21_mlp* mlp, const void* x, int x_dtype, int64_t n, float* y, float* jac, int precision, int flags);
int v21_mlp_jacobian_dev(v21_mlp* mlp, const float* d_x, int64_t ldx, int64_t n, float* d_y, int64_t ldy, float* d_jac,
                         int precision, int flags);
int v21_mlp_set_likelihood(v21_mlp* mlp, const float* data, const float* inv_var, int32_t n);
int v21_mlp_loglike(v21_mlp* mlp, const void* x, int x_dtype, int64_t n, float* lnl, float* grad, int precision, int flags);
int v21_mlp_loglike_dev(v21_mlp* mlp, const float* d_x, int64_t ldx, int64_t n, float* d_lnl, float* d_grad, int precision,
                        int flags);
int v21_route_jacobian(int n_layers, const int* dims, const int* act, int precision, int64_t n, int flags, int* route);
int v21_route_jacobian_rt(int n_layers, const int* dims, const int* act, int precision, int flags, int* route);
int v21_mlp_jit_jacobian(v21_mlp* mlp, int precision, int wait_ms, int* status);
int v21_mlp_last_jac_route(v21_mlp* mlp, int* route, long long counts[4]);

/* ---- forward-only log-likelihood: lnl[n] = -1/2 sum_k w_k (d_k - y_k)^2 WITHOUT its gradient -- the call nested
 * samplers, ensemble samplers and importance sampling make.  No Jacobian is formed.
 *   data == NULL: every row is scored against the likelihood record (v21_mlp_set_likelihood, required either way: the
 *     inverse variances are always the record's).  Otherwise data is (n_data, out_dim) float32 with n % n_data == 0
 *     and row n is scored against data row n / (n / n_data), as in v21_mlp_fit (V21_ERR_ARG otherwise).  Bins with
 *     w == 0 do not influence the result whatever d holds there (inf and NaN included), and with a nuisance record
 *     (v21_mlp_set_nuisance) the result is lnL_m = -1/2 (r^T W r - |b|^2), as v21_mlp_loglike's.
 *   flags: V21_FWD_IN_TRANSFORM / V21_FWD_OUT_TRANSFORM and the forward's route flags, as for v21_mlp_forward_dev.
 * Routes (v21_route_loglike_fwd; csrc/routes.h: 1 = fused, 2 = two-launch).  Fused: the ln L variant of
 *   fused_fwd<Arch, Prec> for the stacks of archs.h -- y is computed with the forward's fused-route arithmetic bit for
 *   bit (for any n: there is no few-row route here) and reduced in the output layer's epilogue, 4 bytes per row leave
 *   the kernel.  It takes a call whose data are uniform per 128-row workgroup: the record, or n / n_data a multiple of
 *   128; no nuisance record, no forward route flag.  Two-launch: everything else -- stacks outside archs.h, stacks
 *   ending in a ReLU, V21_ACT_GAUSS, nuisance records, other data layouts: the forward on the route its own decision
 *   gives for these rows and flags (counted by v21_mlp_last_route; a call of more than V21_SMALL_BATCH_ROWS rows keeps
 *   all its slices off the few-row route) into the likelihood workspace in slices of 16,384 rows, y only, then one
 *   row reduction.  n = 0 is a no-op.  The _dev form never synchronises; the host form works in chunks of 8,192 rows,
 *   rounded down to whole spectra when data is given, and returns when the results are in place.
 *   v21_route_loglike_fwd: the route of a call of n rows against n_data data rows (0: the record) for a handle with
 *   n_modes nuisance modes -- pure host logic.  v21_mlp_last_lnl_route: the route of the last of these calls and the
 *   calls per route (counts[4], indexed by route); v21_mlp_last_jac_route is not touched by them.
 * Route 3 = fused_rt (K19), for a handle that ASKED:
 *   v21_mlp_jit_loglike  the fused route's kernel instantiated for THIS stack at run time (csrc/jit.h: kJitLnl; ReLU,
 *     linear and the smooth activations 3 .. 6 on hidden layers, a linear output layer, widths up to 1,024 where the
 *     registers hold them), semantics as v21_mlp_jit_jacobian: *status 1 ready (also for a compiled-in stack, which
 *     keeps route 1), 0 compiling, V21_ERR_UNSUPPORTED (status -1) with the reason in v21_last_error -- a stack the
 *     kernel cannot express, V21_JIT=0 with nothing cached, a compiler failure.  Requested at most once per (handle,
 *     precision).  It marks the handle as asked for that precision: from the first call that starts with the code
 *     object in place, every call of v21_mlp_loglike_fwd[_dev], v21_mlp_sample_ensemble[_dev] and
 *     v21_mlp_sample_nested[_dev] of the handle that would take route 1 on a stack of archs.h -- the same conditions:
 *     uniform data, no nuisance record, no forward route flag, in_dim <= 8 with the input transform -- takes route 3.  A
 *     call decides its route once, for all its slices, chunks and evaluations; a kernel that arrives mid-call serves the
 *     next call; one that cannot be loaded or needs scratch memory (found when the first call after its arrival
 *     decides its route) leaves the handle on route 2, without an error.  y is the forward's run-time route's
 *     (v21_mlp_jit) bit for bit.  Without the call nothing changes; V21_FWD_FORCE_JIT here still means route 2 with the
 *     run-time forward inside.  v21_jit_prebuild(..., precision | 64, dir) compiles the kernel ahead of time.
 *   v21_route_loglike_fwd_rt / v21_route_ensemble_rt (the nested sampler's: n_live in the place of n_walkers)  the route
 *     of a handle that asked and has its kernel: 3 where v21_route_loglike_fwd / v21_route_ensemble would say 1 for a
 *     compiled stack and this stack can have the kernel, else their answer (which never is 3: they know no handle). */
int v21_mlp_jit_loglike(v21_mlp* mlp, int precision, int wait_ms, int* status);
int v21_route_loglike_fwd_rt(int n_layers, const int* dims, const int* act, int precision, int64_t n, int64_t n_data, int n_modes,
                             int flags, int* route);
int v21_route_ensemble_rt(int n_layers, const int* dims, const int* act, int precision, int64_t n, int64_t n_data, int n_walkers,
                          int n_modes, int flags, int host_form, int* route, int64_t* chunk_rows);
int v21_mlp_loglike_fwd(v21_mlp* mlp, const void* x, int x_dtype, int64_t n, const float* data, int64_t n_data, float* lnl,
                        int precision, int flags);
int v21_mlp_loglike_fwd_dev(v21_mlp* mlp, const float* d_x, int64_t ldx, int64_t n, const float* d_data, int64_t n_data,
                            float* d_lnl, int precision, int flags);
int v21_route_loglike_fwd(int n_layers, const int* dims, const int* act, int precision, int64_t n, int64_t n_data, int n_modes,
                          int flags, int* route);
int v21_mlp_last_lnl_route(v21_mlp* mlp, int* route, long long counts[4]);

/* ---- Fisher matrices and batched maximum-likelihood fits, on the Jacobian of the block above.
 *   v21_mlp_fisher[_dev]  fisher[n, i, j] = sum_k w_k jac[n, i, k] jac[n, j, k], (n, in_dim, in_dim) float32, exactly
 *     symmetric, with w the inverse variances of the likelihood record (v21_mlp_set_likelihood, required) and jac as
 *     v21_mlp_jacobian computes it for the same flags (raw units with V21_FWD_IN_TRANSFORM); lnl / grad (nullable) as
 *     v21_mlp_loglike -- the record's data is read only for them.  in_dim <= 15 (V21_ERR_UNSUPPORTED otherwise).
 *   v21_mlp_fit[_dev]     per row, a projected Levenberg-Marquardt maximisation of ln L in the transformed coordinates
 *     u = par_transform(x) in [-1, 1]^in_dim, the training box of the input transform (required: V21_ERR_STATE
 *     without it; in_dim <= 8).  x0: start rows in raw units, clamped into the box.  Iteration: evaluate ln L, its
 *     gradient g and Fisher matrix F at the proposal; accept it if ln L rose (the start always), lambda /= 10 (>= 1e-12),
 *     else lambda *= 10; solve (F + lambda diag(max(F_ii, tiny))) delta = g (float64 Cholesky); proposal =
 *     clamp(u + delta, -1, 1).  status[n]: 1 the projected step is <= xtol, 2 lambda > 1e12 (no improving step),
 *     3 no information (every F_ii == 0: the start is kept), 0 max_iter proposals evaluated.  lnl: ln L at x_hat, never
 *     below lnl_start (ln L at the clamped start).  x_hat: the accepted point, mapped back in float64
 *     (lo + (u + 1) span / 2, then 10^ for a log column: a log column's lower bound comes back as 10^lo, e.g. the fx
 *     zero floor, not 0), in x0's dtype (_dev: float32, pitch in_dim).  fisher (nullable): v21_mlp_fisher at x_hat in raw
 *     units.  data: NULL = the record's data for every row, else (n_data, out_dim) float32 with n % n_data == 0, row n
 *     fitting data row n / (n / n_data); the record's inverse variances weigh every row.  opts: v21_types.h.
 *     (data non-NULL with n_data < 1, or n % n_data != 0: V21_ERR_ARG.)  lnl_start, fisher and status are nullable.
 *     The evaluations take the Jacobian's route for the flags given (V21_FWD_IN_TRANSFORM is implied); rows are
 *     independent of each other and of how a call is chunked.  v21_mlp_last_jac_route counts each call of these entries
 *     once per Fisher evaluation it asks for: a fisher call once, a fit once for its iterations and once more for the
 *     Fisher matrix at x_hat when that is asked for (never per iteration or per chunk).
 * The host forms work in chunks of 8,192 rows and return when the results are in place; the _dev forms are
 * asynchronous on the context's stream except that a fit reads its running-row count every check_every iterations. */
int v21_mlp_fisher(v21_mlp* mlp, const void* x, int x_dtype, int64_t n, float* fisher, float* lnl, float* grad, int precision, int flags);
int v21_mlp_fisher_dev(v21_mlp* mlp, const float* d_x, int64_t ldx, int64_t n, float* d_fisher, float* d_lnl, float* d_grad,
                       int precision, int flags);
int v21_mlp_fit(v21_mlp* mlp, const void* x0, int x_dtype, int64_t n, const float* data, int64_t n_data, const v21_fit_opts* opts,
                void* x_hat, float* lnl, float* lnl_start, float* fisher, int32_t* status, int precision, int flags);
int v21_mlp_fit_dev(v21_mlp* mlp, const float* d_x0, int64_t ldx, int64_t n, const float* d_data, int64_t n_data,
                    const v21_fit_opts* opts, float* d_x_hat, float* d_lnl, float* d_lnl_start, float* d_fisher, int32_t* d_status,
                    int precision, int flags);

/* ---- MAP fits with held parameters, and the Laplace approximation of the evidence.  v21_mlp_fit_map[_dev] is
 * v21_mlp_fit[_dev] -- arguments, iteration, constants, statuses, chunks -- with two changes, both in float64 in u:
 *   Objective.  ln L(u) + ln p(u), ln p = -1/2 sum_i ((u_i - mu_i) / sd_i)^2 over the normal columns of the handle's prior
 *     record (v21_mlp_set_prior) that are NOT held, when mopts->use_prior is 1 (without a record: the uniform prior); a
 *     proposal is accepted when this sum rose.  The solve becomes (A + lambda diag(max(A_ii, tiny))) delta = g + grad ln p
 *     with A = F + diag(1 / sd^2) on those columns.
 *   Held columns.  mopts->hold[i] = 1: column i is no parameter.  It keeps the float32 u of its clamped start (its x_hat
 *     entry is what max_iter = 0 returns for that start), its prior is never read, and in the system g_i = 0,
 *     A_ij = A_ji = 0 (j != i), A_ii = 1, so that its delta is exactly 0.
 *   status 3 (no information) is decided on the diagonal of A over the free columns: a flat likelihood under a normal
 *     column moves to the prior's mode, clamped into the box; with every column held the clamped start comes back with
 *     status 1 after 0 iterations.
 *   lnl and lnl_start stay ln L alone; fisher stays v21_mlp_fisher at x_hat (likelihood only, raw units).
 * Results beside the fit's (v21_map_out, each nullable), at the accepted point u_hat with lambda = 0:
 *   lnp      ln p(u_hat), unnormalised, over the free normal columns;
 *   laplace  ln L + ln p + d_free / 2 ln(2 pi) - 1/2 ln det A_free, d_free the free columns, the determinant from the
 *            diagonal of A's Cholesky factor; NaN when a free pivot is not positive and finite.  Subtract ln of the
 *            integral of exp(ln p) over the free columns (d_free ln 2 for uniform ones) for the evidence with respect to
 *            the normalised prior, as the samplers define it.  It assumes an interior mode and a smooth ln L: at a mode
 *            on a face of the box it is no evidence;
 *   prec_u   A (n, in_dim, in_dim) float32, exactly symmetric, the held rows and columns those of the identity.
 * With mopts NULL (or use_prior 0 and nothing held) every result of v21_mlp_fit[_dev] comes back bit for bit.
 * V21_ERR_ARG, before any device work and with the handle left usable: use_prior or a hold entry outside {0, 1}. */
int v21_mlp_fit_map(v21_mlp* mlp, const void* x0, int x_dtype, int64_t n, const float* data, int64_t n_data, const v21_fit_opts* opts,
                    const v21_map_opts* mopts, void* x_hat, float* lnl, float* lnl_start, float* fisher, int32_t* status,
                    const v21_map_out* mout, int precision, int flags);
int v21_mlp_fit_map_dev(v21_mlp* mlp, const float* d_x0, int64_t ldx, int64_t n, const float* d_data, int64_t n_data,
                        const v21_fit_opts* opts, const v21_map_opts* mopts, float* d_x_hat, float* d_lnl, float* d_lnl_start,
                        float* d_fisher, int32_t* d_status, const v21_map_out* mout, int precision, int flags);

/* ---- posterior sampling: n independent Markov chains on the device, each a Metropolis-adjusted Langevin sampler whose
 * metric is the Fisher matrix at the current point ("simplified manifold MALA"), of the posterior of v21_mlp_loglike's
 * ln L under a UNIFORM PRIOR ON THE TRAINING BOX in the fit's coordinates u = par_transform(x) in [-1, 1]^in_dim -- that
 * is, log-uniform in the raw value of a log10 column.  Needs the input transform and a likelihood record; in_dim <= 8.
 *   One transition, with G(u) = F(u) + ridge I = L L^T (float64 Cholesky), d = in_dim, step size e:
 *     mu(u) = u + e^2 / 2 G(u)^-1 g(u);   proposal u' = mu(u) + e L(u)^-T xi, xi ~ N(0, I_d), rounded to float32
 *     log q(b | a) = -|L(a)^T (b - mu(a))|^2 / (2 e^2) + sum_i log L_ii(a) - d / 2 log(2 pi e^2)
 *     log alpha = lnL(u') - lnL(u) + log q(u | u') - log q(u' | u);   accepted iff log(uniform) < log alpha.
 *   ln L, g and F at a proposal come from one Fisher evaluation on u, as a fit's do.  The derivative of the metric that
 *   full manifold MALA carries in its drift is left out; the acceptance uses the q above, so the chain is exact.  A
 *   proposal with a coordinate outside [-1, 1] is rejected (never clamped or reflected; its evaluation is not read), and
 *   so is one whose G has no finite Cholesky factor.  With all-zero weights G = ridge I: a random walk on the box.
 *   A call runs n_warmup + n_steps transitions.  In transition t = 1 .. n_warmup of the call a chain adapts its own step
 *   size, log e += t^-0.6 (min(1, alpha) - target_accept); afterwards e is frozen.  Only the n_steps transitions after
 *   the warm-up enter samples (every thin-th of them, n_steps / thin rounded down per chain; transitions beyond the last
 *   whole multiple of thin still enter the moments), mean_u / cov_u and accept_rate.
 *   Random numbers: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85), key =
 *   (seed & 0xffffffff, seed >> 32), counter = (c & 0xffffffff, c >> 32, s, block) with c = chain0 + the chain's row in
 *   the call and s = step0 + the transition's index in the call (warm-up included): a draw depends on nothing else, so
 *   chains do not depend on how a run is split over calls, chunks or GPUs.  A word w gives the uniform (w + 0.5) 2^-32.
 *   Blocks 0 and 1 give xi: block b's words (w0, w1, w2, w3) give xi[4b] = r cos(t), xi[4b + 1] = r sin(t) with
 *   r = sqrt(-2 ln U(w0)), t = 2 pi U(w1), and xi[4b + 2], xi[4b + 3] likewise from (w2, w3) (Box-Muller, float64;
 *   components >= in_dim are not used).  Word 0 of block 2 gives the uniform of the acceptance test.
 *   x0: start rows in raw units (clamped into the box; accepted whatever their ln L).  data / n_data: as for a fit (chain
 *   n samples data row n / (n / n_data)).  eps_start (nullable, n float64): per-chain step sizes instead of eps0 --
 *   with x_last, eps_last, n_warmup = 0 and step0 advanced by the transitions done, a call continues an earlier one
 *   (exactly, when x_last is float64: the state is the float32 u).  opts and results: v21_types.h.  The route is the
 *   Jacobian's; v21_mlp_last_jac_route counts a sample call once, whatever its transitions and chunks.
 * The host form works in chunks of 8,192 chains and returns when the results are in place; the _dev form never
 * synchronises. */
int v21_mlp_sample(v21_mlp* mlp, const void* x0, int x_dtype, int64_t n, const float* data, int64_t n_data, const v21_sample_opts* opts,
                   const double* eps_start, const v21_sample_out* out, int precision, int flags);
int v21_mlp_sample_dev(v21_mlp* mlp, const float* d_x0, int64_t ldx, int64_t n, const float* d_data, int64_t n_data,
                       const v21_sample_opts* opts, const double* d_eps_start, const v21_sample_out* out, int precision, int flags);

/* ---- parallel tempering (replica exchange) of the sampler above: the modes a single chain cannot leave, and the evidence.
 *   Rows and rungs.  A call has n rows; T = n_temps consecutive rows form one ladder (n % T == 0).  Row r is rung
 *   k = r % T of ladder r / T and has beta = betas[k], inside [0, 1] and strictly decreasing in k.  The temperature belongs
 *   to the row; states move between rows.  Step size, moments, counters and stored samples stay with the row, that is,
 *   with the rung: rows with k = 0 and betas[0] = 1 are posterior chains, a row at beta = 0 samples the prior (the box).
 *   Tempered transition.  That of v21_mlp_sample with ln L, g and F replaced by beta ln L, beta g and beta F wherever
 *   they enter the drift, the metric and log alpha: G = beta F + ridge I and
 *     log alpha = beta (lnL' - lnL) + log q(u | u') - log q(u' | u).
 *   At beta = 0 the three products are exactly 0 whatever the evaluation holds, non-finite values included.  The state
 *   keeps the un-tempered float32 ln L, g and F; samples_lnl and lnl_last are un-tempered, last_log_alpha is tempered.
 *   Swap events.  Let S = step0 + (index of the transition in the call), the Philox step word.  With swap_every > 0 a
 *   swap event follows the decision of transition S whenever (S + 1) % swap_every == 0 (warm-up transitions included);
 *   its number is e = (S + 1) / swap_every - 1.  It proposes the pairs (k, k + 1) with k % 2 == e % 2 in every ladder.
 *   Pair (k, k + 1) swaps iff log U < (beta_k - beta_k+1) (lnL_k+1 - lnL_k), formed in float64 from the stored float32
 *   ln L, with U from word 0 of Philox block 3 of the lower row's chain at step S (blocks 0 .. 2 are the transition's); a
 *   NaN right-hand side refuses.  On a swap the two rows exchange their point with its evaluation (u, ln L, g, F) and
 *   nothing else: nothing is re-evaluated.
 *   Order inside one transition: (1) the pending proposal is decided, (2) the step size adapted in warm-up, (3) the swap
 *   event run, if any, (4) moments accumulated and the thinned sample stored -- both see the state after the swap --
 *   (5) the next proposal drawn from that state.
 *   Per row, beside the results of v21_sample_out, in float64 over the kept transitions (v21_temper_out): the mean and
 *   the variance (divided by n_steps, as cov_u) of the un-tempered ln L after the swap event, and swap_accept = swaps
 *   accepted / proposed with this row as the lower one of the pair (0 where none was proposed).  Averaged over ladders,
 *   mean_lnl of rung k estimates E_beta_k[ln L], whose integral over beta from 0 to 1 is ln Z with Z = the integral of L
 *   over the box divided by its volume 2^in_dim.
 *   Invariance.  A draw depends only on (seed, chain, step, block) and a swap event only on S: results do not depend on
 *   how a run is split over calls, host chunks or devices, provided no ladder is split.
 *   temper: NULL = one rung at beta = 1 without swaps.  V21_ERR_ARG, the handle left usable: n_temps outside 1 .. 32, a
 *   beta outside [0, 1] or not below its predecessor, swap_every < 0, n % n_temps != 0, or data given and
 *   (n / n_data) % n_temps != 0 (a ladder would straddle two spectra).  Everything else -- in_dim <= 8, the input
 *   transform and a likelihood record required, nuisance records, eps_start, continuation, the route counted once per
 *   call -- as v21_mlp_sample; with n_temps = 1 every result of v21_sample_out equals that call's bit for bit.
 * The host form works in chunks of the largest multiple of n_temps that is not above 8,192 rows. */
int v21_mlp_sample_tempered(v21_mlp* mlp, const void* x0, int x_dtype, int64_t n, const float* data, int64_t n_data,
                            const v21_sample_opts* opts, const v21_temper_opts* temper, const double* eps_start,
                            const v21_sample_out* out, const v21_temper_out* tout, int precision, int flags);
int v21_mlp_sample_tempered_dev(v21_mlp* mlp, const float* d_x0, int64_t ldx, int64_t n, const float* d_data, int64_t n_data,
                                const v21_sample_opts* opts, const v21_temper_opts* temper, const double* d_eps_start,
                                const v21_sample_out* out, const v21_temper_out* tout, int precision, int flags);

/* ---- the affine-invariant ensemble sampler (Goodman & Weare 2010, the stretch move) on forward-only ln L: no gradient
 * and no Fisher matrix, so it also serves targets whose Fisher metric is singular or misleading.
 *   Target.  That of v21_mlp_sample: ln L is v21_mlp_loglike_fwd's (nuisance records and the w == 0 rule included) under
 *   the uniform prior on the training box in u = par_transform(x) in [-1, 1]^d.  Needs the input transform and a
 *   likelihood record; d = in_dim <= 8.
 *   Rows, ensembles, sets.  A call has n rows; W = n_walkers consecutive rows form one ensemble: W even,
 *   2 (d + 1) <= W <= 512, n % W == 0 and, with a data matrix, (n / n_data) % W == 0.  H = W / 2; walker i = r % W of row r
 *   belongs to set h = i / H and has index j = i % H in it.
 *   One sweep.  Sweep S = step0 + its index in the call (warm-up included) is two half-moves, h = 0 then h = 1; half-move
 *   h updates every walker of set h from the CURRENT positions of set 1 - h of the same ensemble.  For walker i at x_i:
 *     random words (w0, w1, w2) of Philox block 0 of (seed, c = chain0 + row, S) -- function, key and counter mapping as
 *     documented for v21_mlp_sample, a word w giving the uniform U(w) = (w + 0.5) 2^-32;
 *     stretch factor z = ((a - 1) U(w0) + 1)^2 / a, so that g(z) is proportional to 1 / sqrt(z) on [1 / a, a];
 *     partner k = floor(H w1 / 2^32) (the high word of H x w1) within set 1 - h, at x_k;
 *     proposal y = float32(x_k + z (x_i - x_k)), formed in float64 and rounded once;
 *     log alpha = (d - 1) ln z + lnL(y) - lnL(x_i), in float64 from the stored float32 ln L;
 *     accepted iff ln U(w2) < log alpha.
 *   A y with a coordinate outside [-1, 1] is rejected and its evaluation is not read: log alpha is reported as -inf; y is
 *   never clamped or reflected.  A NaN log alpha rejects (and is reported as -inf).
 *   Stretch scale and warm-up.  a is not adapted; the n_warmup sweeps are burn-in and are only discarded.
 *   Start.  x0 in raw units, clamped into the box; every start is accepted whatever its ln L.
 *   Evaluation.  Every ln L of a call -- the starts' too -- is that of the n / 2 proposals of one half-move in a compacted
 *   layout (row e H + j: walker j of the moving set of ensemble e), on u without the input transform, on ONE route decided
 *   once per call (v21_route_ensemble; csrc/routes.h: 1 = fused, 2 = two-launch): v21_mlp_loglike_fwd's decision for that
 *   layout, i.e. fused for the stacks of archs.h against the record, or when H (ensembles per spectrum) is a multiple of
 *   128; no nuisance record, no forward route flag.  v21_mlp_last_lnl_route counts an ensemble call once, whatever its
 *   sweeps and chunks; v21_mlp_last_jac_route is not touched.
 *   Results per row (v21_ensemble_out, v21_types.h): samples (raw units, x0's dtype: the walker's state after its own
 *   half-move of every thin-th kept sweep), samples_lnl, x_last, lnl_last, accept_rate, mean_u / cov_u (float64 over the
 *   n_steps kept sweeps, divided by n_steps as v21_mlp_sample's), last_prop_u, last_log_alpha, last_partner.
 *   Invariance.  A draw depends only on (seed, chain, S): results do not depend on how a run is split over calls, host
 *   chunks or devices, provided no ensemble is split -- by step0, n_warmup = 0 and a float64 x_last (exactly: the state is
 *   the float32 u), and by chain0.
 *   V21_ERR_ARG, the handle left usable: W odd, W < 2 (d + 1), W > 512, n % W != 0, a spectrum's rows not being whole
 *   ensembles, a <= 1 or not finite, and the counts outside v21_mlp_sample's ranges.  n = 0 is a no-op.
 * The host form works in chunks of whole ensembles not above 8,192 rows (whole spectra when they fit; a fused call
 * against a data matrix in multiples of lcm(W, 256) rows, so that every chunk's proposals start on a 128-row boundary --
 * where no such chunk fits the call goes two-launch) and returns when the results are in place; the _dev form never
 * synchronises.  v21_route_ensemble: the route and (chunk_rows, nullable) the host form's chunk (the _dev form: n) of a
 * call of n rows against n_data data rows (0: the record) for a handle with n_modes nuisance modes -- pure host logic. */
int v21_mlp_sample_ensemble(v21_mlp* mlp, const void* x0, int x_dtype, int64_t n, const float* data, int64_t n_data,
                            const v21_ensemble_opts* opts, const v21_ensemble_out* out, int precision, int flags);
int v21_mlp_sample_ensemble_dev(v21_mlp* mlp, const float* d_x0, int64_t ldx, int64_t n, const float* d_data, int64_t n_data,
                                const v21_ensemble_opts* opts, const v21_ensemble_out* out, int precision, int flags);
int v21_route_ensemble(int n_layers, const int* dims, const int* act, int precision, int64_t n, int64_t n_data, int n_walkers,
                       int n_modes, int flags, int host_form, int* route, int64_t* chunk_rows);

/* ---- nested sampling on forward-only ln L: the evidence and weighted posterior samples, no gradient.
 *   Target.  ln L is v21_mlp_loglike_fwd's (nuisance records and the w == 0 rule included) under the uniform prior on
 *   the box u in [-1, 1]^d, u = par_transform's coordinates.  EVERYTHING here is in u: the start rows, the dead and the
 *   live points; the caller maps to raw units (the evaluations run on u, without the input transform: the flag
 *   V21_FWD_IN_TRANSFORM is ignored and no input transform is needed).  Needs a likelihood record; d = in_dim <= 8.
 *   Rows and runs.  A call has n rows; N = n_live consecutive rows form one run, the live points of one spectrum: N even,
 *   16 <= N <= 512 (what one workgroup ranks), n % N == 0 and, with a data matrix, (n / n_data) % N == 0.  k = N / 2.  Runs
 *   are independent.  The library moves any such run; an EVIDENCE needs N >= 8 d (tests/nested_ref.py has the table:
 *   16 live points in 7 dimensions scatter by 3 nats from run to run), which the emulator classes enforce.
 *   Start.  x0 (n, d) in u, clamped into the box (NaN -> -1), or NULL: coordinate i of row r is float32(2 U(w) - 1) of
 *   word i % 4 of Philox block 2 + i / 4 of (seed, chain0 + r, step 0) -- function, key, counter and U as documented for
 *   v21_mlp_sample.  A NaN ln L is stored as -inf, here and only here (a proposal's NaN rejects).
 *   Iteration t = iter0 + its index in the call:
 *     rank    the N live ln L ascending, ties on the row index; the k lowest are the DEAD points at ranks r = 0 .. k - 1,
 *             L* is the ln L at rank k - 1; the survivor of rank r >= k moves to row r of its run;
 *     record  dead_u[t, run, r], dead_lnl[t, run, r], lstar[t, run];
 *     restart row j < k becomes a copy (u and ln L) of survivor floor(k w0 / 2^32), w0 of block 1 of (seed, chain0 +
 *             row, step t);
 *     move    n_repeats times, s = 0 ..: row j < k at x proposes y = x + gamma (x_a - x_b) in float32 (difference,
 *             product, sum, each rounded), a = floor(k w0 / 2^32), b = (a + 1 + floor((k - 1) w1 / 2^32)) mod k survivor
 *             indices (rows k + a, k + b) from block 0 of (seed, chain0 + row, step t n_repeats + s); accepted iff every
 *             coordinate of y lies in [-1, 1] and ln L(y) > L*, strictly, on the float32 values.  Survivors do not move.
 *   After the last move the N rows are the next live set: live_u / live_lnl, and x0 = live_u, iter0 + n_iter continue the
 *   run exactly (the start's ln L is evaluated again, on the same route: the same bits).
 *   Evidence.  Assembled by the caller from dead_lnl and live_lnl: after the death of rank r of iteration t the prior
 *   volume is ln X = -t s_k - sum_{i <= r} 1 / (N - i), s_k = sum_{i < k} 1 / (N - i).
 *   Evaluation.  Every ln L of a call -- the starts' too, in two halves (rows e N + h k + j, h = 0, 1) -- is that of n / 2
 *   rows in a compacted layout (row e k + j: moving slot j of run e) on ONE route decided once per call
 *   (v21_route_nested: v21_route_ensemble's decision and chunk rule with N in the place of W).  v21_mlp_last_lnl_route
 *   counts a call once.  A call makes 2 + n_iter n_repeats evaluations of n / 2 rows.
 *   Invariance.  A draw depends only on (seed, global row, global step): results do not depend on how the iterations are
 *   split over calls (iter0), nor on host chunks or on how the runs are split over calls or devices (chain0).
 *   V21_ERR_ARG, the handle left usable: N odd or out of range, n % N != 0, a spectrum's rows not being whole runs, a
 *   negative count, gamma negative, above 1e6 or not finite, (iter0 + n_iter) n_repeats >= 2^32.  n = 0 is a no-op.
 * The host form works in chunks of whole runs as v21_mlp_sample_ensemble's does and returns when the results are in
 * place; the _dev form never synchronises.  Results: v21_nested_out (v21_types.h). */
int v21_mlp_sample_nested(v21_mlp* mlp, const void* x0, int x_dtype, int64_t n, const float* data, int64_t n_data,
                          const v21_nested_opts* opts, const v21_nested_out* out, int precision, int flags);
int v21_mlp_sample_nested_dev(v21_mlp* mlp, const float* d_x0, int64_t ldx, int64_t n, const float* d_data, int64_t n_data,
                              const v21_nested_opts* opts, const v21_nested_out* out, int precision, int flags);
int v21_route_nested(int n_layers, const int* dims, const int* act, int precision, int64_t n, int64_t n_data, int n_live,
                     int n_modes, int flags, int host_form, int* route, int64_t* chunk_rows);

/* ---- linear nuisance modes (foregrounds) integrated out of the likelihood record.  Data model: d = y(x) + A^T a + noise,
 * A the (n_modes, out_dim) basis, 1 <= n_modes <= 8, with a FLAT PRIOR on the amplitudes a, which are integrated out
 * analytically.  With W = diag(w) the record's inverse variances, Q the W-orthonormalised basis (span Q = span A on the
 * bins with w > 0, Q W Q^T = I), r = d - y, b = Q W r (n_modes values) and B = Q W J^T (n_modes x in_dim), J = jac:
 *     lnL_m = -1/2 (r^T W r - |b|^2)      g_m = J W r - B^T b      F_m = J W J^T - B^T B
 * (constants that do not depend on x dropped, as in v21_mlp_loglike).  lnL_m is the profile likelihood
 * max_a lnL(d - A^T a), and it does not change when any A^T a is added to d.
 *   v21_nuisance_whiten  Q (n_modes, out_dim) and R (n_modes, n_modes, upper triangular, row-major) in float64 with
 *     sqrt(W) A^T = (sqrt(W) Q^T) R, by modified Gram-Schmidt applied twice to the column-normalised weighted basis;
 *     Q is zero where w == 0.  V21_ERR_ARG: n_modes outside 1 .. 8, a diagonal of R below 1e-10 of its mode's norm
 *     (a rank-deficient basis), fewer than n_modes + 1 bins with w > 0.  Pure host arithmetic: no context, no GPU.
 *   v21_mlp_set_nuisance  attaches the basis (float64, copied; NULL clears) to the likelihood record (required:
 *     V21_ERR_STATE without one; V21_ERR_ARG as v21_nuisance_whiten, the handle then keeps what it had).  From then on
 *     v21_mlp_loglike, v21_mlp_fisher, v21_mlp_fit and v21_mlp_sample (and their _dev forms) compute lnL_m, g_m and F_m
 *     in place of lnL, its gradient and J W J^T; F_m stays exactly symmetric.  The handle keeps the basis, Q, R and,
 *     beside the raw data, the projected data d - Q^T (Q W d) (float64, rounded to float32 once) that the reductions
 *     read: W - W Q^T Q W annihilates A, and float32 sums then see residuals of the signal's size.  A data matrix of a
 *     fit or sample call is projected the same way on the device, once per call.  A later v21_mlp_set_likelihood
 *     re-whitens with its weights (V21_ERR_ARG, nothing changed, if they make the basis rank-deficient); with NULL it
 *     clears both records.  Without a nuisance record every entry launches what it launched before.  in_dim <= 15
 *     (V21_ERR_UNSUPPORTED otherwise, v21_mlp_loglike included).
 *   v21_mlp_nuisance_info  n_modes of the handle's nuisance record, 0 without one.
 *   v21_mlp_nuisance_coef  the best-fit amplitudes of the record's raw data at every row, coef[n, :] = a_hat(x_n) =
 *     R^-1 (Q W (d_raw - y(x_n))), (n, n_modes) float64; Q W y is reduced on the device in float32, the rest is float64
 *     on the host.  V21_ERR_STATE without a nuisance record. */
int v21_nuisance_whiten(const double* basis, const float* inv_var, int32_t n_modes, int32_t out_dim, double* q, double* r);
int v21_mlp_set_nuisance(v21_mlp* mlp, const double* basis, int32_t n_modes, int32_t out_dim);
int v21_mlp_nuisance_info(v21_mlp* mlp, int32_t* n_modes);
int v21_mlp_nuisance_coef(v21_mlp* mlp, const void* x, int x_dtype, int64_t n, double* coef, int precision, int flags);

/* ---- the samplers' prior.  Without a prior record the four samplers (v21_mlp_sample, v21_mlp_sample_tempered,
 * v21_mlp_sample_ensemble, v21_mlp_sample_nested and their _dev forms) work under the uniform prior on the box
 * u in [-1, 1]^in_dim of the input transform.  A record makes the prior separable in u, one entry per input column:
 *     kind[i] = 0  uniform on [-1, 1] (mu[i] and sd[i] are not read);
 *     kind[i] = 1  normal(mu[i], sd[i]) in u, truncated to [-1, 1].
 * With ln p(u) = -1/2 sum_i ((u_i - mu_i) / sd_i)^2 over the normal columns (unnormalised, float64):
 *   v21_mlp_sample            targets L p: the gradient gains -(u - mu) / sd^2, the metric diag(1 / sd^2), log alpha
 *                             ln p(u') - ln p(u);
 *   v21_mlp_sample_tempered   the same additions, not scaled by beta: the rung at beta samples L^beta p, the rung at
 *                             beta = 0 the prior, and thermodynamic integration over mean_lnl (which stays the mean of
 *                             ln L alone) gives ln Z with respect to the NORMALISED prior; the swap rule is unchanged;
 *   v21_mlp_sample_ensemble   log alpha gains ln p(y) - ln p(x);
 *   v21_mlp_sample_nested     a move is accepted iff it is inside the box, ln L(y) > L* and log(U) < ln p(y) - ln p(x),
 *                             U = U(w0) of Philox block 4 at the move's step; a drawn start takes, in a normal column,
 *                             mu + sd Phi^-1(Phi(a) + U (Phi(b) - Phi(a))), a, b the standardised box ends and U that of
 *                             the word that draws the column without a record (float64, mirrored where a + b > 0 so
 *                             that Phi is taken in the tail nearer the mode); GIVEN starts are clamped as before, and
 *                             that they are draws of the prior is the caller's business.  The evidence is the mean of
 *                             L under the normalised prior.
 * Every ln L a sampler returns stays ln L.  v21_mlp_loglike, v21_mlp_fisher, v21_mlp_fit and v21_mlp_jacobian do not
 * read the record.
 *   v21_mlp_set_prior  kind, mu, sd: in_dim entries each (copied).  in_dim = 0 or kind = NULL clears the record; a
 *     record whose kinds are all 0 is no record: the samplers then launch what they launched before.  V21_ERR_ARG, the
 *     handle keeping what it had: in_dim is not the stack's (or above 8); a kind outside {0, 1}; for a normal column mu
 *     or sd NULL, sd not finite or below 1e-3, mu not finite or more than 5 sd outside the box (past that the truncated
 *     normal's mass in the box cannot be formed reliably, and such a prior contradicts the emulator's domain).  Pure
 *     host bookkeeping: no GPU work. */
int v21_mlp_set_prior(v21_mlp* mlp, const int32_t* kind, const double* mu, const double* sd, int32_t in_dim);

/* ---- the samplers' held parameters.  A hold record takes input columns out of the four samplers (the entries listed
 * above): a held column i is no parameter of the call but the constant u_i = float32(u[i]) -- rounded ONCE, here, and that
 * float32 is what every state, proposal, stored sample, x_last, dead_u and live_u carries in the column, bit for bit.
 * Its prior is never read (a normal column of the prior record that is held counts as uniform); d_free = the columns
 * left.  No sampler entry changes its signature; with a record
 *   v21_mlp_sample[_tempered]  the start's held coordinates are overwritten; at every point, after the prior's additions,
 *                             g_i = 0, F_ij = F_ji = 0 (j != i), F_ii = 1 (v21_mlp_fit_map's arithmetic), the ridge is
 *                             added to the free pivots only, the held normal is 0 (the free columns draw from the words
 *                             they always drew from), and log q is normalised with d_free: the transition is that of
 *                             the d_free-dimensional sampler on the free block of F + P + ridge I;
 *   v21_mlp_sample_ensemble    the starts' held coordinates are overwritten; log alpha takes (d_free - 1) ln z.  The
 *                             stretch returns a held coordinate exactly: x + z (x - x) = x in float arithmetic;
 *   v21_mlp_sample_nested      given and drawn starts get the held coordinates (a held column consumes no draw; the free
 *                             columns keep their words); the difference move returns them exactly.  The shrinkage and
 *                             v21_nested_evidence are untouched: the evidence is the mean of L under the normalised prior
 *                             of the free columns, at the held values;
 *   results                   mean_u of a held column is u_i, its row and column of cov_u are exact zeros.
 * (n_walkers and n_live keep their rules on in_dim, n_repeats = 0 stays 3 in_dim.)  v21_mlp_fit, v21_mlp_fit_map (which
 * keeps the hold mask of its own options), v21_mlp_fisher, v21_mlp_loglike and v21_mlp_loglike_fwd do not read the record.
 *   v21_mlp_set_hold  hold, u: in_dim entries each (copied); hold[i] in {0, 1}, u[i] read only where hold[i] is 1.
 *     hold = NULL, in_dim = 0 or an all-zero mask clears the record: the samplers then launch what they launched before.
 *     V21_ERR_ARG, the handle keeping what it had: in_dim is not the stack's (or above 8); a mask entry outside {0, 1};
 *     a held u NULL, not finite or outside [-1, 1]; every column held (nothing to sample).  Pure host bookkeeping. */
int v21_mlp_set_hold(v21_mlp* mlp, const int32_t* hold, const double* u, int32_t in_dim);

/* ---- trainer: replaces Model.compile + Model.fit (emulator.py:369-378, :739-747,
 * :756-764; optimizer/loss from notebooks/Training.ipynb cells 4 and 10). ------- */
typedef struct {
  float lr, beta1, beta2, eps; /* Keras Adam: 1e-3, 0.9, 0.999, 1e-7 */
} v21_adam;

/* The stack's output layer must be linear (V21_ERR_UNSUPPORTED otherwise): the reference's output Dense has no
 * activation (emulator.py:44), and the loss gradient is taken with respect to the Dense output. */
int v21_trainer_create(v21_mlp* mlp, int precision, int max_batch, v21_trainer** out);
int v21_trainer_destroy(v21_trainer* tr);
int v21_trainer_set_adam(v21_trainer* tr, const v21_adam* cfg);
int v21_trainer_set_lr(v21_trainer* tr, float lr);
int v21_trainer_get_lr(v21_trainer* tr, float* lr);
/* Resident training / validation matrices.  y == NULL means y = x (autoencoder fit,
 * emulator.py:739-741).  row_weight w_i defines the loss: loss_i = w_i sum_j (y-p)^2
 * (relative_mse_loss, emulator.py:68-81 -> w_i = 1/(D amp_i^2); plain MSE -> 1/D). */
int v21_trainer_set_data(v21_trainer* tr, int which /*0 train, 1 val*/, const float* x,
                         const float* y, const float* row_weight, int64_t n);
/* One Keras epoch: rows visited in `perm` order (n_train int32; NULL = in order),
 * batches of `batch` with the partial last batch kept, epoch loss =
 * sum(batch_loss * n_b) / N.  With a communicator attached each rank takes its
 * slice of every global batch and gradients are all-reduced (sum) before Adam. */
int v21_trainer_run_epoch(v21_trainer* tr, const int32_t* perm, int batch, double* loss);
/* validation pass (which = 1) or loss over the training set (which = 0).  f16 / bf16 trainers on the chain kernel
 * evaluate the whole split in ONE forward-only launch (`batch` is then only validated); f32 trainers walk it in
 * batches of min(batch, max_batch). */
int v21_trainer_eval(v21_trainer* tr, int which, int batch, double* loss);
/* device pointers of the resident split `which` (v21_trainer_set_data): x (n, in_dim), y (n, out_dim; the same pointer as x
 * when the split was set with y == NULL), row weights (n) -- for custom loops that step on slices of the resident training
 * set with v21_trainer_step_dev (a step that reads rows of the resident training inputs lets the fused training kernels gather
 * their 16-bit copy: half the bytes of the step's largest read).  Valid until the next set_data of that split. */
int v21_trainer_get_data_dev(v21_trainer* tr, int which, const float** x, const float** y, const float** row_weight, int64_t* n);
/* single optimizer step on caller-provided device batch (bench / custom loops) */
int v21_trainer_step_dev(v21_trainer* tr, const float* d_x, const float* d_y,
                         const float* d_row_weight, int n_rows, int global_rows);
int v21_trainer_last_step_loss(v21_trainer* tr, double* loss); /* syncs */
/* optimizer state: iter + m + v (Keras optimizer_weights order = arena order) */
int v21_trainer_get_state(v21_trainer* tr, int64_t* iter, float* m, float* v, size_t n);
int v21_trainer_set_state(v21_trainer* tr, int64_t iter, const float* m, const float* v,
                          size_t n);
/* gradient of the last step (after all-reduce), for tests */
int v21_trainer_get_grad(v21_trainer* tr, float* g, size_t n);
/* ---- joint step (BASELINE configs[2]).  The reference trains the autoencoder, THEN encodes the
 * training signals with the finished encoder and trains the latent emulator on those latents
 * (emulator.py:739-764).  A joint epoch takes one optimizer step of EACH model on the same rows of every
 * batch; the emulator's targets are the latents the encoder produces for those rows in that step (no
 * gradient flows back into the encoder).  With the autoencoder's learning rate at 0 it is exactly the
 * reference's second phase.  `ae` holds the signals (set_data(0, signals, NULL, w)), `em` the parameters of the
 * same rows (its y argument is ignored); latent_layer = index of the encoder's linear output layer in `ae`'s
 * stack (linear, or the V21_ACT_GAUSS head: the emulator then learns z_mean).  Two f16 / bf16 trainers (chain kernel), or
 * two f32 trainers of max_batch <= 2,048 (the reference's arithmetic); with a
 * communicator on the context every rank carries its share of every batch and each model's gradients are exchanged as
 * in a plain step.  losses[0] = autoencoder, losses[1] = emulator. */
typedef struct v21_joint v21_joint;
int v21_joint_create(v21_trainer* ae, v21_trainer* em, int latent_layer, v21_joint** out);
int v21_joint_destroy(v21_joint* j);
int v21_joint_run_epoch(v21_joint* j, const int32_t* perm /* nullable */, int batch, double* losses /* [2] */);
/* Validation of both models in one launch on the trainers' validation sets (set_data(1, ...): signals for `ae`, the
 * parameters of the same rows for `em`): losses[0] = the autoencoder's validation loss, losses[1] = the emulator's loss
 * against the latents the CURRENT encoder produces for the validation signals (emulator.py:754 without the host round
 * trip). */
int v21_joint_eval(v21_joint* j, double* losses /* [2] */);
/* Captured-step replay (hipGraph): run_epoch / step_dev capture one optimizer step per
 * batch geometry and replay it; first row, Adam step size and loss slot of each step come from a device
 * table.  Bit-identical to eager launches.  Off by default (the steps are GPU-bound on MI355X: replay frees
 * the host thread, it does not shorten a step); V21_ERR_UNSUPPORTED with a communicator or a
 * V21_ACT_GAUSS layer.  Replaces nothing in the reference (Keras fit, emulator.py:369-378, has no analogue). */
int v21_trainer_use_graph(v21_trainer* tr, int enable);
/* diagnostics ("race detection / sanitizers": GPU AddressSanitizer is not available on this
 * pool): fills the whole LDS of every CU with `pattern` (e.g. 0xFFFFFFFF = NaN as fp32, f16 and bf16) and returns
 * when that is done.  The poison tests launch it immediately before each kernel that keeps activations in LDS, so
 * that a column or mask tile read before it is written meets NaN instead of a fresh process's zeros. */
int v21_debug_poison_lds(v21_ctx* ctx, uint32_t pattern);
/* diagnostics: the shader clock UNDER LOAD.  start: one wave on a private stream samples the shader-clock cycle counter
 * against the constant 100 MHz reference counter every period_us for duration_ms, beside whatever runs on the context's
 * stream meanwhile; read: waits for it; mean / min / max of cycles per nanosecond over the sampling intervals.
 * bench.py reports it as roofline.clock_ghz (DVFS holds ~1.6-1.9 GHz under the fused kernel, 2.4 GHz is nominal). */
int v21_debug_clock_probe_start(v21_ctx* ctx, double duration_ms, double period_us);
/* diagnostics (r5): the shader clock FROM THE TIMED KERNEL ITSELF.  Launches the headline stack's fused kernel (archs.h
 * S1; f16 / bf16) in a separate instantiation whose wave 0 of every workgroup reads s_memtime (shader-clock cycles),
 * s_memrealtime (constant 100 MHz) and HW_REG_XCC_ID when the workgroup starts and when it ends.  d_stamps (device
 * memory): five 64-bit words per workgroup = ceil(n / 128) workgroups: [cycles at start, 100-MHz ticks at start, cycles at
 * end, ticks at end, XCD 0-7 in bits 0-3 | HW_REG_HW_ID of the workgroup's wave 0 in bits 8-39].  (end - start) cycles / ticks * 0.1 = GHz as that workgroup's CU saw it; bench.py reports
 * mean / min / max per XCD over a repeat of its K timed launches.  Otherwise the arguments of v21_mlp_forward_dev. */
int v21_debug_forward_clocked(v21_mlp* mlp, const float* d_x, int64_t ldx, int64_t n, float* d_y, int64_t ldy, int precision,
                              int flags, unsigned long long* d_stamps);
int v21_debug_clock_probe_read(v21_ctx* ctx, double* ghz_mean, double* ghz_min, double* ghz_max, int* samples);
/* diagnostics: the small-batch f32 chain kernel (csrc/train_chain32s.h) follows a host-built job table into the packed
 * weight streams without range checks; v21_trainer_create validates every address a row names against the allocated
 * streams (V21_ERR_STATE instead of a GPU memory fault).  This repeats that check against stream sizes the caller names
 * (bytes; negative = the real ones): the tests hand in a truncated stream.  V21_ERR_UNSUPPORTED for trainers on other paths. */
int v21_debug_check_chain_jobs(v21_trainer* tr, long long fw_bytes, long long bw_bytes);
/* ---- routes: WHICH kernels a call takes (csrc/routes.h holds the one decision the dispatch sites and these queries
 * share; INTEGRATION.md section 6 is the table, tests/test_routes.py asserts it).  The reference has one path (Keras:
 * emulator.py:369-378, 402); the library has several kernels for the same arithmetic, chosen from precision, row count,
 * stack and rank count.  The two v21_route_* queries are pure host logic (no GPU, no handles):
 *   v21_route_forward  the route v21_mlp_forward_dev takes for n rows of this stack (rt_ready: assume the run-time
 *                      instantiated kernel of a stack outside archs.h has arrived); route: 1 small (one NT launch per
 *                      layer), 2 fused_fwd compiled in, 3 fused_fwd instantiated at run time, 4 table-driven chain
 *                      kernel in FORWARD mode, 5 generic per-layer GEMM.
 *   v21_route_train    one optimizer step of `rows` rows of a trainer created with max_batch, on `nranks` ranks
 *                      (rt_ready: assume the run-time instantiated fused TRAINING kernel of a stack outside archs.h has arrived):
 *                      fwd: 1 per-layer NT, 2 train_chain_kernel (16-bit), 3 fused_train (128-row workgroups),
 *                      4 fused_train16 (64-row workgroups), 5 train_chain32_kernel, 6 / 7 train_chain32s_kernel<8> / <4>;
 *                      upd: 1 per-layer NT + adam_repack, 2 dw16_adam_kernel, 3 gemm_dw16[_lds] split-K + adam_repack,
 *                      4 dwadam32_kernel, 5 gemm_nt_dwadam_kernel, 6 sliced NT + adam_repack.
 * v21_mlp_last_route / v21_trainer_last_route report what the LAUNCH SITES recorded for the last call / eager step and
 * how many calls / steps took each route since creation (counts[route]; nullable).  v21_route_name: kind 0 forward,
 * 1 training forward, 2 update. */
int v21_route_forward(int n_layers, const int* dims, const int* act, int precision, int64_t n, int flags, int rt_ready, int* route);
int v21_route_train(int n_layers, const int* dims, const int* act, int precision, int max_batch, int rows, int nranks, int rt_ready, int* fwd, int* upd);
int v21_mlp_last_route(v21_mlp* mlp, int* route, long long counts[8]);
int v21_trainer_last_route(v21_trainer* tr, int* fwd, int* upd, long long fwd_counts[8], long long upd_counts[8]);
const char* v21_route_name(int kind, int route);
/* r5: where an eager optimizer step's time goes, by HIP events on the context's stream.  v21_trainer_phase_timing(tr, n,
 * cut) stamps the next n steps (n = 0: off) with TWO events each -- the step's start and one cut point:
 *   cut 1 after forward + loss + activation gradients (the chain / fused training launch, its stream pack included),
 *   cut 2 after the weight gradients (+ slab sums),  cut 3 after the gradient exchange has been joined,  cut 4 after Adam +
 *   packed copies (the whole step);
 * v21_trainer_phase_times returns the MEDIAN milliseconds from start to cut over the steps stamped since the last call.
 * A HIP event is a packet of its own (an empty interval between two reads ~5 us): the phases are DIFFERENCES of the
 * cumulative times of separate runs, in which the marker's cost cancels (21cmvae_amd/_native.py: Trainer.phase_profile).
 * Single-rank steps whose gradients and Adam are ONE launch have cut 2 = cut 3 = cut 1; the per-layer path has cut 1 = cut 2
 * = everything before the exchange.  Steps of a joint object or a sweep are not stamped. */
int v21_trainer_phase_timing(v21_trainer* tr, int steps, int cut);
int v21_trainer_phase_times(v21_trainer* tr, double* ms, int* steps);
/* diagnostics: which route the eager 16-bit steps of this trainer took since it was created:
 * out[0] steps through the 32-row chain kernel (csrc/train_chain.h), out[1] steps through the fused training kernel
 * (csrc/fused_train.h), out[2] of those that had to launch pack_stream_kernel first (the others found the kernel's
 * weight stream already written by the previous step's Adam pass), out[3] Adam passes that wrote that stream.
 * The tests assert on these so that "fused route == chain route" cannot pass with both taking the same kernel. */
int v21_debug_trainer_counters(v21_trainer* tr, long long out[4]);
/* diagnostics: s_memtime stamps of workgroup 0 of the last chain-kernel launch (train_chain.h):
 * [0] start, [1] batch gathered, [2..L+1] after forward layer l, [L+2] loss reduced,
 * [L+3..] after each backward layer (top down).  Off by default (a stamp holds its wave for ~600 cycles and the
 * other waves meet it at the next barrier: eleven stamps were 2-3 us of every step until r3); enable_stamps turns
 * them on for the launches that follow (steps already recorded into graphs keep what they were recorded with).
 * V21_ERR_STATE when the trainer runs the per-layer path (variational f32 or >512-wide stacks) or stamps are off. */
int v21_trainer_enable_stamps(v21_trainer* tr, int enable);
int v21_trainer_chain_stamps(v21_trainer* tr, uint64_t* out, int n);
/* Variational mode of a stack with a V21_ACT_GAUSS layer (A13; build-side extension, no
 * reference arithmetic exists for it): loss_i = recon_i + kl_weight * KL_i,
 * KL_i = -1/2 sum_d (1 + lv - mu^2 - exp lv).  sample = 0 -> eps = 0 (with kl_weight = 0
 * this is exactly the deterministic autoencoder of emulator.py:517); otherwise eps is a
 * counter-based standard normal keyed on (seed, step, row of the global batch, d) --
 * restated in oracle/ref_numpy.py:gauss_eps.  Evaluation passes use eps = 0. */
int v21_trainer_set_vae(v21_trainer* tr, float kl_weight, int sample, uint64_t seed);

/* ---- sweep: several models trained in lock step on ONE shared batch stream (BASELINE
 * configs[4]: "64 concurrent latent-dim/hidden-width configs packed as batched GEMM", 8 per
 * GPU).  New: the reference trains one model per fit() call (emulator.py:739-747); a sweep
 * runs the same fit arithmetic for every model, with phase k of the step (layer k forward,
 * loss, layer k backward, Adam) issued as one grouped launch for all models.  The trainers
 * must share context, precision, max_batch, depth, activations and in/out width (hidden and
 * latent widths differ); trainer 0 holds the training set (v21_trainer_set_data).  Each
 * trainer keeps its own Adam settings, state and weights and can be used on its own
 * (eval, get_state, ...) between sweep epochs.  count <= 64 (r5; 16 until r4: configs[4] names 64
 * concurrent configs, and a group of 8 models x 8 row blocks leaves three quarters of the chip idle). */
typedef struct v21_sweep v21_sweep;
int v21_sweep_create(v21_trainer** trainers, int count, v21_sweep** out);
int v21_sweep_destroy(v21_sweep* sw); /* the trainers stay alive */
/* one Keras-style epoch of every model (same shuffle, same batches); losses[count] */
int v21_sweep_run_epoch(v21_sweep* sw, const int32_t* perm, int batch, double* losses);

/* ---- data-parallel communicator (new: the reference is single-process, emulator.py:369,739,756).  One
 * process per GPU; every rank trains on its contiguous share of each global batch and the gradients are summed
 * before Adam.  Two transports behind the same step logic:
 *   v21_comm_init       RCCL inside the library (librccl.so.1 is dlopen'ed, so a single-GPU user needs none):
 *                       ncclAllReduce, or ncclReduceScatter + ncclAllGather in sharded mode, on the context stream.
 *   v21_comm_init_host  collectives supplied by the host as callbacks on page-locked HOST buffers (the library
 *                       stages device -> host -> device around them): any transport the host has -- the test
 *                       suite runs two ranks on one GPU over torch.distributed/gloo through it.
 * v21_comm_set_sharded(1): reduce-scatter of the gradient arena -> each rank applies Adam to its 1/R slice of
 * (w, m, v) only -> all-gather of the updated weights; 0 (default): one all-reduce, identical
 * Adam on every rank.  In sharded mode v21_trainer_get_state is a collective call (it gathers m and v).  Switching
 * the mode of a context does not touch trainers that already exist on it: after sharded steps a rank holds current
 * moments for ITS slice only, so call v21_trainer_get_state + v21_trainer_set_state (or create a new trainer) before
 * such a trainer goes on in all-reduce mode. -------- */
#define V21_COMM_ID_BYTES 128
typedef struct v21_comm_host_ops {
  void* user;
  /* all blocking, 0 = ok; buffers are host memory of nranks * n_per (or n) floats, results in place */
  int (*allreduce_sum_f32)(void* user, float* buf, size_t n);
  int (*reduce_scatter_sum_f32)(void* user, float* buf, size_t n_per); /* rank r: sums of [r n_per, (r+1) n_per) there */
  int (*allgather_f32)(void* user, float* buf, size_t n_per);          /* rank r contributes [r n_per, (r+1) n_per) */
} v21_comm_host_ops;
int v21_comm_get_unique_id(v21_ctx* ctx, void* id /* V21_COMM_ID_BYTES */);
int v21_comm_init(v21_ctx* ctx, int nranks, int rank, const void* id);
int v21_comm_init_host(v21_ctx* ctx, int nranks, int rank, const v21_comm_host_ops* ops);
/* r5: a communicator WITHOUT a transport: the context reports `nranks` ranks, a trainer on it computes this rank's share
 * of every global batch and takes the N > 1 step structure (operands -> weight gradients -> [exchange: nothing] -> Adam),
 * so the compute side of a data-parallel step can be timed on ONE GPU (bench.py: dp_compute_only).  The gradients are
 * NOT summed over anything: results are those of a rank whose peers contributed zeros. */
int v21_comm_init_null(v21_ctx* ctx, int nranks, int rank);
/* r5: the all-reduce form's gradient exchange in 1 message (default: the whole arena + loss slot after all weight
 * gradients) or 2: the weight gradients are formed in two launches, the output-side layers first; their half of the arena
 * (and the loss slot) is all-reduced on a second stream while the input-side layers' gradients are still being formed.
 * Same sums per element; with two ranks bit-identical to the one-message form.  Applies to 16-bit chain trainers in
 * all-reduce mode; every rank of a communicator must set the same value. */
int v21_comm_set_buckets(v21_ctx* ctx, int buckets);
int v21_comm_destroy(v21_ctx* ctx);
int v21_comm_set_sharded(v21_ctx* ctx, int on);
/* what the attached communicator reports about itself (RCCL: ncclCommCount / ncclCommUserRank); transport: 0 none,
 * 1 RCCL inside the library, 2 host-staged callbacks.  bench.py prints it beside the data-parallel legs. */
int v21_comm_info(v21_ctx* ctx, int* nranks, int* rank, int* transport);
int v21_comm_allreduce_f32(v21_ctx* ctx, float* d_buf, size_t n);           /* sum, in place */
int v21_comm_reduce_scatter_f32(v21_ctx* ctx, float* d_buf, size_t n_per);  /* in place over nranks * n_per floats */
int v21_comm_allgather_f32(v21_ctx* ctx, float* d_buf, size_t n_per);       /* in place over nranks * n_per floats */

#ifdef __cplusplus
}
#endif
#endif /* V21_H */
