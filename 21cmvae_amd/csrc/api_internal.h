// api_internal.h -- what the translation units of the C ABI share (r4: v21_api.hip, one 3,300-line file until then, is
// now api_base.hip (errors, contexts, memory, events, communicator, diagnostics), api_forward.hip (dense stacks and the
// forward routes), api_trainer.hip (trainers, the step machinery, captured steps), api_sweep.hip and api_joint.hip --
// all behind the unchanged include/v21.h).  Kernels live in the headers included below; a kernel template is
// instantiated by the unit that launches it, non-template kernels have internal linkage.  The fused kernels of archs.h
// are the exception: fused_inst.hip instantiates them, one object each, from the family traits of fused_families.h, and
// the units reach them through the launcher tables of compiled.h.  Device memory of a handle is owned by its Dev
// members (below): nothing here or in the units frees a handle's buffer by hand.
#pragma once
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

// the library is built with -fvisibility=hidden: only what include/v21.h declares is exported
#pragma GCC visibility push(default)
#include "../../include/v21.h"
#pragma GCC visibility pop
#include "compiled.h"
#include "fused_fwd.h"
#include "jit.h"
#include "gemm.h"
#include "gemm_nt.h"
#include "train_kernels.h"
#include "train_chain.h"
#include "train_chain32.h"
#include "train_chain32s.h"
#include "dw_adam32.h"
#if defined(V21_CHAIN_FINE) || defined(V21_T_STAMPS)
constexpr int kStampSlots = 2048;  // (diagnostic builds: per-wave / per-workgroup stamps)
#else
constexpr int kStampSlots = 64;
#endif
#include "dw_adam.h"
#include "routes.h"
#include "rowmath.h"

// act.h's codes are include/v21.h's
static_assert(v21::kActLinear == V21_ACT_LINEAR && v21::kActRelu == V21_ACT_RELU && v21::kActGauss == V21_ACT_GAUSS &&
              v21::kActTanh == V21_ACT_TANH && v21::kActSigmoid == V21_ACT_SIGMOID && v21::kActElu == V21_ACT_ELU &&
              v21::kActSoftplus == V21_ACT_SOFTPLUS, "csrc/act.h and include/v21.h agree on the activation codes");
static inline bool act_known(int code) { return code >= V21_ACT_LINEAR && code <= V21_ACT_SOFTPLUS; }

namespace v21 { struct FitRow; }  // fit_kernels.h (api_fit.hip); both row states are built on rowmath.h
namespace v21 { struct SampleRow; struct TemperRow; }  // sample_kernels.h (api_sample.hip)
namespace v21 { struct EnsRow; }  // ensemble_kernels.h (api_ensemble.hip)
namespace v21 { struct NestRow; }  // nested_kernels.h (api_nested.hip)
using namespace v21;

// ---- errors: v21_last_error() returns the calling thread's last message (api_base.hip)
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
#define HIPCHK(expr)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail(V21_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),    \
                  __FILE__, __LINE__);                                                    \
  } while (0)
#define CHK(expr)            \
  do {                       \
    int r_ = (expr);         \
    if (r_ != V21_OK) return r_; \
  } while (0)
static inline long long p16(int d) { return (d + 15) & ~15; }  // row pitch: whole 16-float groups
// Zeroed bytes behind every packed weight stream of the chain kernels: two 4-KiB chunks.  A stream is whole chunks, so
// its end is a page boundary; the rolling prefetch requests addresses AHEAD of what it uses, and a request must never
// leave the allocation (train_chain32s.h: the r3 abort).
constexpr size_t kChainStreamSlack = 8192;
// floats behind the P parameters of an arena: the loss slot, then room to round P + 1 up to whole shards of up to
// 64 ranks (sharded data-parallel Adam works on nranks * ceil((P + 1) / nranks) elements in place)
constexpr size_t kArenaPad = 4 + 64;

// ---- device memory: every device allocation of a handle (v21_ctx, v21_mlp, v21_trainer, v21_sweep, v21_joint) is a Dev
// member of it.  A grow-only allocation of T elements: reserve(count) reallocates only to grow (the old block is freed
// first, so two copies are never live; capacity 0 if the allocation fails), zeroed(count, st) also clears those elements
// on st, release() frees, and so does the destructor -- which is why every v21_*_destroy makes the device current and
// drains the handle's stream(s) BEFORE it deletes the handle, and why a create function that fails half way leaks nothing.
// Converts to T*; get() spells the pointer out where a type is deduced from it (kernel-launch arguments).
template <class T>
struct Dev {
  T* p = nullptr;
  size_t n = 0;  // capacity, elements
  Dev() = default;
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
  ~Dev() { release(); }
  int reserve(size_t count) {
    if (n >= count) return V21_OK;
    if (p) { HIPCHK(hipFree(p)); p = nullptr; }
    n = 0;
    HIPCHK(hipMalloc((void**)&p, count * sizeof(T)));
    n = count;
    return V21_OK;
  }
  int zeroed(size_t count, hipStream_t st) {
    CHK(reserve(count));
    HIPCHK(hipMemsetAsync(p, 0, count * sizeof(T), st));
    return V21_OK;
  }
  void release() {
    if (p) hipFree(p);
    p = nullptr;
    n = 0;
  }
  T* get() const { return p; }
  operator T*() const { return p; }
};

// ---- context (api_base.hip)
typedef void* nccl_comm;  // (rccl.h is not included: librccl is dlopen'ed by api_base.hip)
struct v21_ctx {
  int device = 0;
  hipStream_t own = nullptr, stream = nullptr;
  nccl_comm comm = nullptr;
  int nranks = 1, rank = 0;
  // host-staged collectives (v21_comm_init_host): the same data-parallel logic over any transport the host has
  bool host_comm = false;
  v21_comm_host_ops host{};
  float* h_stage = nullptr;
  size_t h_stage_n = 0;
  int sharded = 0;  // 1: reduce-scatter -> Adam on this rank's shard -> all-gather (v21_comm_set_sharded)
  // r5: a communicator WITHOUT a transport (v21_comm_init_null): this rank computes its share of every global batch and
  // takes the N > 1 step structure (operands -> gradients -> [exchange: nothing] -> Adam), so that the compute side of a
  // data-parallel step can be timed on one GPU (bench.py: dp_compute_only)
  bool null_comm = false;
  // r5: the gradient exchange in `buckets` messages (v21_comm_set_buckets; 1 = one message after all weight gradients,
  // 2 = the upper layers' half leaves on comm_stream while the lower layers' gradients are still being formed)
  int buckets = 1;
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_bucket[2] = {nullptr, nullptr}, ev_comm_done = nullptr;
  // v21_mlp_forward on many rows: results leave over PCIe on a second stream, slice by slice, while the next slice
  // is being computed (created on first use)
  hipStream_t copy_stream = nullptr;
  hipEvent_t slice_done[2] = {nullptr, nullptr};
  // v21_debug_clock_probe_*: the sampling wave runs on its own stream beside the kernels under test
  hipStream_t probe_stream = nullptr;
  Dev<unsigned long long> d_probe;  // 2 * probe_cap() stamps, then the sample count
  int probe_cap() const { return d_probe.n ? (int)((d_probe.n - 1) / 2) : 0; }
};
int use(v21_ctx* c);

// ---- the chain kernels' packed weight streams (train_chain.h, train_chain32.h, train_chain32s.h), by format: where layer
// l's fragments start in the forward and the backward stream (elements), the fragment and tile counts of a width, the
// streams' bytes (an allocation adds kChainStreamSlack).  A trainer's Adam pass writes the streams that the forward route
// of its stack reads: both take the layout from here.
enum ChainFmt { CHAIN_FMT_16, CHAIN_FMT_32, CHAIN_FMT_32S };  // 16-bit; fp32 in 32-feature tiles; fp32 in 64-feature tiles
struct ChainLayout {
  ChainFmt fmt = CHAIN_FMT_16;
  std::vector<long long> fw_off, bw_off;
  long long fw_bytes = 0, bw_bytes = 0;
  int esize() const { return fmt == CHAIN_FMT_16 ? 2 : 4; }
  int frags(int d) const { return fmt == CHAIN_FMT_16 ? chain_steps(d) : fmt == CHAIN_FMT_32S ? chain32s_frags(d) : chain32_frags(d); }
  int tiles(int d) const { return fmt == CHAIN_FMT_32S ? (d + 63) / 64 : (d + 31) / 32; }
  // layer l (c.K -> c.N) for a chain kernel: KS / NT / NS / KT, the offsets in units of one lane's 16 bytes
  void layer(ChainLayer& c, int l) const {
    c.KS = frags(c.K); c.NT = tiles(c.N); c.NS = frags(c.N); c.KT = tiles(c.K);
    c.fw_off = fw_off[l] / (16 / esize()); c.bw_off = bw_off[l] / (16 / esize());
  }
  // ... and for the Adam pass that packs the streams: KS / NS, the offsets in elements
  void layer(AdamLayer& a, int l) const { a.fw_off = fw_off[l]; a.bw_off = bw_off[l]; a.KS = frags(a.K); a.NS = frags(a.N); }
};

// ---- a nuisance record as the host builds it (api_nuisance.hip): Q (K, out) and R (K, K) of v21_nuisance_whiten, Q W d of
// the record's raw data (K), and what the device holds: Q in float32 and the projected data d - Q^T (Q W d)
struct NuisRecord {
  std::vector<double> q, r, cd;
  std::vector<float> qf, proj;
};

// ---- dense stack (api_forward.hip)
struct v21_mlp {
  v21_ctx* ctx = nullptr;
  int L = 0;
  std::vector<int> dims, act;
  std::vector<long long> w_off, b_off;
  size_t nparams = 0;
  Dev<float> d_w;  // nparams + kArenaPad floats
  int fused_id = -1;
  Dev<unsigned char> d_stream[3];
  bool stream_ok[3] = {false, false, false};
  bool has_tin = false, has_tout = false;
  v21_affine_in tin{};
  float out_std = 1.f;
  Dev<float> d_mean;
  Dev<float> d_act[2];  // generic path scratch
  // host-API staging
  Dev<float> d_xs, d_ys;
  Dev<double> d_xs64;  // float64 rows of v21_mlp_forward awaiting the float64 par_transform
  int maxdim = 0;
  bool wpad_ok = false;  // false after the arena was rewritten from outside a trainer (set_weights)
  // small-batch latency path: fp32 W^T copies + two padded activation images
  Dev<float> d_wt;
  std::vector<long long> wt_off;
  bool wt_ok = false;
  Dev<float> d_small[2];
  Dev<float> d_xpad;  // host-API staging of zero-padded input rows
  // one-launch forward of ANY stack up to 512 wide in f16 / bf16 (train_chain.h, FORWARD mode): the packed forward
  // weight stream per precision (+ the backward stream the packing kernel writes beside it), rebuilt lazily
  Dev<unsigned char> d_cfw[3], d_cbw[3];
  bool cfw_ok[3] = {false, false, false};
  ChainLayout clay[2];  // [0]: 16-bit streams, [1]: fp32 (train_chain32.h); filled on first use
  Dev<v21_affine_in> d_tin;  // device copy of the input transform
  // fused_fwd<this stack, precision> instantiated at run time (jit.h) for stacks outside archs.h; requested on the
  // first large forward call, used once its code object is there
  v21::JitKernel* jit[3] = {nullptr, nullptr, nullptr};
  bool jit_asked[3] = {false, false, false};
  // routes.h: the route of the last v21_mlp_forward_dev call and how many calls took each (v21_mlp_last_route)
  int last_route = 0;
  long long route_count[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long* clk_stamps = nullptr;  // set for the duration of v21_debug_forward_clocked
  // width of layer l's Dense output: dims[l+1], or 2*dims[l+1] = [z_mean | z_log_var] for V21_ACT_GAUSS
  int nw(int l) const { return act[l] == V21_ACT_GAUSS ? 2 * dims[l + 1] : dims[l + 1]; }
  // parameter Jacobian, log-likelihood, Fisher matrices and fits (api_jacobian.hip, api_fit.hip): the likelihood record
  // (d, 1 / sigma^2; out_dim floats each) and the route of the last call (routes.h: JacRoute).  Buffers, grown on demand:
  Dev<float> lk_data, lk_w;
  Dev<float> lk_ws;      // y and jac of one kLkSlice slice of rows before they are reduced
  Dev<float> jxt, jfac;  // transformed rows and their factors, pitch in_dim (jac_prep)
  Dev<double> hin;       // the host forms' chunk: its raw rows (float32 or float64) ...
  Dev<char> stage;       // ... and its results with its further inputs (ChunkStage)
  Dev<FitRow> fit;       // fit state (fit_kernels.h), then F / ln L / gradient of its rows, running rows per iteration, data
  Dev<float> fF, fl, fg, fdata;
  Dev<int> fit_cnt;
  Dev<SampleRow> smp;    // chain state of a sample call (sample_kernels.h; its evaluations land in fF / fl / fg)
  Dev<TemperRow> tmp;    // a tempered sample call's sums of ln L and swap counts per row
  Dev<EnsRow> ens;       // walker state of an ensemble call (ensemble_kernels.h) ...
  Dev<float> ens_prop, ens_lnl;  // ... and the compacted proposals of one half-move (n / 2 rows) with their ln L
  Dev<NestRow> nst;      // live points of a nested call (nested_kernels.h; its proposals share ens_prop / ens_lnl)
  bool has_lk = false;
  // the samplers' prior record (api_prior.hip: v21_mlp_set_prior), as their step kernels take it by value; without one
  // (has_prior false: never set, cleared, or every column uniform) they run their PRIOR = false instantiations
  bool has_prior = false;
  PriorArgs prior{};
  // the samplers' hold record (api_hold.hip: v21_mlp_set_hold), as their init, step and finish kernels take it by value;
  // without one (has_hold false: never set, cleared, or nothing held) they run their HOLD = false instantiations, which
  // take no such argument.  Read by the four samplers' launch sites alone (through SamplerRecords)
  bool has_hold = false;
  HoldArgs hold{};
  // linear nuisance modes marginalised in those reductions (api_nuisance.hip): nu_k modes (0: none), the float64 basis
  // as it was handed in, the record built from it, and the host copy of the likelihood record both are re-whitened from.
  // On the device: Q in float32 (the reductions) and float64 (nuis_project_kernel), the record's projected data BESIDE
  // the raw data, and the projected rows of a fit or sample call's data matrix.
  int nu_k = 0;
  std::vector<double> nu_basis;
  NuisRecord nu;
  std::vector<float> lk_h_data, lk_h_w;
  Dev<float> nu_qf, lk_proj, nu_ws;
  Dev<double> nu_qd;
  // the data the record's reductions read
  const float* lk_read() const { return nu_k ? lk_proj.get() : lk_data.get(); }
  int last_jac_route = 0;
  long long jac_route_count[4] = {0, 0, 0, 0};
  // fused_jac<this stack, precision> instantiated at run time (jit.h: kJitJac), only for a handle that ASKED
  // (v21_mlp_jit_jacobian, or a call with V21_FWD_FORCE_JIT): routes.h JAC_FUSED_RT
  v21::JitKernel* jac_jit[3] = {nullptr, nullptr, nullptr};
  bool jac_jit_asked[3] = {false, false, false};
  // forward-only ln L (api_loglike.hip; routes.h: LnlRoute): the route of the last call and the calls per route
  int last_lnl_route = 0;
  long long lnl_route_count[4] = {0, 0, 0, 0};
  // fused_fwd<this stack, precision's ln L traits> instantiated at run time (jit.h: kJitLnl), only for a handle that
  // ASKED (v21_mlp_jit_loglike): routes.h LNL_FUSED_RT
  v21::JitKernel* lnl_jit[3] = {nullptr, nullptr, nullptr};
  bool lnl_jit_asked[3] = {false, false, false};
};
// what a sampler's launch site hands its kernels: the hold record (hold: there is one) and the prior record with the
// held normal columns made uniform -- a held column is no parameter, its prior is never read: FitMapArgs::free_prior's
// rule (fit_kernels.h) applied on the host -- (pri: a free normal column is left)
struct SamplerRecords {
  bool pri, hold;
  PriorArgs pr;
  HoldArgs ho;
};
static inline SamplerRecords sampler_records(const v21_mlp* m) {
  SamplerRecords r{m->has_prior, m->has_hold, m->prior, m->hold};
  if (!r.hold || !r.pri) return r;
  r.pri = false;
  for (int i = 0; i < kFitMaxIn; ++i) {
    if ((r.ho.mask >> i) & 1u) {
      r.pr.kind[i] = 0;
      r.pr.mu[i] = r.pr.w[i] = r.pr.wmu[i] = 0.0;
    }
    if (r.pr.kind[i]) r.pri = true;
  }
  return r;
}
// the layout of this stack's chain streams in `fmt`
static inline ChainLayout chain_layout(const v21_mlp* m, ChainFmt fmt) {
  ChainLayout y;
  y.fmt = fmt;
  const long long frag = fmt == CHAIN_FMT_16 ? 512 : 256;  // elements of one fragment
  long long of = 0, ob = 0;
  for (int l = 0; l < m->L; ++l) {
    const int K = m->dims[l], N = m->nw(l);
    y.fw_off.push_back(of); of += (long long)y.tiles(N) * y.frags(K) * frag;
    y.bw_off.push_back(ob); ob += (long long)y.tiles(K) * y.frags(N) * frag;
  }
  y.fw_bytes = of * y.esize(); y.bw_bytes = ob * y.esize();
  return y;
}
// api_forward.hip: what every route query (v21_route_*) checks first -- its pointers, n_layers in 1 .. 16, widths >= 1,
// precision 0 .. 2 (V21_ERR_ARG)
int route_query_args(bool ptrs, int n_layers, const int* dims, const int* act, int precision);
// api_forward.hip: fused_fwd's packed weight stream of this stack (built on first use)
int mlp_fused_stream(v21_mlp* m, int prec, const unsigned char** stream);
// api_jacobian.hip, shared with api_fit.hip and api_loglike.hip.  The host forms work in chunks of kJacHostChunk rows; the likelihood
// workspace holds kLkSlice rows.
constexpr long long kJacHostChunk = 8192, kLkSlice = 16384;
constexpr long long kNoPitch = LLONG_MAX;  // jac_args: the pitch of rows a call does not have
// what an entry point is checked for beyond its arguments: its in_dim limit, whether it reads the likelihood record,
// and whether it is a fit (input transform required, state checked even for n == 0)
struct JacEntry { const char* name; int max_in; bool like, fit; };
// archs.h holds this stack: it has compiled fused kernels (a row of compiled.h's g_infer: forward, ln L variant, Jacobian)
bool jac_fused_compiled(int L, const int* dims, const int* act);
// the checks of all eight entry points: the pointers they require (ptrs), n >= 0, pitches (ldx, ldy; host rows:
// kNoPitch) and x_dtype, the entry's in_dim limit, then -- from here on only for n > 0, except for a fit -- precision and
// the state the call needs.  Leaves flags with their defined bits only and, for n > 0, the context's device current.
int jac_args(v21_mlp* m, bool ptrs, long long n, long long ldx, long long ldy, int x_dtype, int precision, int& flags, const JacEntry& e);
// the route of one entry-point call (on ldy: a _dev Jacobian's y pitch, else out_dim), counted once -- and decided once:
// every slice, chunk and iteration of the call takes it (a run-time kernel that arrives mid-call serves the next call)
int jac_route(v21_mlp* m, int precision, int flags, long long ldy);
// device rows (float32 / float64, pitch ld) -> m->jxt / jfac, grown to n rows, on the context's stream
int jac_prep(v21_mlp* m, const void* d_src, int dtype, long long ld, long long n, int tin);
// Jacobian mode of `route` on the prepped rows into the likelihood workspace, slice by slice, each slice then reduced
// there by reduce(y, jac, r0, rows) (y: nullptr unless want_y; r0: the slice's first row)
int jac_slices(v21_mlp* m, int route, long long n, bool want_y, int prec, int flags,
               const std::function<int(const float*, const float*, long long, long long)>& reduce);
// the reduction of every consumer (jac_reduce_kernel, reduce_kernels.h; marginalised when the handle has a nuisance
// record, at most kJacMaxIn inputs): F (n, din, din), lnl, grad and the (n, nu_k) sums b -- each nullable, b only with
// a nuisance record -- of the n prepped rows on `route`; row n of the call reads data row (row0 + n) / rpd of pitch
// ld_data (the fit's and the sampler's evaluations are this call too)
int reduce_run(v21_mlp* m, int route, long long n, float* d_F, float* d_lnl, float* d_grad, float* d_b, const float* d_data,
               long long ld_data, long long rpd, long long row0, int prec, int flags);
// api_fit.hip, shared with api_sample.hip: the data a fit or sample call (`what`) of n rows reduces against.  Without a
// data matrix the record's (n_data ignored); else n_data rows (at least one, dividing n: call_data_args, V21_ERR_ARG,
// before the call's options are checked and before any device work), from the host staged in m->fdata, projected when
// a nuisance record is set (call_data, n > 0); row r reads data row r / rpd of pitch ld
struct CallData { const float* d; long long ld, rpd; };
int call_data_args(const char* what, long long n, bool has_data, long long n_data);
int call_data(v21_mlp* m, long long n, const float* data, bool on_host, long long n_data, CallData* out);
// api_nuisance.hip: the record of `k` modes from the host copies of basis, weights and data (no device work; V21_ERR_ARG as
// v21_nuisance_whiten) and its upload (synchronises); the rows of a caller's (n_data, out_dim) data matrix projected
// into m->nu_ws (*out: those, or d_data itself without a nuisance record)
int nuis_build(const double* basis, const float* w, const float* d, int k, int dout, NuisRecord& rec);
int nuis_upload(v21_mlp* m, const NuisRecord& rec);
int nuis_project(v21_mlp* m, const float* d_data, long long n_data, const float** out);
// api_loglike.hip, shared with api_ensemble.hip and api_nested.hip: lnl of the n device rows d_x (pitch ldx; raw, or transformed already with
// V21_FWD_IN_TRANSFORM cleared) that start at row0 of a call of n_call rows, on `route` (routes.h: LnlRoute), on the
// context's stream
int lnl_run(v21_mlp* m, int route, const float* d_x, long long ldx, long long n, long long n_call, const CallData& cd, long long row0,
            float* d_lnl, int prec, int flags);
// whether a call of this handle in `precision` may take LNL_FUSED_RT: the handle asked (v21_mlp_jit_loglike), the code
// object is there (never waited for here) AND loaded on the context's device -- one that cannot be loaded or needs scratch
// memory is marked failed by the load, so this call and every later one decide as a handle that never asked, before
// anything of the call has run.  Asked once per entry-point call, with the context's device current.
bool lnl_rt_ready(v21_mlp* m, int precision);
// api_sample.hip, shared with api_ensemble.hip: the ranges of the counts in the options of entry `what` (V21_ERR_ARG),
// and the states a row stores
int sample_counts(const char* what, int n_steps, int n_warmup, int thin, long long chain0, long long step0);
static inline long long sample_keep(int n_steps, int thin) { return thin > 0 ? n_steps / thin : 0; }
// api_sample.hip, shared with api_ensemble.hip and api_nested.hip: the n rows of entry `what` are whole `noun` (ladders,
// ensembles, runs) of G rows and, with per_data, so are the n / n_data rows of a data row (V21_ERR_ARG)
int whole_groups(const char* what, const char* noun, long long n, int G, bool per_data, long long n_data);
// api_ensemble.hip, shared with api_nested.hip: the samplers on forward-only ln L in groups of G rows (an ensemble's
// walkers, a run's live points).  The body of their route queries behind the query's arguments -- shape: the entry's own
// check of G and n --, the route of one entry-point call, counted once, and the evaluation of a half-move: half_eval
// reserves the n / 2 pending proposals (m->ens_prop: on u) and their ln L (m->ens_lnl) of the n rows at row0 of a call of
// n_call rows, with the call's data in the proposals' compacted layout; run() evaluates them once (lnl_run)
int ens_route_query(const char* what, int n_layers, const int* dims, const int* act, int precision, long long n, long long n_data, int G,
                    int n_modes, int flags, int host_form, int* route, int64_t* chunk_rows, const std::function<int()>& shape, bool rt = false);
EnsRoute ens_route(v21_mlp* m, int precision, long long rpd, long long n, int G, int flags, bool host_form);
struct HalfEval {
  float *prop, *lnl; long long half, n_call, row0; CallData hd; int route, prec, flags;
  int run(v21_mlp* m) const { return lnl_run(m, route, prop, m->dims[0], half, n_call, hd, row0, lnl, prec, flags); }
};
int half_eval(v21_mlp* m, int route, long long n, long long n_call, const CallData& data, long long row0, int prec, int flags, HalfEval* ev);
// A host form stages every chunk of its results in m->stage.  The arrays of the call are listed once: add(host, dev,
// bytes) for an array of `bytes` per unit -- host: the caller's (null: not asked for, no slot), dev: where the chunk's
// device pointer goes (null without a slot), in: an input, copied to the device instead of back.  A unit is `unit` rows
// (1; a nested call's arrays are per run of n_live rows).  A slot of `copies` > 1 is (copies, units, ..) on both sides --
// the chunk's on the device, the call's on the host, hence a pitched copy back -- and one of 0 copies stages nothing.
// From that one list come a chunk's size (reserve), its device pointers with the uploads (place) and the copies back
// (fetch); jac_chunks is the only caller of the three.  A slot starts on 16 bytes: the kernels store dwords, and
// doubles on 8 bytes, so no result depends on it; 16 is what a 4-dword store would need.
struct ChunkStage {
  struct Slot { char* host; void* dev; size_t bytes; long long copies; bool in; };
  std::vector<Slot> slots;
  long long unit = 1;
  long long total = 0;  // units of the whole call (reserve): the pitch of the caller's arrays with copies > 1
  template <class T>
  void add(const T* host, T** dev, size_t bytes, bool in = false, long long copies = 1) {
    *dev = nullptr;
    if (host) slots.push_back({(char*)host, dev, bytes, copies, in});
  }
  static size_t span(const Slot& s, long long units) { return ((size_t)units * s.bytes * (size_t)s.copies + 15) & ~(size_t)15; }
  // m->stage for chunks of up to chunk_rows of the call's n rows, and never less than a chunk's Jacobian y and jac, so
  // that no host form regrows what another left
  int reserve(v21_mlp* m, long long n, long long chunk_rows) {
    total = n / unit;
    size_t mine = 0;
    for (const Slot& s : slots) mine += span(s, chunk_rows / unit);
    return m->stage.reserve(std::max(mine, (size_t)chunk_rows * m->dims[m->L] * (1 + m->dims[0]) * sizeof(float)));
  }
  int place(v21_mlp* m, long long r0, long long rows) const {
    char* p = m->stage.get();
    for (const Slot& s : slots) {
      memcpy(s.dev, &p, sizeof p);
      if (s.in) HIPCHK(hipMemcpyAsync(p, s.host + r0 / unit * s.bytes, (size_t)(rows / unit) * s.bytes, hipMemcpyHostToDevice, m->ctx->stream));
      p += span(s, rows / unit);
    }
    return V21_OK;
  }
  int fetch(v21_mlp* m, long long r0, long long rows) const {
    const char* p = m->stage.get();
    for (const Slot& s : slots) {
      const size_t width = (size_t)(rows / unit) * s.bytes;
      char* dst = s.host + r0 / unit * s.bytes;
      if (!s.in && s.copies == 1) HIPCHK(hipMemcpyAsync(dst, p, width, hipMemcpyDeviceToHost, m->ctx->stream));
      if (!s.in && s.copies > 1)
        HIPCHK(hipMemcpy2DAsync(dst, (size_t)total * s.bytes, p, width, width, (size_t)s.copies, hipMemcpyDeviceToHost, m->ctx->stream));
      p += span(s, rows / unit);
    }
    return V21_OK;
  }
};
// a host form's rows, chunk by chunk: reserve the stage; then per chunk upload (m->hin) and prep its rows (x null: the
// call has none), place, run(r0, rows) on the device pointers that `add` registered, fetch and sync.  chunk_rows: the
// rows of a chunk (whole ladders, ensembles, runs or spectra where the call has them)
int jac_chunks(v21_mlp* m, const void* x, int x_dtype, long long n, int tin, ChunkStage& sg,
               const std::function<int(long long, long long)>& run, long long chunk_rows = kJacHostChunk);
// the results v21_sample_out and v21_ensemble_out share, `keep` states per row, samples and x_last of esz bytes per element
template <class Out>
static void stage_sampler_out(ChunkStage& sg, const Out& host, Out& dev, long long keep, int din, size_t esz) {
  sg.add(host.samples, &dev.samples, keep * din * esz);
  sg.add(host.samples_lnl, &dev.samples_lnl, keep * sizeof(float));
  sg.add(host.x_last, &dev.x_last, din * esz);
  sg.add(host.lnl_last, &dev.lnl_last, sizeof(float));
  sg.add(host.accept_rate, &dev.accept_rate, sizeof(double));
  sg.add(host.mean_u, &dev.mean_u, din * sizeof(double));
  sg.add(host.cov_u, &dev.cov_u, (size_t)din * din * sizeof(double));
  sg.add(host.last_prop_u, &dev.last_prop_u, din * sizeof(float));
  sg.add(host.last_log_alpha, &dev.last_log_alpha, sizeof(double));
}

// ---- trainer (api_trainer.hip)
struct v21_trainer {
  v21_mlp* mlp = nullptr;
  v21_ctx* ctx = nullptr;
  int prec = 0, max_batch = 0;
  v21_adam adam{1e-3f, 0.9f, 0.999f, 1e-7f};
  long long iter = 0;
  size_t P = 0;
  Dev<float> d_g, d_m, d_v;  // P + kArenaPad floats; d_g[P] = loss slot
  // the data sets (0: training, 1: validation), each replaced as a whole by v21_trainer_set_data; n[which] == 0: none.
  // d_y is a view: of d_ybuf, or of d_x where the targets are the inputs (y_is_x)
  Dev<float> d_x[2], d_ybuf[2], d_rw[2];
  float* d_y[2] = {nullptr, nullptr};
  Dev<unsigned short> d_x16; long long ldx16 = 0;  // the training inputs as 16-bit operand elements (fused training kernels: ChainStep::x16)
  long long n[2] = {0, 0};
  bool y_is_x[2] = {false, false};
  Dev<int> d_perm;
  long long Bp = 0;  // row pitch of the transposed buffers (batch padded to 32, + slack)
  std::vector<Dev<float>> d_h, d_ht, d_dz, d_dzt;
  Dev<float> d_wt, d_wp;
  std::vector<long long> wt_off, wp_off;
  bool copies_ok = false;
  bool nt_ok = false;  // the fp32 W^T / padded-W copies of the per-layer path are fresh (chain steps skip them)
  Dev<float> d_yb, d_wb, d_rowloss;
  Dev<float> d_steploss;  // an epoch's per-step losses (ensure_steploss)
  Dev<float> d_evalsum;
  Dev<float> d_slab;  // split-K partial gradients: max_slices x (P + 4)
  int max_slices = 1;
  // variational latent layer (V21_ACT_GAUSS, A13)
  Dev<float> d_zs, d_dzs, d_dzst;  // [z_mean | z_log_var], its gradient, transposed
  Dev<float> d_klrow;
  float kl_weight = 0.f;
  int sample = 1;
  unsigned long long seed = 0;
  // the chain kernels (routes.h: TrainerKind); on the fp32 ones d_fw / d_bw hold fp32 fragments, the gradient operands are d_ht / d_dzt
  Dev<int> d_jobs;  // train_chain32s.h: C32sJob rows
  Dev<unsigned char> d_fw, d_bw;  // the packed streams (+ kChainStreamSlack), allocated once at creation
  ChainLayout lay;                // ... and their layout in this trainer's format
  Dev<float> d_partial;
  Dev<unsigned long long> d_ticket;  // the batch loss as 2^-32 fixed point (16 bytes)
  std::vector<Dev<unsigned short>> d_ht16, d_dzt16;  // fragment-ordered weight-gradient operands (train_chain.h)
  // large steps on a fused training kernel (fused_train.h): its run-time instantiation for a stack outside archs.h
  // (jit.hip; asked for at creation), the kernel's packed stream and the stream's layout
  v21::JitKernel* train_jit = nullptr;
  Dev<unsigned char> d_tstream;
  TrainStream ts;
  bool ts_write = false;        // the Adam pass that ends the current step also rewrites d_tstream (the step took the fused kernel)
  long long n_chain_steps = 0, n_fused_steps = 0, n_stream_packs = 0, n_stream_adam = 0;  // v21_debug_trainer_counters
  // routes.h: what the trainer committed to at creation, the route of its last eager step (written where the kernels are
  // launched) and how many steps took each (v21_trainer_last_route)
  TrainerKind kind;
  StepRoute last_route;
  long long fwd_count[8] = {0, 0, 0, 0, 0, 0, 0, 0}, upd_count[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool tstream_fresh = false;   // d_tstream holds the arena's current weights (cleared by every ensure_copies: any other step, eval, sweep, joint)
  Dev<int> d_dworder;                  // dw_adam.h: tile order per XCD (two-dimensional blocks per layer)
  int dw_xper = 0;
  long long BS = 0;                    // batch steps of 16 per feature tile
  Dev<unsigned long long> d_stamps;
  bool stamps_on = false;  // v21_trainer_enable_stamps: a stamp costs the stamping wave ~600 cycles (s_memtime + its wait), eleven per launch
  // ---- replayed steps (hipGraph).  One optimizer step is captured once per (rows, global rows, data pointers)
  // and replayed; what differs between steps comes from a device table of StepDesc (train_kernels.h) that the
  // host fills for the steps ahead: an epoch's steps in run_epoch, the next kDescRing steps in step_dev.
  int graph_mode = 0;         // 0: off (default, see graph_eligible), 1: asked for (v21_trainer_use_graph)
  bool capturing = false;     // train_on_rows is being recorded, not run
  Dev<StepDesc> d_desc; StepDesc* h_desc = nullptr;  // device table, page-locked staging copy of as many entries
  Dev<int> d_cur;             // index of the next step's descriptor
  long long desc_next = 0, desc_count = 0;  // host mirror of *d_cur, entries valid in the table
  long long desc_iter0 = -1; float desc_lr = -1.f; bool desc_epoch = false;  // what the table was built for
  // r5: HIP-event stamps of an eager step (v21_trainer_phase_timing / v21_trainer_phase_times): two events per step -- its
  // start and ONE cut point (1 after the chain launch, 2 after the last weight-gradient launch, 3 after the exchange has
  // been joined, 4 after Adam) -- for up to phase_cap steps after they were switched on
  bool phase_on = false;
  std::vector<hipEvent_t> phase_ev;
  int phase_steps = 0, phase_cap = 0, phase_seen = 0, phase_cut = 4;
  struct StepGraph { int rows, brows; const void *x, *y, *rw, *idx; long long row0; hipGraph_t graph; hipGraphExec_t exec; };
  std::vector<StepGraph> graphs;
  int graph_misses = 0;
};
constexpr long long kDescRing = 1024;
static inline StepCtx step_ctx(const v21_trainer* t) { return t->capturing ? StepCtx{t->d_desc, t->d_cur} : StepCtx{nullptr, nullptr}; }

// ---- shared between the units
// one grouped launch of the latency-oriented NT GEMM (gemm_nt.h); instantiated per unit and group type
template <class GROUP>
static int launch_nt(int prec, GROUP& grp, hipStream_t st) {
  long long work = 0;  // (routes.h: nt_tile)
  for (int i = 0; i < grp.count; ++i) work += (long long)((grp.p[i].M + 63) / 64) * ((grp.p[i].N + 63) / 64) * std::max(1, grp.p[i].nz);
  const int T = nt_tile(work) / 32;
  int blocks = 0;
  for (int i = 0; i < grp.count; ++i) {
    NtArgs& g = grp.p[i];
    g.tile = 32 * T;
    g.nx = (g.N + g.tile - 1) / g.tile; g.ny = (g.M + g.tile - 1) / g.tile;
    if (g.nz < 1) g.nz = 1;
    if (g.a_scale == 0.f) g.a_scale = 1.f;
    if (g.b_scale == 0.f) g.b_scale = 1.f;
    if (g.out_scale == 0.f) g.out_scale = 1.f;
    if (g.nz == 1) { g.k_chunk = g.K > 0 ? g.K : 1; g.slab_stride = 0; }  // (routes.h: nt_slices)
    grp.first[i] = blocks;
    blocks += g.nx * g.ny * g.nz;
  }
  grp.first[grp.count] = blocks;
  if (blocks <= 0) return V21_OK;
  bool smooth = false;  // a problem with an epilogue of act.h: the kernel's ACT instantiation (gemm_nt.h)
  for (int i = 0; i < grp.count; ++i) smooth = smooth || grp.p[i].ep == NT_FWD_ACT || grp.p[i].ep == NT_DX_ACT;
#define V21_NT(PT) \
  do { if (smooth && T == 2) hipLaunchKernelGGL((gemm_nt_kernel<PT, 2, GROUP, true>), dim3(blocks), dim3(256), 0, st, grp); \
       else if (smooth) hipLaunchKernelGGL((gemm_nt_kernel<PT, 1, GROUP, true>), dim3(blocks), dim3(256), 0, st, grp); \
       else if (T == 2) hipLaunchKernelGGL((gemm_nt_kernel<PT, 2, GROUP>), dim3(blocks), dim3(256), 0, st, grp); \
       else hipLaunchKernelGGL((gemm_nt_kernel<PT, 1, GROUP>), dim3(blocks), dim3(256), 0, st, grp); } while (0)
  switch (prec) {
    case V21_PREC_F32: V21_NT(PrecF32); break;
    case V21_PREC_F16: V21_NT(PrecF16); break;
    default: V21_NT(PrecBF16); break;
  }
#undef V21_NT
  HIPCHK(hipGetLastError());
  return V21_OK;
}
// one of the four <A, GAUSS> instantiations of a chain kernel family (A0 / A1: the two precisions, or 4 / 8 rows per workgroup)
#define V21_CHAIN_LAUNCH(KERN, A0, A1, first, gauss, lds, grid, block, st, ...)                           \
  do {                                                                                                     \
    if ((first) && (gauss)) hipLaunchKernelGGL((KERN<A0, true>), grid, block, lds, st, __VA_ARGS__);      \
    else if (first) hipLaunchKernelGGL((KERN<A0, false>), grid, block, lds, st, __VA_ARGS__);             \
    else if (gauss) hipLaunchKernelGGL((KERN<A1, true>), grid, block, lds, st, __VA_ARGS__);              \
    else hipLaunchKernelGGL((KERN<A1, false>), grid, block, lds, st, __VA_ARGS__);                        \
  } while (0)
float adam_alpha(const v21_adam& a, long long t);  // api_trainer.hip
// Where a step's batch loss goes.  `slot` >= 0: entry `slot` of the epoch's loss table (v21_trainer::d_steploss), written by
// the kernel that publishes the loss -- a device-to-device copy per step would be a launch of its own.  Otherwise the step
// ends by copying the arena's loss slot (d_g[P]) to `out`, if there is one.
struct StepLoss { float* out; int slot; };
AdamArgs adam_args(v21_trainer* t, bool do_adam, float alpha, bool skip_nt = false, const StepLoss* pub = nullptr);  // api_trainer.hip
int chain_attr(int prec);  // api_trainer.hip
ChainModel chain_model(v21_trainer* t);  // api_trainer.hip
ChainModel chain_model32(v21_trainer* t);  // api_trainer.hip
ChainStep chain_step(const float* x, long long ldx, const float* y, long long ldy, const float* rw, const int* d_idx, long long first, int rows, int brows, int dout, const v21_trainer* vae = nullptr, long long row0 = 0);  // api_trainer.hip
void destroy_graphs(v21_trainer* t);  // api_trainer.hip
void dw16_problems(v21_trainer* t, int rows, int brows, int* nslice_out, std::vector<Dw16Args>& probs);  // api_trainer.hip
int ensure_copies(v21_trainer* t, bool need_nt = true);  // api_trainer.hip
int gather_batch(v21_trainer* t, const float* x, long long ldx, const float* y, long long ldy_src, const float* rw, const int* d_idx, long long first, int rows);  // api_trainer.hip
float grad_opscale(int brows, int dout);  // api_trainer.hip
void invalidate_streams(v21_mlp* m);  // api_forward.hip
int launch_chain32_args(ChainArgs& a, hipStream_t st, bool small, const RouteEnv& e);  // api_trainer.hip: train_chain32[s]_kernel over a.rows rows, one model
int launch_dw16(int prec, const std::vector<Dw16Args>& probs, hipStream_t st, const DwXRows* xr = nullptr);  // api_trainer.hip
int launch_dw32_group(const std::vector<v21_trainer*>& trs, const Dw32Model* d_tab, int rows, long long step_index, int max_blocks, hipStream_t st, bool small_slabs = false);  // api_sweep.hip
int launch_dw_adam_group(const std::vector<v21_trainer*>& tr, const DwAdamModel* d_tab, const std::vector<DwAdamModel>& h_tab, int rows, int brows, long long slot, hipStream_t st);  // api_trainer.hip
void launch_joint32_kernel(int rpw, bool gauss, dim3 grid, dim3 block, hipStream_t st, const ChainModel* tab, const ChainStep& sa, const ChainStep& sb);  // api_trainer.hip
void launch_joint_kernel(int prec, bool gauss, dim3 grid, dim3 block, hipStream_t st, const ChainModel* tab, const ChainStep& sa, const ChainStep& sb);  // api_trainer.hip
// exchange (unless `exchanged`), Adam, packed copies; `pub`: this Adam pass publishes the loss (api_trainer.hip)
int reduce_and_update(v21_trainer* t, int fold, bool exchanged = false, const StepLoss* pub = nullptr);
void weights_updated(v21_trainer* t, bool nt_ok);  // api_trainer.hip: every copy but the updater's own is stale
int step_tail(v21_trainer* t, const StepLoss& loss);  // api_trainer.hip: the loss copied out (slot < 0), weights_updated
int chain32_update(v21_trainer* t, int rows, float* loss_out);  // api_trainer.hip: the update of an f32 step whose chain ran
// api_base.hip: the all-reduce of d_buf[0, n) on a stream of the caller's choice (RCCL: enqueued there; host-staged
// transport: blocking, staged through that stream; null transport / one rank: nothing)
int comm_allreduce_on(v21_ctx* c, float* d_buf, size_t n, hipStream_t st);
int refresh_dw32_table(const std::vector<v21_trainer*>& trs, Dw32Model* d_tab, std::vector<Dw32Model>& h_tab, int* max_blocks, bool* ok, hipStream_t st);  // api_sweep.hip
int refresh_dw_adam_table(const std::vector<v21_trainer*>& tr, Dev<DwAdamModel>& d_tab, std::vector<DwAdamModel>& h_tab, hipStream_t st);  // api_trainer.hip
int launch_nt_many(int prec, std::vector<NtArgs>& probs, hipStream_t st);  // api_trainer.hip
void launch_chain_forward_mode(int prec, dim3 grid, dim3 block, hipStream_t st, const ChainArgs& a);  // api_trainer.hip

// ---- pieces of a step shared by the trainer, the sweep and the joint step (api_trainer.hip)
int zero_grad(v21_trainer* t);                 // arena + loss slot = 0: a rank without rows in this step
int reduce_slabs(v21_trainer* t, int nslice);  // the nslice split-K slabs summed into the arena
// layer l's NT problems: forward (A: its input rows), [dW; db] = [H^T; 1^T] dZ over the slices `sl`, dH = dZ W^T masked
NtArgs nt_forward(const v21_trainer* t, int l, const float* A, int rows, bool want_t);
NtArgs nt_dw(const v21_trainer* t, int l, const float* A, const float* B, int rows, NtSlices sl, float gs);
NtArgs nt_dx(const v21_trainer* t, int l, const float* A, int rows, float gs);
// every layer's f32 gradient + Adam in one launch (dw_adam32.h), less what changes per step (K, alpha, replay, slot: -1);
// returns the launch's workgroups
int dw32_model(const v21_trainer* t, int tile, Dw32Model& md);

// a device table built on the host, uploaded only when it changed (after the stream drained: a step in flight may read it)
template <class T>
static int upload_if_changed(const std::vector<T>& tab, std::vector<T>& host, T* dev, hipStream_t st) {
  if (tab.size() == host.size() && memcmp(tab.data(), host.data(), tab.size() * sizeof(T)) == 0) return V21_OK;
  HIPCHK(hipStreamSynchronize(st));
  host = tab;
  HIPCHK(hipMemcpyAsync(dev, host.data(), tab.size() * sizeof(T), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  return V21_OK;
}

// ---- epochs (api_trainer.hip): the row table checked and uploaded (*d_idx: nullptr without one); the loss table grown
int upload_rows(v21_trainer* t, const int32_t* perm, const int** d_idx);
int ensure_steploss(v21_trainer* t, long long cap);
struct EpochBatch { long long first, lo; int brows, rows; };  // global batch [first, first + brows), this rank's [lo, lo + rows)
static inline EpochBatch epoch_batch(const v21_ctx* c, long long n, int batch, long long s) {
  EpochBatch b;
  b.first = s * batch;
  b.brows = (int)std::min<long long>(batch, n - b.first);
  b.lo = b.first + (long long)b.brows * c->rank / c->nranks;
  b.rows = (int)(b.first + (long long)b.brows * (c->rank + 1) / c->nranks - b.lo);
  return b;
}
// loss[k]: trainer k's per-step losses summed over n rows (Keras' epoch loss) / its fixed-point validation sum, cleared
int epoch_losses(const std::vector<v21_trainer*>& trs, long long steps, long long n, double* loss);
int read_tickets(const std::vector<v21_trainer*>& trs, long long n, double* loss);
