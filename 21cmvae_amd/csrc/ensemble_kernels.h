// ensemble_kernels.h -- the affine-invariant ensemble sampler on the device (api_ensemble.hip; include/v21.h:
// v21_mlp_sample_ensemble): Goodman & Weare's stretch move on forward-only ln L, in the transformed coordinates
// u in [-1, 1]^din of the fit under the handle's prior on that box (rowmath.h: PriorArgs; uniform without a record;
// with one, PRIOR, the acceptance gains ln p(y) - ln p(x) and nothing else changes).  W consecutive rows form one
// ensemble of two sets of H = W / 2 walkers; a sweep is two half-moves, and half-move h moves every walker of set h
// along the line to a partner drawn from the current positions of set 1 - h.
//   ensemble_step_kernel    one launch per half-move, after the evaluation of the pending proposals: it DECIDES them
//                           (accepts or rejects, keeps the sweep: Moments of rowmath.h), meets a barrier, then DRAWS the
//                           other set's proposals from the positions just decided;
//   ensemble_finish_kernel  the last state back to raw parameters and the per-row results.
// The proposals of one half-move lie compacted in a buffer of n / 2 rows (row e H + j: walker j of the moving set of
// ensemble e): every ln L of a call, the starts' included, is evaluated in that layout on one route.
// Launch k = 0 .. 2 T + 2 of a call of T sweeps decides set (k - 1) % 2 (k >= 1) and draws for set k % 2 (k <= 2 T + 1):
//   k = 0, 1  draw: the clamped start of the set, a "proposal" that k + 1 accepts whatever its ln L;
//   k >= 2    draw: the stretch proposal of sweep (k - 2) / 2;    k >= 3  decide: that of sweep (k - 3) / 2.
// A 256-thread workgroup takes floor(256 / H) whole ensembles: thread (slot, j) decides walker j of one set and then
// draws for walker j of the other, whose partner was decided by a thread of the same workgroup.  The partner's position
// is read from global memory after the barrier, as the tempered sampler's swap does (sample_kernels.h): writer and reader
// share a CU and its L1, the barrier's workgroup-scope release / acquire orders them.  No thread returns before the
// barrier; threads past the workgroup's ensembles or past n skip the work on both sides of it.
// Acceptance of walker x's proposal y = x_k + z (x - x_k), iff log(uniform) < log alpha:
//   log alpha = (din - 1) ln z + ln L(y) - ln L(x)   [PRIOR: + ln p(y) - ln p(x)]
// No LDS, no atomics; float64 in registers.  Random numbers: Philox4x32-10 of sample_kernels.h, block 0 at step = the
// sweep: w0 the stretch, w1 the partner, w2 the acceptance uniform.  The prior draws nothing.
// With a hold record (HOLD; rowmath.h: HoldArgs) the start launches (k < 2) write the held float32 over the start's and
// the stretch's Jacobian counts the free columns, lz = (d_free - 1) ln z.  The stretch itself needs no change: every
// walker of an ensemble carries the same float32 x in a held column, xi - xp is exactly 0 there, and x + z 0 rounds
// to x, so a proposal, and with it every state and stored sample, returns the held value bit for bit.  The launch site
// hands over the prior record with the held normal columns made uniform; the finish kernel writes the held column's
// mean_u as the value and its cov_u row and column as exact zeros (hold_finish).
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include "rowmath.h"
#include "sample_kernels.h"

namespace v21 {

// per-walker state
struct EnsRow {
  float u[kFitMaxIn];    // current position
  float lnl;             // ln L there
  int reject;            // the pending proposal left the box: rejected unread
  int partner;           // of the pending / last proposal: row index within the ensemble (-1: none yet)
  int pad_;
  double lz;             // (din - 1) ln z of the pending proposal
  double log_alpha;      // of the last half-move decided
  Moments m;             // of the kept sweeps
};
static_assert(offsetof(EnsRow, m) + sizeof(Moments) == sizeof(EnsRow), "the moments are the tail of the row state");

// what one call's step launches share
struct EnsArgs {
  long long n;
  int din, W, H, epw;          // walkers per ensemble, per set, ensembles per workgroup
  long long total, n_warmup;   // sweeps of the call (warm-up + kept), of them warm-up
  long long thin, n_keep;      // every thin-th kept sweep is stored (0: none), n_keep = n_steps / thin of them
  double a;                    // stretch scale
  uint64_t seed, chain0, step0;
  void* samples;               // (n, n_keep, din) raw units, nullable
  float* samples_lnl;          // (n, n_keep), nullable
  float* last_prop_u;          // (n, din), nullable: written by a walker's last decision
  v21_affine_in t;
};

// one thread per (ensemble, j): launch k of the call (above).  start: the transformed start rows (n, din), read by
// k = 0, 1; prop: the compacted proposals (n / 2, din); lnl_new: their evaluation (n / 2).  XT: the samples' type;
// PRIOR: the handle holds a prior record, pr (else not read).  HOLD: it holds a hold record; Hold: HoldArgs for HOLD =
// true, no argument for HOLD = false.
template <class XT, bool PRIOR, bool HOLD, class... Hold>
__global__ void __launch_bounds__(256) ensemble_step_kernel(EnsRow* st, const float* __restrict__ start, float* __restrict__ prop,
                                                            const float* __restrict__ lnl_new, long long k, const EnsArgs a,
                                                            const PriorArgs pr, const Hold... hold) {
  static_assert(sizeof...(Hold) == (HOLD ? 1 : 0), "HOLD takes one HoldArgs, its absence nothing");
  [[maybe_unused]] const auto& ho = hold_of(hold...);
  constexpr int NI = kFitMaxIn;
  const int din = a.din, H = a.H, W = a.W;
  const int slot = (int)threadIdx.x / H, j = (int)threadIdx.x % H;
  const long long e = (long long)blockIdx.x * a.epw + slot;
  // (no thread returns before the barrier: one that is not `active` skips the work on both sides of it)
  const bool active = slot < a.epw && e * W < a.n;
  const long long p = e * H + j;
  const long long last = 2 * a.total + 2;
  if (active && k >= 1) {
    // ---- decide the pending proposal of walker j of set hd
    const int hd = (int)((k - 1) & 1);
    const long long row = e * W + (long long)hd * H + j;
    EnsRow& s = st[row];
    const float* y = prop + p * din;
    const float lnl_y = lnl_new[p];
    bool accept = true;  // (k = 1, 2: the start, whatever its ln L)
    const long long sweep = (k - 3) / 2;
    if (k >= 3) {
      double log_alpha = -INFINITY;
      accept = false;
      if (!s.reject) {
        log_alpha = s.lz + ((double)lnl_y - (double)s.lnl);
        if constexpr (PRIOR) log_alpha += prior_logp(pr, y, din) - prior_logp(pr, s.u, din);
        if (log_alpha != log_alpha) log_alpha = -INFINITY;
        uint32_t w[4];
        sample_block(a.seed, a.chain0 + (uint64_t)row, (uint32_t)(a.step0 + (uint64_t)sweep), 0u, w);
        accept = log(sample_uniform(w[2])) < log_alpha;
      }
      s.log_alpha = log_alpha;
    }
    if (accept) {
#pragma unroll
      for (int i = 0; i < NI; ++i)
        if (i < din) s.u[i] = y[i];
      s.lnl = lnl_y;
    }
    if (k >= 3 && sweep >= a.n_warmup) {
      // a kept sweep: moments, and every thin-th state in raw units
      double u[NI];
      widen_row(s.u, din, u);
      s.m.add(u, din, accept);
      Moments::store<XT>(row, sweep - a.n_warmup + 1, a.thin, a.n_keep, a.samples, a.samples_lnl, u, din, s.lnl, a.t);
    }
    if (k + 2 > last && a.last_prop_u)  // (the walker's last decision of the call)
      for (int i = 0; i < din; ++i) a.last_prop_u[row * din + i] = y[i];
  }
  __syncthreads();  // (the positions the decisions above took are in place for this workgroup's readers)
  if (active && k < last) {
    // ---- draw for walker j of set hw
    const int hw = (int)(k & 1);
    const long long row = e * W + (long long)hw * H + j;
    EnsRow& s = st[row];
    float* y = prop + p * din;
    if (k < 2) {
      // the start into the box, the state reset
      const float* x0 = start + row * din;
      for (int i = 0; i < din; ++i) y[i] = box_clamp1(x0[i]);
      hold_row<HOLD>(ho, din, y);
      s.lnl = 0.f;
      s.reject = 0;
      s.partner = -1;
      s.lz = 0.0;
      s.log_alpha = 0.0;
      s.m.clear();
    } else {
      const long long sweep = (k - 2) / 2;
      uint32_t w[4];
      sample_block(a.seed, a.chain0 + (uint64_t)row, (uint32_t)(a.step0 + (uint64_t)sweep), 0u, w);
      const double r = (a.a - 1.0) * sample_uniform(w[0]) + 1.0;
      const double z = r * r / a.a;
      const int kp = (int)(((uint64_t)(uint32_t)H * (uint64_t)w[1]) >> 32);
      const int prow = (1 - hw) * H + kp;
      const float* xk = st[e * W + prow].u;
      bool inside = true, finite = true;
      float yf[NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const double xi = i < din ? (double)s.u[i] : 0.0, xp = i < din ? (double)xk[i] : 0.0;
        yf[i] = (float)(xp + z * (xi - xp));
        if (i < din && !(yf[i] >= -1.f && yf[i] <= 1.f)) inside = false;
        if (i < din && !(fabsf(yf[i]) < 3.0e38f)) finite = false;
      }
      s.reject = inside ? 0 : 1;
      s.partner = prow;
      s.lz = (double)(hold_free<HOLD>(ho, din) - 1) * log(z);
#pragma unroll
      for (int i = 0; i < NI; ++i)
        if (i < din) y[i] = finite ? yf[i] : s.u[i];
    }
  }
}

// one thread per row: the last state in raw units (raw_row) and the per-row results (nullable; the moments' over `kept`
// sweeps: Moments::finish)
struct EnsOutDev {
  void* x_last;
  float* lnl_last;
  double *accept_rate, *mean_u, *cov_u, *last_log_alpha;
  int* last_partner;
};
template <class XT, bool HOLD, class... Hold>
__global__ void __launch_bounds__(256) ensemble_finish_kernel(const EnsRow* __restrict__ st, long long n, int din, long long kept,
                                                              const v21_affine_in t, const EnsOutDev o, const Hold... hold) {
  static_assert(sizeof...(Hold) == (HOLD ? 1 : 0), "HOLD takes one HoldArgs, its absence nothing");
  [[maybe_unused]] const auto& ho = hold_of(hold...);
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const EnsRow& s = st[row];
  raw_row<XT>(o.x_last, row, din, s.u, t);
  if (o.lnl_last) o.lnl_last[row] = s.lnl;
  s.m.finish(row, din, kept, s.u, o.mean_u, o.cov_u, o.accept_rate);
  hold_finish<HOLD>(ho, row, din, o.mean_u, o.cov_u);
  if (o.last_log_alpha) o.last_log_alpha[row] = s.log_alpha;
  if (o.last_partner) o.last_partner[row] = s.partner;
}

}  // namespace v21
