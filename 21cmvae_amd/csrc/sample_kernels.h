// sample_kernels.h -- posterior sampling on the device (api_sample.hip): a batched Metropolis-adjusted Langevin sampler
// whose metric is the Fisher matrix at the current point ("simplified manifold MALA"), one thread per chain, in the
// transformed coordinates u in [-1, 1]^din of the fit (fit_kernels.h) under the handle's prior on that box: uniform, or
// with a prior record (include/v21.h: v21_mlp_set_prior; rowmath.h: PriorArgs) separable with truncated-normal columns.
//   sample_init_kernel    clamps the transformed start rows into the box and resets the chain state;
//   sample_step_kernel    consumes the evaluation (ln L, gradient, Fisher matrix: jac_reduce_kernel) of the pending
//                         proposal: accepts or rejects it, adapts the step size in warm-up, keeps the transition
//                         (rowmath.h: Moments), then draws and writes the next proposal;
//   sample_finish_kernel  the last state back to raw parameters and the results;
//   sample_step_tempered_kernel / sample_finish_tempered_kernel  the same chains as the rungs of parallel-tempered ladders
//                         (below, "parallel tempering"): the step kernel's three parts with ln L, g and F scaled by the
//                         row's inverse temperature, and between them the swap event among the threads of a workgroup.
// The transition, with G(u) = F(u) + ridge I = L L^T, d = din and step size e:
//   mu(u) = u + e^2 / 2 G(u)^-1 g(u);   u' = float32(mu(u) + e L(u)^-T xi),  xi ~ N(0, I_d)
//   log q(b | a) = -|L(a)^T (b - mu(a))|^2 / (2 e^2) + sum_i log L_ii(a) - d / 2 log(2 pi e^2)
//   log alpha = lnL(u') - lnL(u) + log q(u | u') - log q(u' | u);   accept iff log(uniform) < log alpha
// With a prior record (PRIOR) the target is L p, ln p(u) = -1/2 sum_i ((u_i - mu_i) / sd_i)^2 over the normal columns:
//   g(u) = grad ln L(u) - (u - mu) / sd^2,  F(u) = Fisher(u) + diag(1 / sd^2),  log alpha += ln p(u') - ln p(u),
// the additions made after a tempered rung's beta has scaled ln L's terms and not scaled themselves (a rung samples
// L^beta p, the beta = 0 rung the prior).  The state and every stored ln L stay ln L alone.
// (the metric's derivative term of full manifold MALA is left out; the acceptance uses the q that was really drawn
// from, at the float32 u' that is really evaluated, so the chain is exact).  A proposal with a coordinate outside
// [-1, 1], or whose G has no finite Cholesky factor, is rejected: log alpha = -inf, its evaluation is not read.
// Cholesky, solves (rowmath.h) and log-densities are float64 in registers.  Random numbers: Philox4x32-10, include/v21.h:
//   blocks 0 and 1, step = the transition: the proposal's normals;  block 2, same step: the acceptance uniform (w0);
//   block 3, step = the transition a swap event follows: the swap's uniform (w0), drawn for the pair's lower row.
// The prior draws nothing.
// With a hold record (HOLD; include/v21.h: v21_mlp_set_hold; rowmath.h: HoldArgs) a held column i is no parameter: the
// init kernel writes its float32 over the start's, at every point g_i = 0, F_ij = F_ji = 0, F_ii = 1 after the prior's
// additions (hold_eval), the ridge goes to the FREE pivots only -- so a held pivot is exactly 1, its row and column of L
// exactly 0, its log 0 and its drift component 0 --, its normal is 0 (drawn from the same Philox words and dropped: a
// free column's draw does not depend on what is held), u'_i is the stored float32 bit for bit, and log q is normalised
// over the d_free free columns: the transition is that of the d_free-dimensional sampler on the free block.  The launch
// site hands over the prior record with the held normal columns made uniform.  The swap, TemperArgs and Moments are untouched.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include "rowmath.h"

namespace v21 {

// ---- Philox4x32-10 (Salmon et al. 2011): counter c[4], key (k0, k1) -> four words in c
__host__ __device__ inline void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1;
    c[3] = (uint32_t)p0;
    c[0] = n0;
    c[2] = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}
// the draws of transition `step` of chain `chain` (both global: chain0 + row, step0 + step), include/v21.h:
// counter (chain low word, chain high word, step, block), key (seed low word, seed high word)
__host__ __device__ inline void sample_block(uint64_t seed, uint64_t chain, uint32_t step, uint32_t block, uint32_t w[4]) {
  w[0] = (uint32_t)chain; w[1] = (uint32_t)(chain >> 32); w[2] = step; w[3] = block;
  philox4x32_10(w, (uint32_t)seed, (uint32_t)(seed >> 32));
}
__host__ __device__ inline double sample_uniform(uint32_t w) { return ((double)w + 0.5) * (1.0 / 4294967296.0); }

constexpr double kSampleTwoPi = 6.283185307179586476925286766559;

// per-chain state
struct SampleRow {
  EvalPoint p;                   // current point
  int reject;                    // the pending proposal left the box (or could not be drawn): rejected unread
  double eps;                    // step size
  double lq_fwd;                 // log q(pending proposal | current point)
  double log_alpha;              // of the last transition decided
  Moments m;                     // of the kept transitions
};
static_assert(offsetof(SampleRow, m) + sizeof(Moments) == sizeof(SampleRow), "the moments are the tail of the row state");

// what one sample call's step launches share
struct SampleArgs {
  long long n;
  int din;
  long long total, n_warmup;     // transitions of the call (warm-up + kept), of them warm-up
  long long thin, n_keep;        // every thin-th kept transition is stored (0: none), n_keep = n_steps / thin of them
  double ridge, target;
  uint64_t seed, chain0, step0;
  void* samples;                 // (n, n_keep, din) raw units, nullable
  float* samples_lnl;            // (n, n_keep), nullable
  v21_affine_in t;
};

// Cholesky factor of G = F + ridge I (rowmath.h); false: a pivot is not positive and finite
// HOLD: a held pivot gets no ridge
template <bool HOLD = false, class H = NoHold>
__device__ inline bool sample_chol(const double* F, double ridge, int din, double* Lm, const H& ho = {}) {
  if constexpr (HOLD)
    return chol_factor(F, din, Lm, [&](int i) { return ho.held(i) ? 0.0 : ridge; }, [](double pivot) { return pivot > 0.0 && pivot < 1.79e308; });
  else
    return chol_factor(F, din, Lm, [&](int) { return ridge; }, [](double pivot) { return pivot > 0.0 && pivot < 1.79e308; });
}
// mu = u + e^2 / 2 G^-1 g (two triangular solves) and sum_i log L_ii
__device__ inline double sample_drift(const double* Lm, const double* u, const double* g, double eps, int din, double* mu) {
  constexpr int NI = kFitMaxIn;
  double z[NI], ld = 0.0;
  solve_lower(Lm, g, z);
  solve_upper(Lm, z, mu);
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    if (i < din) ld += log(Lm[i * (i + 1) / 2 + i]);
    mu[i] = u[i] + 0.5 * eps * eps * mu[i];
  }
  return ld;
}
// log q(b | a) from a's factor, drift and log-determinant term; dn: the dimension of its normalisation (din; d_free
// with a hold record, whose held columns add exact zeros everywhere else)
__device__ inline double sample_logq(const double* Lm, const double* mu, double ld, const double* b, double eps, int din, int dn) {
  constexpr int NI = kFitMaxIn;
  double q = 0.0;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    double v = 0.0;  // (L^T (b - mu))_i = sum_{k >= i} L[k][i] (b - mu)_k
#pragma unroll
    for (int k = i; k < NI; ++k) v += Lm[k * (k + 1) / 2 + i] * (b[k] - mu[k]);
    if (i < din) q += v * v;
  }
  return -q / (2.0 * eps * eps) + ld - 0.5 * dn * log(kSampleTwoPi * eps * eps);
}

// one thread per chain: u_prop (pitch din, the rows the next evaluation reads) into the box (box_clamp), the state reset;
// the step size from eps_start (nullable: eps0).  HOLD: the held coordinates over the start's; Hold: HoldArgs for HOLD =
// true, no argument for HOLD = false
template <bool HOLD, class... Hold>
__global__ void __launch_bounds__(256) sample_init_kernel(SampleRow* __restrict__ st, float* __restrict__ up, float* __restrict__ fac,
                                                          long long n, int din, double eps0, const double* __restrict__ eps_start,
                                                          const Hold... hold) {
  static_assert(sizeof...(Hold) == (HOLD ? 1 : 0), "HOLD takes one HoldArgs, its absence nothing");
  [[maybe_unused]] const auto& ho = hold_of(hold...);
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  box_clamp(up + row * din, fac + row * din, din);
  hold_row<HOLD>(ho, din, up + row * din);
  SampleRow& s = st[row];
  double e = eps_start ? eps_start[row] : eps0;
  s.eps = e > 0.0 && e < 1.79e308 ? e : eps0;
  s.p.lnl = 0.f;
  s.reject = 0;
  s.lq_fwd = 0.0;
  s.log_alpha = 0.0;
  s.m.clear();
}

// ---- the three parts of a step, shared by sample_step_kernel and sample_step_tempered_kernel.  TEMPER: ln L, g and F
// enter the drift, the metric and log alpha multiplied by the row's inverse temperature beta (include/v21.h); without
// it beta is not read and the arithmetic is the untempered one, operation for operation.
// beta v, exactly 0 at beta = 0 whatever v holds
__device__ __forceinline__ double temper_mul(double beta, double v) { return beta == 0.0 ? 0.0 : beta * v; }
template <bool TEMPER>
__device__ __forceinline__ void temper_eval(double beta, double* g, double* F) {
  if constexpr (TEMPER) {
#pragma unroll
    for (int i = 0; i < kFitMaxIn; ++i) g[i] = temper_mul(beta, g[i]);
#pragma unroll
    for (int p = 0; p < kFitPacked; ++p) F[p] = temper_mul(beta, F[p]);
  }
}

// the decision of the pending proposal after evaluation number `it` of the call (lnl_new, gn, Fn: the row's, at upr):
// it == 0 is the start's, accepted whatever its value; it >= 1 is the proposal's of transition it - 1.  Adapts the
// step size in warm-up and takes an accepted proposal as the current point.  -> accepted; have_factor: Lm, mu and ld
// belong to the current point at the current step size
template <bool TEMPER, bool PRIOR, bool HOLD, class H>
__device__ __forceinline__ bool sample_decide(SampleRow& s, const float* upr, const float* lnl_new, const float* gn, const float* Fn,
                                              long long it, long long row, const SampleArgs& a, double beta, const PriorArgs& pr,
                                              const H& ho, double& eps, double* Lm, double* mu, double& ld, bool& have_factor) {
  constexpr int NI = kFitMaxIn, NP = kFitPacked;
  const int din = a.din;
  double F[NP], g[NI], u[NI];
  bool accept = it == 0;
  if (it > 0) {
    // the proposal's side of the acceptance ratio
    double log_alpha = -INFINITY;
    if (!s.reject) {
      double up64[NI];
      widen_row(upr, din, up64);
      widen_eval(gn, Fn, din, g, F);
      temper_eval<TEMPER>(beta, g, F);
      prior_eval<PRIOR>(pr, up64, din, g, F);
      hold_eval<HOLD>(ho, din, g, F);
      s.p.widen_u(din, u);
      if (sample_chol<HOLD>(F, a.ridge, din, Lm, ho)) {
        ld = sample_drift(Lm, up64, g, eps, din, mu);
        const double lq_rev = sample_logq(Lm, mu, ld, u, eps, din, hold_free<HOLD>(ho, din));
        if constexpr (TEMPER)
          log_alpha = temper_mul(beta, (double)*lnl_new - (double)s.p.lnl) + lq_rev - s.lq_fwd;
        else
          log_alpha = (double)*lnl_new - (double)s.p.lnl + lq_rev - s.lq_fwd;
        if constexpr (PRIOR) log_alpha += prior_logp(pr, up64, din) - prior_logp(pr, u, din);
        if (log_alpha != log_alpha) log_alpha = -INFINITY;
        uint32_t w[4];
        sample_block(a.seed, a.chain0 + (uint64_t)row, (uint32_t)(a.step0 + (uint64_t)(it - 1)), 2u, w);
        accept = log(sample_uniform(w[0])) < log_alpha;
        have_factor = accept;
      }
    }
    s.log_alpha = log_alpha;
    if (it <= a.n_warmup) {
      // Robbins-Monro on log eps, transition t = it (1-based) of the warm-up
      const double al = log_alpha >= 0.0 ? 1.0 : exp(log_alpha);
      eps *= exp(pow((double)it, -0.6) * (al - a.target));
      s.eps = eps;
      if (accept) have_factor = false;  // (the drift of the next proposal takes the new step size: rebuilt below)
    }
  }
  if (accept) s.p.take(upr, *lnl_new, gn, Fn, din);
  return accept;
}

// a kept transition (it > n_warmup) at the current point u: moments, and every thin-th state in raw units.  T: the
// samples' type.
template <class T>
__device__ __forceinline__ void sample_keep(SampleRow& s, const double* u, bool accept, long long it, long long row, const SampleArgs& a) {
  if (it > a.n_warmup) {
    s.m.add(u, a.din, accept);
    Moments::store<T>(row, it - a.n_warmup, a.thin, a.n_keep, a.samples, a.samples_lnl, u, a.din, s.p.lnl, a.t);
  }
}

// the proposal of transition `it` from the current point u, written to upr
template <bool TEMPER, bool PRIOR, bool HOLD, class H>
__device__ __forceinline__ void sample_draw(SampleRow& s, float* upr, const double* u, long long it, long long row, const SampleArgs& a,
                                            double beta, const PriorArgs& pr, const H& ho, double eps, double* Lm, double* mu, double ld,
                                            bool have_factor) {
  constexpr int NI = kFitMaxIn, NP = kFitPacked;
  const int din = a.din;
  if (!have_factor) {
    double F[NP], g[NI];
    s.p.widen(din, g, F);
    temper_eval<TEMPER>(beta, g, F);
    prior_eval<PRIOR>(pr, u, din, g, F);
    hold_eval<HOLD>(ho, din, g, F);
    if (!sample_chol<HOLD>(F, a.ridge, din, Lm, ho)) {
      // (only a start whose evaluation is not finite: the chain stays where it is)
      s.reject = 1;
      s.lq_fwd = 0.0;
#pragma unroll
      for (int i = 0; i < NI; ++i)
        if (i < din) upr[i] = s.p.u[i];
      return;
    }
    ld = sample_drift(Lm, u, g, eps, din, mu);
  }
  double xi[NI] = {};
  const uint64_t chain = a.chain0 + (uint64_t)row;
  const uint32_t step = (uint32_t)(a.step0 + (uint64_t)it);
#pragma unroll
  for (int b = 0; b < NI / 4; ++b) {
    if (4 * b < din) {
      uint32_t w[4];
      sample_block(a.seed, chain, step, (uint32_t)b, w);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const double r = sqrt(-2.0 * log(sample_uniform(w[2 * h]))), th = kSampleTwoPi * sample_uniform(w[2 * h + 1]);
        xi[4 * b + 2 * h] = r * cos(th);
        xi[4 * b + 2 * h + 1] = r * sin(th);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NI; ++i)
    if (i >= din) xi[i] = 0.0;  // (the rest of the last block's draws)
  if constexpr (HOLD) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
      if (ho.held(i)) xi[i] = 0.0;  // (a held column's normal: drawn and dropped)
  }
  // u' = mu + eps L^-T xi, rounded to the float32 that is evaluated
  double v[NI], ub[NI];
  bool inside = true;
  solve_upper(Lm, xi, v);
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    float f = (float)(mu[i] + eps * v[i]);
    // (a held mu_i is u_i and its v_i exactly 0, so f is the stored float32 already unless a free column's NaN reached it)
    if constexpr (HOLD)
      if (i < din && ho.held(i)) f = ho.u[i];
    ub[i] = i < din ? (double)f : 0.0;
    if (i < din && !(f >= -1.f && f <= 1.f)) inside = false;
  }
  bool finite = true;
#pragma unroll
  for (int i = 0; i < NI; ++i)
    if (i < din && !(fabs(ub[i]) < 3.0e38)) finite = false;
  s.reject = inside ? 0 : 1;
  s.lq_fwd = inside ? sample_logq(Lm, mu, ld, ub, eps, din, hold_free<HOLD>(ho, din)) : 0.0;
#pragma unroll
  for (int i = 0; i < NI; ++i)
    if (i < din) upr[i] = finite ? (float)ub[i] : s.p.u[i];
}

// one thread per chain, after evaluation number `it` of the call (lnl_new, g_new, F_new at u_prop, u coordinates):
// the pending proposal is decided (sample_decide), a kept transition accumulated and stored (sample_keep) and, unless
// it == a.total, the proposal of transition `it` drawn and written to u_prop (sample_draw).  T: the samples' type;
// PRIOR: the handle holds a prior record, pr (else not read).  HOLD: it holds a hold record; Hold: HoldArgs for HOLD =
// true, no argument for HOLD = false.
template <class T, bool PRIOR, bool HOLD, class... Hold>
__global__ void __launch_bounds__(256) sample_step_kernel(SampleRow* __restrict__ st, float* __restrict__ up, const float* __restrict__ lnl_new,
                                                          const float* __restrict__ g_new, const float* __restrict__ F_new, long long it,
                                                          const SampleArgs a, const PriorArgs pr, const Hold... hold) {
  static_assert(sizeof...(Hold) == (HOLD ? 1 : 0), "HOLD takes one HoldArgs, its absence nothing");
  [[maybe_unused]] const auto& ho = hold_of(hold...);
  constexpr int NI = kFitMaxIn, NP = kFitPacked;
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= a.n) return;
  const int din = a.din;
  SampleRow& s = st[row];
  float* upr = up + row * din;
  double eps = s.eps;
  double u[NI], Lm[NP], mu[NI];
  bool have_factor = false;  // Lm, mu and ld below belong to the current point
  double ld = 0.0;
  const bool accept =
      sample_decide<false, PRIOR, HOLD>(s, upr, lnl_new + row, g_new + row * din, F_new + row * din * din, it, row, a, 1.0, pr, ho, eps, Lm,
                                        mu, ld, have_factor);
  // the current point
  s.p.widen_u(din, u);
  sample_keep<T>(s, u, accept, it, row, a);
  if (it == a.total) return;
  sample_draw<false, PRIOR, HOLD>(s, upr, u, it, row, a, 1.0, pr, ho, eps, Lm, mu, ld, have_factor);
}

// ---- parallel tempering (include/v21.h: v21_mlp_sample_tempered): T consecutive rows are the rungs of one ladder, row r
// at inverse temperature betas[r % T].  A 256-thread workgroup takes floor(256 / T) whole ladders (rows_per_wg rows;
// its other threads and the rows past n only meet the barriers), so the partners of a swap are threads of one
// workgroup.  A swap event exchanges the EvalPoints of the swapping pairs through global memory: both rows of a pair
// form the same decision from the two stored ln L and the lower row's Philox word, a swapping row reads its partner's
// point into registers, a barrier follows, then it writes that point over its own.  The prior cancels in the swap rule.
struct TemperArgs {
  int T, swap_every, rows_per_wg;
  double betas[32];
};
// what a row accumulates beside SampleRow's moments, over the kept transitions: sum ln L, sum ln L^2 (un-tempered, after
// the swap event) and, as the lower row of a pair, the swaps proposed and accepted
struct TemperRow {
  double sl, sll;
  long long proposed, swapped;
};

template <class T, bool PRIOR, bool HOLD, class... Hold>
__global__ void __launch_bounds__(256) sample_step_tempered_kernel(SampleRow* st, TemperRow* __restrict__ tr, float* __restrict__ up,
                                                                   const float* __restrict__ lnl_new, const float* __restrict__ g_new,
                                                                   const float* __restrict__ F_new, long long it, const SampleArgs a,
                                                                   const TemperArgs ta, const PriorArgs pr, const Hold... hold) {
  static_assert(sizeof...(Hold) == (HOLD ? 1 : 0), "HOLD takes one HoldArgs, its absence nothing");
  [[maybe_unused]] const auto& ho = hold_of(hold...);
  constexpr int NI = kFitMaxIn, NP = kFitPacked;
  const long long row = (long long)blockIdx.x * ta.rows_per_wg + threadIdx.x;
  // (no thread returns before the last barrier: one that is not `active` skips the work between them)
  const bool active = (int)threadIdx.x < ta.rows_per_wg && row < a.n;
  const int din = a.din;
  const int k = (int)threadIdx.x % ta.T;  // the rung: rows_per_wg and the call's first row are multiples of T
  const double beta = ta.betas[k];
  float* upr = up + row * din;
  double eps = 0.0, ld = 0.0;
  double u[NI], Lm[NP], mu[NI];
  bool have_factor = false, accept = false;
  if (active) {
    eps = st[row].eps;
    accept = sample_decide<true, PRIOR, HOLD>(st[row], upr, lnl_new + row, g_new + row * din, F_new + row * din * din, it, row, a, beta, pr,
                                              ho, eps, Lm, mu, ld, have_factor);
  }
  // the swap event that follows transition S = step0 + it - 1: the same branch for every thread of the launch
  const uint64_t s1 = a.step0 + (uint64_t)it;  // S + 1
  if (it > 0 && ta.swap_every > 0 && s1 % (uint64_t)ta.swap_every == 0) {
    __syncthreads();  // (the points the decisions above took are in place)
    constexpr int NW = (int)(sizeof(EvalPoint) / sizeof(float));  // (word by word: the partner's point stays in registers)
    static_assert(sizeof(EvalPoint) == NW * sizeof(float), "EvalPoint is floats throughout");
    float other[NW];
    bool swap = false;
    const int lo_k = (k & 1) == (int)((s1 / (uint64_t)ta.swap_every - 1) & 1) ? k : k - 1;  // the lower rung of this row's pair
    if (active && lo_k >= 0 && lo_k + 1 < ta.T) {
      const long long lo = row - (k - lo_k);
      const double rhs = (ta.betas[lo_k] - ta.betas[lo_k + 1]) * ((double)st[lo + 1].p.lnl - (double)st[lo].p.lnl);
      uint32_t w[4];
      sample_block(a.seed, a.chain0 + (uint64_t)lo, (uint32_t)(s1 - 1), 3u, w);
      swap = log(sample_uniform(w[0])) < rhs;  // (a NaN right-hand side refuses)
      if (swap) {
        const float* src = (const float*)&st[k == lo_k ? lo + 1 : lo].p;
#pragma unroll
        for (int i = 0; i < NW; ++i) other[i] = src[i];
      }
      if (k == lo_k && it > a.n_warmup) {
        tr[row].proposed += 1;
        if (swap) tr[row].swapped += 1;
      }
    }
    __syncthreads();  // (every partner's point is in registers)
    if (swap) {
      float* dst = (float*)&st[row].p;
#pragma unroll
      for (int i = 0; i < NW; ++i) dst[i] = other[i];
      have_factor = false;  // (the factor in registers belonged to the point that left)
    }
  }
  if (!active) return;
  SampleRow& s = st[row];
  s.p.widen_u(din, u);
  if (it > a.n_warmup) {
    const double l = (double)s.p.lnl;
    tr[row].sl += l;
    tr[row].sll += l * l;
  }
  sample_keep<T>(s, u, accept, it, row, a);
  if (it == a.total) return;
  sample_draw<true, PRIOR, HOLD>(s, upr, u, it, row, a, beta, pr, ho, eps, Lm, mu, ld, have_factor);
}

// one thread per chain: the last state in raw units (raw_row) and the per-chain results (nullable; the moments'
// over `kept` transitions: Moments::finish)
struct SampleOutDev {
  void* x_last;
  float* lnl_last;
  double *eps_last, *accept_rate, *mean_u, *cov_u;
  float* last_prop_u;
  double* last_log_alpha;
};
template <class T, bool HOLD, class... Hold>
__global__ void __launch_bounds__(256) sample_finish_kernel(const SampleRow* __restrict__ st, const float* __restrict__ up, long long n, int din,
                                                            long long kept, const v21_affine_in t, const SampleOutDev o, const Hold... hold) {
  static_assert(sizeof...(Hold) == (HOLD ? 1 : 0), "HOLD takes one HoldArgs, its absence nothing");
  [[maybe_unused]] const auto& ho = hold_of(hold...);
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const SampleRow& s = st[row];
  raw_row<T>(o.x_last, row, din, s.p.u, t);
  if (o.lnl_last) o.lnl_last[row] = s.p.lnl;
  if (o.eps_last) o.eps_last[row] = s.eps;
  s.m.finish(row, din, kept, s.p.u, o.mean_u, o.cov_u, o.accept_rate);
  hold_finish<HOLD>(ho, row, din, o.mean_u, o.cov_u);
  if (o.last_prop_u)
    for (int j = 0; j < din; ++j) o.last_prop_u[row * din + j] = up[row * din + j];
  if (o.last_log_alpha) o.last_log_alpha[row] = s.log_alpha;
}

// one thread per row: the tempered results (nullable) over `kept` transitions: mean_lnl = sum ln L / K, var_lnl = sum
// ln L^2 / K - mean_lnl^2, swap_accept = swapped / proposed (kept == 0: the current ln L, 0; nothing proposed: 0)
struct TemperOutDev {
  double *mean_lnl, *var_lnl, *swap_accept;
};
static __global__ void __launch_bounds__(256) sample_finish_tempered_kernel(const SampleRow* __restrict__ st, const TemperRow* __restrict__ tr,
                                                                            long long n, long long kept, const TemperOutDev o) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const TemperRow& t = tr[row];
  const double inv = kept > 0 ? 1.0 / (double)kept : 0.0;
  const double mean = kept > 0 ? t.sl * inv : (double)st[row].p.lnl;
  if (o.mean_lnl) o.mean_lnl[row] = mean;
  if (o.var_lnl) o.var_lnl[row] = kept > 0 ? t.sll * inv - mean * mean : 0.0;
  if (o.swap_accept) o.swap_accept[row] = t.proposed > 0 ? (double)t.swapped / (double)t.proposed : 0.0;
}

}  // namespace v21
