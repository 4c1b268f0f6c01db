// sample_kernels.h -- posterior sampling on the device (api_sample.hip): a batched Metropolis-adjusted Langevin sampler
// whose metric is the Fisher matrix at the current point ("simplified manifold MALA"), one thread per chain, in the
// transformed coordinates u in [-1, 1]^din of the fit (fit_kernels.h) under a uniform prior on that box.
//   sample_init_kernel    clamps the transformed start rows into the box and resets the chain state;
//   sample_step_kernel    consumes the evaluation (ln L, gradient, Fisher matrix: jac_reduce_kernel) of the pending
//                         proposal: accepts or rejects it, adapts the step size in warm-up, accumulates the moments,
//                         stores a thinned sample in raw units, then draws and writes the next proposal;
//   sample_finish_kernel  the last state back to raw parameters and the results.
// The transition, with G(u) = F(u) + ridge I = L L^T, d = din and step size e:
//   mu(u) = u + e^2 / 2 G(u)^-1 g(u);   u' = float32(mu(u) + e L(u)^-T xi),  xi ~ N(0, I_d)
//   log q(b | a) = -|L(a)^T (b - mu(a))|^2 / (2 e^2) + sum_i log L_ii(a) - d / 2 log(2 pi e^2)
//   log alpha = lnL(u') - lnL(u) + log q(u | u') - log q(u' | u);   accept iff log(uniform) < log alpha
// (the metric's derivative term of full manifold MALA is left out; the acceptance uses the q that was really drawn
// from, at the float32 u' that is really evaluated, so the chain is exact).  A proposal with a coordinate outside
// [-1, 1], or whose G has no finite Cholesky factor, is rejected: log alpha = -inf, its evaluation is not read.
// Cholesky, solves (rowmath.h) and log-densities are float64 in registers.  Random numbers: Philox4x32-10, include/v21.h.
#pragma once
#include <hip/hip_runtime.h>

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
  double su[kFitMaxIn];          // moments of the kept transitions: sum u, sum u u^T (upper triangle), accepted
  double suu[kFitPacked];
  long long accepted;
};

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
__device__ inline bool sample_chol(const double* F, double ridge, int din, double* Lm) {
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
// log q(b | a) from a's factor, drift and log-determinant term
__device__ inline double sample_logq(const double* Lm, const double* mu, double ld, const double* b, double eps, int din) {
  constexpr int NI = kFitMaxIn;
  double q = 0.0;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    double v = 0.0;  // (L^T (b - mu))_i = sum_{k >= i} L[k][i] (b - mu)_k
#pragma unroll
    for (int k = i; k < NI; ++k) v += Lm[k * (k + 1) / 2 + i] * (b[k] - mu[k]);
    if (i < din) q += v * v;
  }
  return -q / (2.0 * eps * eps) + ld - 0.5 * din * log(kSampleTwoPi * eps * eps);
}

// one thread per chain: u_prop (pitch din, the rows the next evaluation reads) into the box (box_clamp), the state reset;
// the step size from eps_start (nullable: eps0)
static __global__ void __launch_bounds__(256) sample_init_kernel(SampleRow* __restrict__ st, float* __restrict__ up, float* __restrict__ fac,
                                                                 long long n, int din, double eps0, const double* __restrict__ eps_start) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  box_clamp(up + row * din, fac + row * din, din);
  SampleRow& s = st[row];
  double e = eps_start ? eps_start[row] : eps0;
  s.eps = e > 0.0 && e < 1.79e308 ? e : eps0;
  s.p.lnl = 0.f;
  s.reject = 0;
  s.lq_fwd = 0.0;
  s.log_alpha = 0.0;
  for (int i = 0; i < kFitMaxIn; ++i) s.su[i] = 0.0;
  for (int i = 0; i < kFitPacked; ++i) s.suu[i] = 0.0;
  s.accepted = 0;
}

// one thread per chain, after evaluation number `it` of the call (lnl_new, g_new, F_new at u_prop, u coordinates):
// it == 0 is the start's, accepted whatever its value; it >= 1 is the proposal's of transition it - 1, which is decided
// here.  Unless it == a.total the proposal of transition `it` is then drawn and written to u_prop.  T: the samples' type.
template <class T>
__global__ void __launch_bounds__(256) sample_step_kernel(SampleRow* __restrict__ st, float* __restrict__ up, const float* __restrict__ lnl_new,
                                                          const float* __restrict__ g_new, const float* __restrict__ F_new, long long it,
                                                          const SampleArgs a) {
  constexpr int NI = kFitMaxIn, NP = kFitPacked;
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= a.n) return;
  const int din = a.din;
  SampleRow& s = st[row];
  float* upr = up + row * din;
  const float *gn = g_new + row * din, *Fn = F_new + row * din * din;
  double eps = s.eps;
  double F[NP], g[NI], u[NI], Lm[NP], mu[NI];
  bool have_factor = false;  // Lm, mu and ld below belong to the current point
  double ld = 0.0;
  bool accept = it == 0;
  if (it > 0) {
    // the proposal's side of the acceptance ratio
    double log_alpha = -INFINITY;
    if (!s.reject) {
      double up64[NI];
      widen_row(upr, din, up64);
      widen_eval(gn, Fn, din, g, F);
      s.p.widen_u(din, u);
      if (sample_chol(F, a.ridge, din, Lm)) {
        ld = sample_drift(Lm, up64, g, eps, din, mu);
        const double lq_rev = sample_logq(Lm, mu, ld, u, eps, din);
        log_alpha = (double)lnl_new[row] - (double)s.p.lnl + lq_rev - s.lq_fwd;
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
  if (accept) s.p.take(upr, lnl_new[row], gn, Fn, din);
  // the current point
  s.p.widen_u(din, u);
  if (it > a.n_warmup) {
    // a kept transition: moments, and every thin-th state in raw units
    int p = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      if (i < din) s.su[i] += u[i];
#pragma unroll
      for (int j = i; j < NI; ++j, ++p)
        if (j < din) s.suu[p] += u[i] * u[j];
    }
    if (accept) s.accepted += 1;
    const long long k = it - a.n_warmup;  // kept transitions so far
    if (a.thin > 0 && k % a.thin == 0 && k / a.thin <= a.n_keep) {
      const long long slot = row * a.n_keep + (k / a.thin - 1);
      if (a.samples)
        for (int j = 0; j < din; ++j) ((T*)a.samples)[slot * din + j] = (T)box_to_raw(u[j], j, a.t);
      if (a.samples_lnl) a.samples_lnl[slot] = s.p.lnl;
    }
  }
  if (it == a.total) return;
  // the proposal of transition `it`
  if (!have_factor) {
    s.p.widen(din, g, F);
    if (!sample_chol(F, a.ridge, din, Lm)) {
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
  // u' = mu + eps L^-T xi, rounded to the float32 that is evaluated
  double v[NI], ub[NI];
  bool inside = true;
  solve_upper(Lm, xi, v);
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const float f = (float)(mu[i] + eps * v[i]);
    ub[i] = i < din ? (double)f : 0.0;
    if (i < din && !(f >= -1.f && f <= 1.f)) inside = false;
  }
  bool finite = true;
#pragma unroll
  for (int i = 0; i < NI; ++i)
    if (i < din && !(fabs(ub[i]) < 3.0e38)) finite = false;
  s.reject = inside ? 0 : 1;
  s.lq_fwd = inside ? sample_logq(Lm, mu, ld, ub, eps, din) : 0.0;
#pragma unroll
  for (int i = 0; i < NI; ++i)
    if (i < din) upr[i] = finite ? (float)ub[i] : s.p.u[i];
}

// one thread per chain: the last state in raw units (box_to_raw) and the per-chain
// results (nullable): with K kept transitions, mean_u = sum u / K, cov_u = sum u u^T / K - mean_u mean_u^T (both
// triangles), accept_rate = accepted / K (K == 0: the current point, zeros, 0)
struct SampleOutDev {
  void* x_last;
  float* lnl_last;
  double *eps_last, *accept_rate, *mean_u, *cov_u;
  float* last_prop_u;
  double* last_log_alpha;
};
template <class T>
__global__ void __launch_bounds__(256) sample_finish_kernel(const SampleRow* __restrict__ st, const float* __restrict__ up, long long n, int din,
                                                            long long kept, const v21_affine_in t, const SampleOutDev o) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const SampleRow& s = st[row];
  for (int j = 0; j < din; ++j) ((T*)o.x_last)[row * din + j] = (T)box_to_raw((double)s.p.u[j], j, t);
  if (o.lnl_last) o.lnl_last[row] = s.p.lnl;
  if (o.eps_last) o.eps_last[row] = s.eps;
  if (o.accept_rate) o.accept_rate[row] = kept > 0 ? (double)s.accepted / (double)kept : 0.0;
  const double inv = kept > 0 ? 1.0 / (double)kept : 0.0;
  if (o.mean_u)
    for (int j = 0; j < din; ++j) o.mean_u[row * din + j] = kept > 0 ? s.su[j] * inv : (double)s.p.u[j];
  if (o.cov_u) {
    int p = 0;
    for (int i = 0; i < kFitMaxIn; ++i)
      for (int j = i; j < kFitMaxIn; ++j, ++p)
        if (j < din) {
          const double c = kept > 0 ? s.suu[p] * inv - (s.su[i] * inv) * (s.su[j] * inv) : 0.0;
          o.cov_u[(row * din + i) * din + j] = c;
          o.cov_u[(row * din + j) * din + i] = c;
        }
  }
  if (o.last_prop_u)
    for (int j = 0; j < din; ++j) o.last_prop_u[row * din + j] = up[row * din + j];
  if (o.last_log_alpha) o.last_log_alpha[row] = s.log_alpha;
}

}  // namespace v21
