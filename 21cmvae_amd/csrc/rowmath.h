// rowmath.h -- what the per-row step kernels of the fit (fit_kernels.h) and the samplers (sample_kernels.h,
// ensemble_kernels.h) share: one thread per row, float64 in registers, in the transformed coordinates u in [-1, 1]^din (the training box par_transform
// maps to), din <= kFitMaxIn.  Packed layouts: a symmetric matrix as its upper triangle by rows (element (i, j), i <= j, at
// i NI - i (i - 1) / 2 + (j - i)), a Cholesky factor L as its lower triangle by rows (L[i][j] at i (i + 1) / 2 + j); rows
// and columns >= din are those of the identity, so every loop runs over NI = kFitMaxIn with constant indices.
//   EvalPoint               a point with its evaluation (ln L, gradient, Fisher matrix): the head of the row states;
//   widen_row / widen_upper / widen_eval  a row of din floats, a Fisher matrix, and an evaluation row's gradient and
//                           Fisher matrix, to float64 registers;
//   chol_factor             L of F + diag(addend), the caller's addend and pivot test;
//   solve_lower / _upper    L z = g and L^T x = z;
//   box_clamp1 / box_clamp  a coordinate, and a start row, into the box;
//   box_to_raw / raw_row    a coordinate, and a row of a result, back to raw units;
//   PriorArgs               the prior record as the step kernels take it;
//   prior_logp / prior_eval its ln p, and its gradient and precision added to an evaluation;
//   HoldArgs / NoHold       the hold record as the samplers' kernels take it (HOLD), and its absence;
//   hold_eval / hold_row / hold_free / hold_finish  a held column in an evaluation, a row, the count, the results;
//   Moments                 the bookkeeping of a sampler's kept transitions, the tail of its row state: the sums of u and
//                           u u^T and the accepted count, the thinned store of a state, the per-row results.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/v21_types.h"

namespace v21 {

constexpr int kFitMaxIn = 8;
constexpr int kFitPacked = kFitMaxIn * (kFitMaxIn + 1) / 2;

// the handle's prior record (include/v21.h: v21_mlp_set_prior; api_prior.hip) as the step kernels of the four samplers
// and of the MAP fit receive it, by value: per input column its kind (0: uniform on [-1, 1], 1: normal(mu, sd) truncated
// to it), mu, w = 1 / sd^2 and wmu = mu / sd^2.  Columns >= din are never read.
struct PriorArgs {
  int kind[kFitMaxIn];
  double mu[kFitMaxIn], w[kFitMaxIn], wmu[kFitMaxIn];
};

// ---- the prior record in the step kernels of the four samplers and of the MAP fit.  PRIOR = false: none of it is
// read, the arithmetic is the uniform prior's.
// ln p(u), unnormalised: -1/2 sum_i w_i (u_i - mu_i)^2 over the normal columns
template <class U>
__device__ __forceinline__ double prior_logp(const PriorArgs& pr, const U* u, int din) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < kFitMaxIn; ++i)
    if (i < din && pr.kind[i]) {
      const double d = (double)u[i] - pr.mu[i];
      s += pr.w[i] * d * d;
    }
  return -0.5 * s;
}
// g += grad ln p(u) = w mu - w u and F += diag(w), g and F (packed upper triangle) those of u
template <bool PRIOR>
__device__ __forceinline__ void prior_eval(const PriorArgs& pr, const double* u, int din, double* g, double* F) {
  if constexpr (PRIOR) {
#pragma unroll
    for (int i = 0; i < kFitMaxIn; ++i)
      if (i < din && pr.kind[i]) {
        g[i] += pr.wmu[i] - pr.w[i] * u[i];
        F[i * kFitMaxIn - i * (i - 1) / 2] += pr.w[i];
      }
  }
}

// ---- the handle's hold record (include/v21.h: v21_mlp_set_hold; api_hold.hip) as the init, step and finish kernels of
// the four samplers receive it, by value: bit i of mask set = input column i is held at u[i], the float32 every state,
// proposal and stored sample of that column carries.  A kernel's HOLD = false form takes no such argument (a parameter
// pack, as fit_lm_kernel's Map): its argument list and its code are what they were.
struct HoldArgs {
  unsigned mask;
  float u[kFitMaxIn];
  __device__ __forceinline__ bool held(int i) const { return (mask >> i) & 1u; }
};
struct NoHold {};
__device__ __forceinline__ NoHold hold_of() { return {}; }
__device__ __forceinline__ const HoldArgs& hold_of(const HoldArgs& h) { return h; }
// a held column i of an evaluation (g, packed F), after the prior's additions: g_i = 0, F_ij = F_ji = 0 (j != i),
// F_ii = 1 -- the arithmetic of FitMapArgs::system (fit_kernels.h)
template <bool HOLD, class H>
__device__ __forceinline__ void hold_eval(const H& ho, int din, double* g, double* F) {
  if constexpr (HOLD) {
    int p = 0;
#pragma unroll
    for (int i = 0; i < kFitMaxIn; ++i) {
      if (i < din && ho.held(i)) g[i] = 0.0;
#pragma unroll
      for (int j = i; j < kFitMaxIn; ++j, ++p)
        if (j < din && (ho.held(i) || ho.held(j))) F[p] = i == j ? 1.0 : 0.0;
    }
  }
}
// the held coordinates written over those of a row of din floats
template <bool HOLD, class H>
__device__ __forceinline__ void hold_row(const H& ho, int din, float* u) {
  if constexpr (HOLD) {
#pragma unroll
    for (int i = 0; i < kFitMaxIn; ++i)
      if (i < din && ho.held(i)) u[i] = ho.u[i];
  }
}
// d_free: the columns that are sampled (HOLD = false: din itself)
template <bool HOLD, class H>
__device__ __forceinline__ int hold_free(const H& ho, int din) {
  if constexpr (HOLD) return din - __popc(ho.mask);
  else return din;
}
// a sampler's per-row results after Moments::finish: mean_u of a held column is the held value, its row and column of
// cov_u exact zeros (both nullable)
template <bool HOLD, class H>
__device__ __forceinline__ void hold_finish(const H& ho, long long row, int din, double* mean_u, double* cov_u) {
  if constexpr (HOLD) {
    for (int i = 0; i < din; ++i)
      if (ho.held(i)) {
        if (mean_u) mean_u[row * din + i] = (double)ho.u[i];
        if (cov_u)
          for (int j = 0; j < din; ++j) cov_u[(row * din + i) * din + j] = cov_u[(row * din + j) * din + i] = 0.0;
      }
  }
}

// din floats in float64 registers, zeros past din
__device__ inline void widen_row(const float* v, int din, double* v64) {
#pragma unroll
  for (int i = 0; i < kFitMaxIn; ++i) v64[i] = i < din ? (double)v[i] : 0.0;
}
// a Fisher matrix to packed float64 registers, zeros past din; at(i, j, p): where the source holds element (i, j), i <= j,
// whose packed position is p
template <class At>
__device__ inline void widen_upper(const float* F, int din, double* F64, At at) {
  int p = 0;
#pragma unroll
  for (int i = 0; i < kFitMaxIn; ++i)
#pragma unroll
    for (int j = i; j < kFitMaxIn; ++j, ++p) F64[p] = j < din ? (double)F[at(i, j, p)] : 0.0;
}

struct EvalPoint {
  float u[kFitMaxIn];   // the point
  float g[kFitMaxIn];   // gradient of ln L there (u coordinates)
  float F[kFitPacked];  // Fisher matrix there, upper triangle by rows
  float lnl;            // ln L there

  // an evaluation row as the new point: up (din), g_new (din), F_new (din, din)
  __device__ void take(const float* up, float lnl_new, const float* g_new, const float* F_new, int din) {
    lnl = lnl_new;
    int p = 0;
#pragma unroll
    for (int i = 0; i < kFitMaxIn; ++i) {
      if (i < din) {
        u[i] = up[i];
        g[i] = g_new[i];
      }
#pragma unroll
      for (int j = i; j < kFitMaxIn; ++j, ++p)
        if (j < din) F[p] = F_new[i * din + j];
    }
  }
  // the point in float64 registers, zeros past din
  __device__ void widen_u(int din, double* u64) const { widen_row(u, din, u64); }
  // its gradient and packed Fisher matrix in float64 registers, zeros past din
  __device__ void widen(int din, double* g64, double* F64) const {
    widen_row(g, din, g64);
    widen_upper(F, din, F64, [](int, int, int p) { return p; });
  }
};

// an evaluation row that is not (yet) taken as the point, the sampler's proposal: g_new (din) and F_new (din, din) in
// float64 registers as EvalPoint::widen leaves them
__device__ inline void widen_eval(const float* g_new, const float* F_new, int din, double* g64, double* F64) {
  widen_row(g_new, din, g64);
  widen_upper(F_new, din, F64, [din](int i, int j, int) { return i * din + j; });
}

// Cholesky factor Lm of A = F + diag(addend(i)); false: pivot_ok(pivot) failed for a row < din (Lm is then not used)
template <class Addend, class PivotOk>
__device__ inline bool chol_factor(const double* F, int din, double* Lm, Addend addend, PivotOk pivot_ok) {
  constexpr int NI = kFitMaxIn;
  bool ok = true;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      // A[i][j] = A[j][i]: the upper triangle's element (j, i)
      const int pu = j * NI - j * (j - 1) / 2 + (i - j);
      double sum = F[pu];
      if (i == j) sum += addend(i);
#pragma unroll
      for (int k = 0; k < j; ++k) sum -= Lm[i * (i + 1) / 2 + k] * Lm[j * (j + 1) / 2 + k];
      if (i == j) {
        if (i < din && !pivot_ok(sum)) ok = false;
        Lm[i * (i + 1) / 2 + i] = i < din ? sqrt(sum) : 1.0;
      } else {
        Lm[i * (i + 1) / 2 + j] = i < din ? sum / Lm[j * (j + 1) / 2 + j] : 0.0;
      }
    }
  }
  return ok;
}
// L z = g (forward substitution)
__device__ inline void solve_lower(const double* Lm, const double* g, double* z) {
  constexpr int NI = kFitMaxIn;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    double sum = g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) sum -= Lm[i * (i + 1) / 2 + k] * z[k];
    z[i] = sum / Lm[i * (i + 1) / 2 + i];
  }
}
// L^T x = z (back substitution)
__device__ inline void solve_upper(const double* Lm, const double* z, double* x) {
  constexpr int NI = kFitMaxIn;
#pragma unroll
  for (int i = NI - 1; i >= 0; --i) {
    double sum = z[i];
#pragma unroll
    for (int k = i + 1; k < NI; ++k) sum -= Lm[k * (k + 1) / 2 + i] * x[k];
    x[i] = sum / Lm[i * (i + 1) / 2 + i];
  }
}

// a coordinate into the box: clamp(v, -1, 1), NaN -> -1 (a log column's non-positive raw value)
__device__ inline float box_clamp1(float v) { return v >= -1.f ? (v <= 1.f ? v : 1.f) : -1.f; }
// a transformed start row (pitch din, the row the next evaluation reads) into the box; fac = 1 (the evaluations run on
// u, without the input transform)
__device__ inline void box_clamp(float* up, float* fac, int din) {
  for (int j = 0; j < din; ++j) {
    up[j] = box_clamp1(up[j]);
    fac[j] = 1.f;
  }
}
// u (transformed) -> raw, float64, the inverse of par_transform: lo + (u + 1) span / 2, then 10^ for a log column (its
// lower bound comes back as 10^lo, e.g. the zero floor, never 0)
__device__ inline double box_to_raw(double u, int j, const v21_affine_in& t) {
  double v = t.lo[j] + (u + 1.0) * t.span[j] / 2.0;
  if (t.log_mask[j]) v = pow(10.0, v);
  return v;
}
// row `row` of x (n, din) of type T = the point u in raw units
template <class T>
__device__ inline void raw_row(void* x, long long row, int din, const float* u, const v21_affine_in& t) {
  for (int j = 0; j < din; ++j) ((T*)x)[row * din + j] = (T)box_to_raw((double)u[j], j, t);
}

// ---- the kept transitions of a sampler's row (a chain, a rung, a walker)
struct Moments {
  double su[kFitMaxIn];    // sum u
  double suu[kFitPacked];  // sum u u^T, upper triangle by rows
  long long accepted;

  __device__ void clear() {
    for (int i = 0; i < kFitMaxIn; ++i) su[i] = 0.0;
    for (int i = 0; i < kFitPacked; ++i) suu[i] = 0.0;
    accepted = 0;
  }
  // one kept transition that ended at u
  __device__ __forceinline__ void add(const double* u, int din, bool accept) {
    int p = 0;
#pragma unroll
    for (int i = 0; i < kFitMaxIn; ++i) {
      if (i < din) su[i] += u[i];
#pragma unroll
      for (int j = i; j < kFitMaxIn; ++j, ++p)
        if (j < din) suu[p] += u[i] * u[j];
    }
    if (accept) accepted += 1;
  }
  // the state (u, lnl) after kept transition k = 1, 2 .. of `row`: every thin-th (thin = 0: none) of the first n_keep thin
  // goes to samples (n, n_keep, din; raw units, type T) and samples_lnl (n, n_keep), both nullable
  template <class T>
  __device__ __forceinline__ static void store(long long row, long long k, long long thin, long long n_keep, void* samples,
                                               float* samples_lnl, const double* u, int din, const float& lnl, const v21_affine_in& t) {
    if (thin > 0 && k % thin == 0 && k / thin <= n_keep) {
      const long long slot = row * n_keep + (k / thin - 1);
      if (samples)
        for (int j = 0; j < din; ++j) ((T*)samples)[slot * din + j] = (T)box_to_raw(u[j], j, t);
      if (samples_lnl) samples_lnl[slot] = lnl;
    }
  }
  // the per-row results (nullable) over K = kept transitions: mean_u = sum u / K, cov_u = sum u u^T / K - mean_u mean_u^T
  // (both triangles), accept_rate = accepted / K (K == 0: the current point u, zeros, 0)
  __device__ void finish(long long row, int din, long long kept, const float* u, double* mean_u, double* cov_u, double* accept_rate) const {
    if (accept_rate) accept_rate[row] = kept > 0 ? (double)accepted / (double)kept : 0.0;
    const double inv = kept > 0 ? 1.0 / (double)kept : 0.0;
    if (mean_u)
      for (int j = 0; j < din; ++j) mean_u[row * din + j] = kept > 0 ? su[j] * inv : (double)u[j];
    if (cov_u) {
      int p = 0;
      for (int i = 0; i < kFitMaxIn; ++i)
        for (int j = i; j < kFitMaxIn; ++j, ++p)
          if (j < din) {
            const double c = kept > 0 ? suu[p] * inv - (su[i] * inv) * (su[j] * inv) : 0.0;
            cov_u[(row * din + i) * din + j] = c;
            cov_u[(row * din + j) * din + i] = c;
          }
    }
  }
};

}  // namespace v21
