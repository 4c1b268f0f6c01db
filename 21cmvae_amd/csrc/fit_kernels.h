// fit_kernels.h -- projected Levenberg-Marquardt fits on the device (api_fit.hip), one thread per row in the transformed
// coordinates u in [-1, 1]^din (rowmath.h), on the evaluations (ln L, gradient, Fisher matrix) of jac_reduce_kernel
// (reduce_kernels.h):
//   fit_init_kernel    clamps the transformed start rows into the box and resets the row state;
//   fit_lm_kernel      accept / reject the evaluated proposal, then the next damped Gauss-Newton step, solved by a
//                      float64 Cholesky factorisation in registers; <false>: of ln L, <true>: of ln L + ln p under the
//                      handle's prior record with held columns masked out of the solve (the MAP fit);
//   fit_finish_kernel  the accepted point back to raw parameters and the results;
//   fit_map_finish_kernel  the same and ln p, the Laplace evidence and the posterior precision there.
#pragma once
#include <hip/hip_runtime.h>

#include "rowmath.h"

namespace v21 {

constexpr double kFitLamMin = 1e-12, kFitLamMax = 1e12, kFitTiny = 1e-30;
constexpr double kFitLn2Pi = 1.8378770664093454835606594728112;
// per-row state; status: -1 running, 0 iteration limit, 1 converged (||step||_inf <= xtol), 2 no improving step
// (lambda > kFitLamMax), 3 no information (every diag(F) == 0)
struct FitRow {
  EvalPoint p;                   // accepted point
  float lnl0;                    // ln L at the start
  double lam;
  int status;
  int iters;                     // accepted + rejected proposals evaluated after the start
};

// one thread per row: u_prop (pitch din, the rows the next evaluation reads) into the box (box_clamp), the state reset
static __global__ void __launch_bounds__(256) fit_init_kernel(FitRow* __restrict__ st, float* __restrict__ up, float* __restrict__ fac,
                                                       long long n, int din, double lam0) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  box_clamp(up + row * din, fac + row * din, din);
  FitRow& s = st[row];
  s.lam = lam0;
  s.p.lnl = 0.f;
  s.lnl0 = 0.f;
  s.status = -1;
  s.iters = 0;
}

// ---- the MAP fit (include/v21.h: v21_mlp_fit_map).  What fit_lm_kernel<true, FitMapArgs> and fit_map_finish_kernel
// take beside the plain fit's arguments, by value: the handle's prior record (read only with use_prior), and per input
// column whether it is held.  The plain fit's kernel takes nothing more: its argument list is what it was.
struct FitMapArgs {
  PriorArgs pr;
  int use_prior;
  int hold[kFitMaxIn];

  // the record the fit works with: the normal columns that are not held (a held column is no parameter: its prior is
  // never read); without use_prior nothing of pr is read
  __device__ __forceinline__ PriorArgs free_prior() const {
    PriorArgs f;
#pragma unroll
    for (int i = 0; i < kFitMaxIn; ++i) {
      const bool on = use_prior && !hold[i] && pr.kind[i];
      f.kind[i] = on ? 1 : 0;
      f.mu[i] = on ? pr.mu[i] : 0.0;
      f.w[i] = on ? pr.w[i] : 0.0;
      f.wmu[i] = on ? pr.wmu[i] : 0.0;
    }
    return f;
  }
  // the system of the posterior at u: g += grad ln p, F += diag(1 / sd^2) on the free normal columns, then a held
  // column i becomes g_i = 0, F_ij = F_ji = 0 (j != i), F_ii = 1: its delta is exactly 0 and its pivot 1
  __device__ __forceinline__ void system(const PriorArgs& f, const double* u, int din, double* g, double* F) const {
    constexpr int NI = kFitMaxIn;
    prior_eval<true>(f, u, din, g, F);
    int p = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      if (i < din && hold[i]) g[i] = 0.0;
#pragma unroll
      for (int j = i; j < NI; ++j, ++p)
        if (j < din && (hold[i] || hold[j])) F[p] = i == j ? 1.0 : 0.0;
    }
  }
};
struct FitNoMap {};
__device__ __forceinline__ FitNoMap fit_map_of() { return {}; }
__device__ __forceinline__ const FitMapArgs& fit_map_of(const FitMapArgs& a) { return a; }

// one thread per row, after the evaluation (lnl_new, g_new, F_new: u coordinates) of the proposal u_prop.  first: the
// evaluation of the start, accepted whatever its value.  Running rows are counted into *active.
// MAP = false: the maximum-likelihood fit.  MAP = true: the objective is ln L + ln p, ln p recomputed from the stored u
// in float64 (the state's lnl stays ln L alone), on the system FitMapArgs::system forms; "no information" is tested on
// the diagonal of that system over the free columns (no free column: nothing to move, the step is 0).  Map: FitMapArgs
// for MAP = true, no argument for MAP = false.
template <bool MAP, class... Map>
__global__ void __launch_bounds__(256) fit_lm_kernel(FitRow* __restrict__ st, float* __restrict__ up, const float* __restrict__ lnl_new,
                                                     const float* __restrict__ g_new, const float* __restrict__ F_new, long long n,
                                                     int din, int first, double xtol, int* __restrict__ active,
                                                     const Map... map) {
  static_assert(sizeof...(Map) == (MAP ? 1 : 0), "the MAP fit takes one FitMapArgs, the plain fit nothing");
  [[maybe_unused]] const auto& ma = fit_map_of(map...);
  constexpr int NI = kFitMaxIn;
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  FitRow& s = st[row];
  if (s.status >= 0) return;
  float* u = up + row * din;
  double lam = s.lam;
  const float ln = lnl_new[row];
  if (!first) s.iters += 1;
  [[maybe_unused]] PriorArgs pf;
  bool rose;
  if constexpr (MAP) {
    pf = ma.free_prior();
    rose = first || (double)ln + prior_logp(pf, u, din) > (double)s.p.lnl + prior_logp(pf, s.p.u, din);
  } else {
    rose = first || ln > s.p.lnl;
  }
  if (rose) {
    if (first) s.lnl0 = ln;
    s.p.take(u, ln, g_new + row * din, F_new + row * din * din, din);
    lam = fmax(lam / 10.0, kFitLamMin);
  } else {
    lam *= 10.0;
  }
  // the accepted point in float64; without information on its diagonal there is no step
  double F[kFitPacked], g[NI], ua[NI];
  s.p.widen_u(din, ua);
  s.p.widen(din, g, F);
  bool info = false;
  if constexpr (MAP) {
    ma.system(pf, ua, din, g, F);
    bool any_free = false;
#pragma unroll
    for (int i = 0, p = 0; i < NI; p += NI - i, ++i)
      if (i < din && !ma.hold[i]) {
        any_free = true;
        if (F[p] != 0.0) info = true;
      }
    if (!any_free) info = true;
  } else {
#pragma unroll
    for (int i = 0, p = 0; i < NI; p += NI - i, ++i)
      if (i < din && F[p] != 0.0) info = true;
  }
  int status = -1;
  double delta[NI] = {};
  if (!info) {
    status = 3;
  } else {
    // delta = A^-1 g, A = F + lam diag(max(F_ii, tiny)), lam raised until A has a Cholesky factor
    for (;;) {
      if (lam > kFitLamMax) { status = 2; break; }
      double Lm[kFitPacked], z[NI];
      const bool ok = chol_factor(F, din, Lm, [&](int i) { return lam * fmax(F[i * NI - i * (i - 1) / 2], kFitTiny); },
                                  [](double pivot) { return pivot > 0.0; });
      if (!ok) { lam *= 10.0; continue; }
      solve_lower(Lm, g, z);
      solve_upper(Lm, z, delta);
      break;
    }
  }
  s.lam = lam;
  if (status < 0) {
    // the projected step
    double step = 0.0;
    float un[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const double v = fmin(fmax(ua[i] + delta[i], -1.0), 1.0);
      un[i] = (float)v;
      // (belt and braces: a held delta is exactly 0 and (float)clamp((double)u) is the stored u already, unless a free
      // column's NaN reached it through the solve)
      if constexpr (MAP)
        if (i < din && ma.hold[i]) un[i] = s.p.u[i];
      if (i < din) step = fmax(step, fabs((double)un[i] - ua[i]));
    }
    if (step <= xtol) {
      status = 1;
    } else {
#pragma unroll
      for (int i = 0; i < NI; ++i)
        if (i < din) u[i] = un[i];
      atomicAdd(active, 1);
      return;
    }
  }
  // stopped: the row keeps its accepted point (and later evaluations of it change nothing)
  s.status = status;
#pragma unroll
  for (int i = 0; i < NI; ++i)
    if (i < din) u[i] = s.p.u[i];
}

// one thread per row: x_hat (of type T) = the accepted point in raw units (raw_row), and the per-row results (nullable)
template <class T>
__global__ void __launch_bounds__(256) fit_finish_kernel(const FitRow* __restrict__ st, void* __restrict__ x_hat, float* __restrict__ lnl,
                                  float* __restrict__ lnl0, int* __restrict__ status, long long n, int din, const v21_affine_in t) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const FitRow& s = st[row];
  raw_row<T>(x_hat, row, din, s.p.u, t);
  if (lnl) lnl[row] = s.p.lnl;
  if (lnl0) lnl0[row] = s.lnl0;
  if (status) status[row] = s.status < 0 ? 0 : s.status;
}

// one thread per row, the MAP fit's finish: fit_finish_kernel's results, and (each nullable) at the accepted point u^,
// on A = F(u^) + P with the held rows and columns those of the identity (FitMapArgs::system, lambda = 0):
//   lnp      ln p(u^), unnormalised, over the free normal columns;
//   laplace  ln L + ln p + d_free / 2 ln 2 pi - 1/2 ln det A, the determinant from the diagonal of A's Cholesky factor
//            (a held pivot is 1 and adds 0); NaN when a pivot is not positive and finite;
//   prec_u   A (din, din) in float32, both triangles from one value.
template <class T>
__global__ void __launch_bounds__(256) fit_map_finish_kernel(const FitRow* __restrict__ st, void* __restrict__ x_hat, float* __restrict__ lnl,
                                      float* __restrict__ lnl0, int* __restrict__ status, double* __restrict__ lnp,
                                      double* __restrict__ laplace, float* __restrict__ prec_u, long long n, int din,
                                      const v21_affine_in t, const FitMapArgs ma) {
  constexpr int NI = kFitMaxIn;
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const FitRow& s = st[row];
  raw_row<T>(x_hat, row, din, s.p.u, t);
  if (lnl) lnl[row] = s.p.lnl;
  if (lnl0) lnl0[row] = s.lnl0;
  if (status) status[row] = s.status < 0 ? 0 : s.status;
  if (!lnp && !laplace && !prec_u) return;
  const PriorArgs pf = ma.free_prior();
  const double lp = prior_logp(pf, s.p.u, din);
  if (lnp) lnp[row] = lp;
  if (!laplace && !prec_u) return;
  double F[kFitPacked], g[NI], ua[NI];
  s.p.widen_u(din, ua);
  s.p.widen(din, g, F);
  ma.system(pf, ua, din, g, F);
  if (prec_u) {
    int p = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = i; j < NI; ++j, ++p)
        if (j < din) {
          const float a = (float)F[p];
          prec_u[(row * din + i) * din + j] = a;
          prec_u[(row * din + j) * din + i] = a;
        }
  }
  if (laplace) {
    double Lm[kFitPacked];
    const bool ok = chol_factor(F, din, Lm, [](int) { return 0.0; }, [](double pivot) { return pivot > 0.0 && pivot < INFINITY; });
    double half_logdet = 0.0;
    int d_free = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i)
      if (i < din) {
        half_logdet += log(Lm[i * (i + 1) / 2 + i]);
        if (!ma.hold[i]) d_free += 1;
      }
    laplace[row] = ok ? (double)s.p.lnl + lp + 0.5 * (double)d_free * kFitLn2Pi - half_logdet : (double)NAN;
  }
}

}  // namespace v21
