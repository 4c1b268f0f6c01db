// fit_kernels.h -- projected Levenberg-Marquardt fits on the device (api_fit.hip), one thread per row in the transformed
// coordinates u in [-1, 1]^din (rowmath.h), on the evaluations (ln L, gradient, Fisher matrix) of jac_reduce_kernel
// (reduce_kernels.h):
//   fit_init_kernel    clamps the transformed start rows into the box and resets the row state;
//   fit_lm_kernel      accept / reject the evaluated proposal, then the next damped Gauss-Newton step, solved by a
//                      float64 Cholesky factorisation in registers;
//   fit_finish_kernel  the accepted point back to raw parameters and the results.
#pragma once
#include <hip/hip_runtime.h>

#include "rowmath.h"

namespace v21 {

constexpr double kFitLamMin = 1e-12, kFitLamMax = 1e12, kFitTiny = 1e-30;
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

// one thread per row, after the evaluation (lnl_new, g_new, F_new: u coordinates) of the proposal u_prop.  first: the
// evaluation of the start, accepted whatever its value.  Running rows are counted into *active.
static __global__ void __launch_bounds__(256) fit_lm_kernel(FitRow* __restrict__ st, float* __restrict__ up, const float* __restrict__ lnl_new,
                                                     const float* __restrict__ g_new, const float* __restrict__ F_new, long long n,
                                                     int din, int first, double xtol, int* __restrict__ active) {
  constexpr int NI = kFitMaxIn;
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  FitRow& s = st[row];
  if (s.status >= 0) return;
  float* u = up + row * din;
  double lam = s.lam;
  const float ln = lnl_new[row];
  if (!first) s.iters += 1;
  if (first || ln > s.p.lnl) {
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
#pragma unroll
  for (int i = 0, p = 0; i < NI; p += NI - i, ++i)
    if (i < din && F[p] != 0.0) info = true;
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

}  // namespace v21
