// fit_kernels.h -- Fisher matrices and projected Levenberg-Marquardt fits on the device (api_fit.hip):
//   jac_fisher_kernel  F = J^T W J (W = diag(inv_var)) of every row, and optionally ln L and its gradient, from the y and
//                      J the Jacobian kernels (fused_jac.h / jac_generic.h, Jacobian mode) left in the likelihood
//                      workspace: jac_loglike_kernel's decomposition (one wave per row, bins on the lanes, shuffles).
//   fit_init_kernel    clamps the transformed start rows into the training box [-1, 1]^din and resets the row state;
//   fit_lm_kernel      one thread per row: accept / reject the evaluated proposal, then the next damped Gauss-Newton
//                      step, solved by a float64 Cholesky factorisation in registers;
//   fit_finish_kernel  the accepted point back to raw parameters (float64 inverse of par_transform) and the results.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/v21_types.h"

namespace v21 {

// one wave per row (block 256 = 4 rows, grid ceil(n_rows / 4)).  y: (n_rows, dout), jac: (n_rows, din, dout) of one
// slice whose first row is row0 of the call.  fisher[n, i, j] = sum_k w_k jac[n, i, k] jac[n, j, k] (din x din, both
// triangles from one accumulator); lnl / grad as jac_loglike_kernel (nullable; data is read only for them): row
// row0 + n reads data row (row0 + n) / rows_per_data of pitch ld_data (ld_data = 0: one shared record).  Bins with
// w == 0 are skipped.  NI: the largest din of the instantiation (8 or kFisherMaxIn), NI (NI + 1) / 2 accumulators.
constexpr int kFisherMaxIn = 15;  // (= kJacMaxIn of jac_generic.h: the fused Jacobian's limit)
template <int NI>
__global__ void __launch_bounds__(256) jac_fisher_kernel(const float* __restrict__ y, const float* __restrict__ jac,
                                                         const float* __restrict__ data, long long ld_data, long long rows_per_data,
                                                         long long row0, const float* __restrict__ wv, float* __restrict__ fisher,
                                                         float* __restrict__ lnl, float* __restrict__ grad, long long n_rows, int din,
                                                         int dout) {
  constexpr int NP = NI * (NI + 1) / 2;
  const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (n >= n_rows) return;  // (whole waves: the shuffles below run with every lane of a live wave)
  const bool like = lnl || grad;
  const float* d = like ? data + ((row0 + n) / rows_per_data) * ld_data : nullptr;
  float fp[NP] = {}, lp = 0.f, gp[NI] = {};
  for (int k = lane; k < dout; k += 64) {
    const float w = wv[k];
    if (w == 0.f) continue;
    float jk[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) jk[j] = j < din ? jac[(n * din + j) * dout + k] : 0.f;
    int p = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const float wj = w * jk[i];
#pragma unroll
      for (int j = i; j < NI; ++j, ++p)
        if (j < din) fp[p] += wj * jk[j];
    }
    if (like) {
      const float r = d[k] - y[n * dout + k], wr = w * r;
      lp += wr * r;
#pragma unroll
      for (int j = 0; j < NI; ++j)
        if (j < din) gp[j] += wr * jk[j];
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    int p = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = i; j < NI; ++j, ++p)
        if (j < din) fp[p] += __shfl_xor(fp[p], o);
    if (like) {
      lp += __shfl_xor(lp, o);
#pragma unroll
      for (int j = 0; j < NI; ++j)
        if (j < din) gp[j] += __shfl_xor(gp[j], o);
    }
  }
  if (lane != 0) return;
  float* F = fisher + n * din * din;
  int p = 0;
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = i; j < NI; ++j, ++p)
      if (j < din) {
        F[i * din + j] = fp[p];
        F[j * din + i] = fp[p];
      }
  if (lnl) lnl[n] = -0.5f * lp;
  if (grad)
#pragma unroll
    for (int j = 0; j < NI; ++j)
      if (j < din) grad[n * din + j] = gp[j];
}

// ---- fits: projected LM in the transformed coordinates u in [-1, 1]^din (the training box par_transform maps to)
constexpr int kFitMaxIn = 8;
constexpr double kFitLamMin = 1e-12, kFitLamMax = 1e12, kFitTiny = 1e-30;
// per-row state; status: -1 running, 0 iteration limit, 1 converged (||step||_inf <= xtol), 2 no improving step
// (lambda > kFitLamMax), 3 no information (every diag(F) == 0)
struct FitRow {
  float u[kFitMaxIn];            // accepted point
  float g[kFitMaxIn];            // gradient of ln L there (u coordinates)
  float F[kFitMaxIn * (kFitMaxIn + 1) / 2];  // Fisher matrix there, upper triangle by rows
  double lam;
  float lnl, lnl0;               // ln L at the accepted point and at the start
  int status;
  int iters;                     // accepted + rejected proposals evaluated after the start
};

// one thread per row: u_prop (pitch din, the rows the next evaluation reads) = clamp(xt, -1, 1), NaN -> -1 (a log
// column's non-positive raw value); fac = 1 (the evaluations run on u, without the input transform)
static __global__ void __launch_bounds__(256) fit_init_kernel(FitRow* __restrict__ st, float* __restrict__ up, float* __restrict__ fac,
                                                       long long n, int din, double lam0) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  for (int j = 0; j < din; ++j) {
    const float v = up[row * din + j];
    up[row * din + j] = v >= -1.f ? (v <= 1.f ? v : 1.f) : -1.f;
    fac[row * din + j] = 1.f;
  }
  FitRow& s = st[row];
  s.lam = lam0;
  s.lnl = 0.f;
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
  if (first || ln > s.lnl) {
    s.lnl = ln;
    if (first) s.lnl0 = ln;
    const float* Fn = F_new + row * din * din;
    int p = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      if (i < din) {
        s.u[i] = u[i];
        s.g[i] = g_new[row * din + i];
      }
#pragma unroll
      for (int j = i; j < NI; ++j, ++p)
        if (j < din) s.F[p] = Fn[i * din + j];
    }
    lam = fmax(lam / 10.0, kFitLamMin);
  } else {
    lam *= 10.0;
  }
  // the accepted point's Fisher matrix (float64), its diagonal, and the gradient
  double F[NI * (NI + 1) / 2], dg[NI], g[NI], ua[NI];
  bool info = false;
  {
    int p = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      g[i] = i < din ? (double)s.g[i] : 0.0;
      ua[i] = i < din ? (double)s.u[i] : 0.0;
#pragma unroll
      for (int j = i; j < NI; ++j, ++p) F[p] = j < din ? (double)s.F[p] : 0.0;
    }
  }
#pragma unroll
  for (int i = 0, p = 0; i < NI; p += NI - i, ++i) {
    dg[i] = F[p];
    if (i < din && F[p] != 0.0) info = true;
  }
  int status = -1;
  double delta[NI] = {};
  if (!info) {
    status = 3;
  } else {
    for (;;) {
      if (lam > kFitLamMax) { status = 2; break; }
      // Cholesky factor L (lower, by rows: L[i][j] at i (i + 1) / 2 + j) of A = F + lam diag(max(F_ii, tiny))
      double Lm[NI * (NI + 1) / 2];
      bool ok = true;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
          // A[i][j] = A[j][i]: the upper triangle's element (j, i)
          const int pu = j * NI - j * (j - 1) / 2 + (i - j);
          double sum = F[pu];
          if (i == j) sum += lam * fmax(dg[i], kFitTiny);
#pragma unroll
          for (int k = 0; k < j; ++k) sum -= Lm[i * (i + 1) / 2 + k] * Lm[j * (j + 1) / 2 + k];
          if (i == j) {
            if (i < din && !(sum > 0.0)) ok = false;
            Lm[i * (i + 1) / 2 + i] = i < din ? sqrt(sum) : 1.0;
          } else {
            Lm[i * (i + 1) / 2 + j] = i < din ? sum / Lm[j * (j + 1) / 2 + j] : 0.0;
          }
        }
      }
      if (!ok) { lam *= 10.0; continue; }
      double z[NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        double sum = g[i];
#pragma unroll
        for (int k = 0; k < i; ++k) sum -= Lm[i * (i + 1) / 2 + k] * z[k];
        z[i] = sum / Lm[i * (i + 1) / 2 + i];
      }
#pragma unroll
      for (int i = NI - 1; i >= 0; --i) {
        double sum = z[i];
#pragma unroll
        for (int k = i + 1; k < NI; ++k) sum -= Lm[k * (k + 1) / 2 + i] * delta[k];
        delta[i] = sum / Lm[i * (i + 1) / 2 + i];
      }
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
    if (i < din) u[i] = s.u[i];
}

// one thread per row: x_hat = the accepted point in raw units, float64 (lo + (u + 1) span / 2, then 10^ for a log column
// -- its lower bound comes back as 10^lo, e.g. the zero floor, never 0), and the per-row results (nullable)
template <class T>
__global__ void __launch_bounds__(256) fit_finish_kernel(const FitRow* __restrict__ st, T* __restrict__ x_hat, float* __restrict__ lnl,
                                  float* __restrict__ lnl0, int* __restrict__ status, long long n, int din, const v21_affine_in t) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const FitRow& s = st[row];
  for (int j = 0; j < din; ++j) {
    double v = t.lo[j] + ((double)s.u[j] + 1.0) * t.span[j] / 2.0;
    if (t.log_mask[j]) v = pow(10.0, v);
    x_hat[row * din + j] = (T)v;
  }
  if (lnl) lnl[row] = s.lnl;
  if (lnl0) lnl0[row] = s.lnl0;
  if (status) status[row] = s.status < 0 ? 0 : s.status;
}

}  // namespace v21
