// nuisance_kernels.h -- linear nuisance (foreground) modes marginalised inside the reductions of the likelihood record
// (api_jacobian.hip: v21_mlp_set_nuisance; include/v21.h has the mathematics).  With Q the (K, out) basis orthonormalised
// under W = diag(w) (Q W Q^T = I_K), r = d - y, b = Q W r and B = Q W J^T:
//     ln L_m = -1/2 (r^T W r - |b|^2),   g_m = J W r - B^T b,   F_m = J W J^T - B^T B.
//   jac_marg_kernel      jac_fisher_kernel (fit_kernels.h) with the K + K in_dim extra sums b and B: F_m (optional), ln L_m
//                        and g_m of every row, and optionally b itself (the amplitudes are R^-1 (b + Q W d_raw));
//   nuis_project_kernel  d~ = d - Q^T (Q W d) of every row of a (n_data, out) data matrix, float64 sums, rounded to float32
//                        once: float32 cannot form r^T W r - |b|^2 from data that carry a foreground 10^4 times the signal,
//                        and W - W Q^T Q W annihilates whatever the projection removes, so the results do not change.
#pragma once
#include <hip/hip_runtime.h>

namespace v21 {

constexpr int kNuisMaxModes = 8;

// one wave per row (block 256 = 4 rows, grid ceil(n_rows / 4)), bins on the lanes, w == 0 bins skipped, shuffle
// reductions, no LDS and no barrier: jac_fisher_kernel's decomposition and its arguments, plus q (nk, dout) float32 and
// bout (n_rows, nk; nullable).  Q is read from global memory: its 4 nk dout <= 14 KB stay in the vector cache for the
// four rows of a workgroup, and staging them in LDS would read as much per workgroup and add a barrier.  NI / NK: the
// largest din / nk of the instantiation; FISHER: F is formed (without it NI (NI + 1) / 2 accumulators fewer: the
// log-likelihood entry; B is summed only when F or the gradient is asked for).  Lane 0 forms F - B^T B, g - B^T b and
// lp - |b|^2 in float64 from the reduced float32 sums and rounds once; both triangles of F come from one value.  data
// is read only for lnl / grad / bout.
template <int NI, int NK, bool FISHER>
__global__ void __launch_bounds__(256) jac_marg_kernel(const float* __restrict__ y, const float* __restrict__ jac,
                                                       const float* __restrict__ data, long long ld_data, long long rows_per_data,
                                                       long long row0, const float* __restrict__ wv, const float* __restrict__ q, int nk,
                                                       float* __restrict__ fisher, float* __restrict__ lnl, float* __restrict__ grad,
                                                       float* __restrict__ bout, long long n_rows, int din, int dout) {
  constexpr int NP = FISHER ? NI * (NI + 1) / 2 : 1;
  const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (n >= n_rows) return;  // (whole waves: the shuffles below run with every lane of a live wave)
  const bool like = lnl || grad || bout;
  const bool need_B = FISHER || grad;  // (uniform: ln L and b alone do not read B)
  const float* d = like ? data + ((row0 + n) / rows_per_data) * ld_data : nullptr;
  float fp[NP] = {}, lp = 0.f, gp[NI] = {}, bp[NK] = {}, Bp[NK][NI] = {};
  for (int k = lane; k < dout; k += 64) {
    const float w = wv[k];
    if (w == 0.f) continue;
    float jk[NI], wj[NI], qk[NK];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      jk[j] = j < din ? jac[(n * din + j) * dout + k] : 0.f;
      wj[j] = w * jk[j];
    }
#pragma unroll
    for (int m = 0; m < NK; ++m) qk[m] = m < nk ? q[(long long)m * dout + k] : 0.f;
    if constexpr (FISHER) {
      int p = 0;
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = i; j < NI; ++j, ++p)
          if (j < din) fp[p] += wj[i] * jk[j];
    }
    if (need_B) {
#pragma unroll
      for (int m = 0; m < NK; ++m)
#pragma unroll
        for (int j = 0; j < NI; ++j)
          if (m < nk && j < din) Bp[m][j] += qk[m] * wj[j];
    }
    if (like) {
      const float r = d[k] - y[n * dout + k], wr = w * r;
      lp += wr * r;
#pragma unroll
      for (int j = 0; j < NI; ++j)
        if (j < din) gp[j] += wr * jk[j];
#pragma unroll
      for (int m = 0; m < NK; ++m)
        if (m < nk) bp[m] += qk[m] * wr;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    if constexpr (FISHER) {
      int p = 0;
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = i; j < NI; ++j, ++p)
          if (j < din) fp[p] += __shfl_xor(fp[p], o);
    }
    if (need_B) {
#pragma unroll
      for (int m = 0; m < NK; ++m)
#pragma unroll
        for (int j = 0; j < NI; ++j)
          if (m < nk && j < din) Bp[m][j] += __shfl_xor(Bp[m][j], o);
    }
    if (like) {
      lp += __shfl_xor(lp, o);
#pragma unroll
      for (int j = 0; j < NI; ++j)
        if (j < din) gp[j] += __shfl_xor(gp[j], o);
#pragma unroll
      for (int m = 0; m < NK; ++m)
        if (m < nk) bp[m] += __shfl_xor(bp[m], o);
    }
  }
  if (lane != 0) return;
  if constexpr (FISHER) {
    float* F = fisher + n * din * din;
    int p = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = i; j < NI; ++j, ++p)
        if (j < din) {
          double s = 0.0;
#pragma unroll
          for (int m = 0; m < NK; ++m)
            if (m < nk) s += (double)Bp[m][i] * (double)Bp[m][j];
          const float v = (float)((double)fp[p] - s);
          F[i * din + j] = v;
          F[j * din + i] = v;
        }
  }
  if (lnl) {
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < NK; ++m)
      if (m < nk) s += (double)bp[m] * (double)bp[m];
    lnl[n] = (float)(-0.5 * ((double)lp - s));
  }
  if (grad)
#pragma unroll
    for (int j = 0; j < NI; ++j)
      if (j < din) {
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < NK; ++m)
          if (m < nk) s += (double)Bp[m][j] * (double)bp[m];
        grad[n * din + j] = (float)((double)gp[j] - s);
      }
  if (bout)
#pragma unroll
    for (int m = 0; m < NK; ++m)
      if (m < nk) bout[n * nk + m] = bp[m];
}

// one wave per data row (block 256 = 4 rows, grid ceil(n_data / 4)): c = Q W d (nk float64 sums over the bins with
// w > 0, reduced by shuffles), then out[k] = float32(d[k] - sum_m q[m, k] c[m]) (Q is zero where w == 0: those bins pass
// through).  q: (nk, dout) float64; data / out: (n_data, dout).
static __global__ void __launch_bounds__(256) nuis_project_kernel(const float* __restrict__ data, const float* __restrict__ wv,
                                                                  const double* __restrict__ q, int nk, float* __restrict__ out,
                                                                  long long n_data, int dout) {
  const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (n >= n_data) return;
  const float* d = data + n * dout;
  double c[kNuisMaxModes] = {};
  for (int k = lane; k < dout; k += 64) {
    if (wv[k] == 0.f) continue;  // (whatever d holds there)
    const double wd = (double)wv[k] * (double)d[k];
#pragma unroll
    for (int m = 0; m < kNuisMaxModes; ++m)
      if (m < nk) c[m] += q[(long long)m * dout + k] * wd;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
    for (int m = 0; m < kNuisMaxModes; ++m)
      if (m < nk) c[m] += __shfl_xor(c[m], o);
  for (int k = lane; k < dout; k += 64) {
    double v = (double)d[k];
#pragma unroll
    for (int m = 0; m < kNuisMaxModes; ++m)
      if (m < nk) v -= q[(long long)m * dout + k] * c[m];
    out[n * dout + k] = (float)v;
  }
}

}  // namespace v21
