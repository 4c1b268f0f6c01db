// nuisance_kernels.h -- linear nuisance (foreground) modes marginalised inside the reductions of the likelihood record
// (api_jacobian.hip: v21_mlp_set_nuisance; include/v21.h has the mathematics).  With Q the (K, out) basis orthonormalised
// under W = diag(w) (Q W Q^T = I_K), r = d - y, b = Q W r and B = Q W J^T:
//     ln L_m = -1/2 (r^T W r - |b|^2),   g_m = J W r - B^T b,   F_m = J W J^T - B^T B.
// The sums b and B and the float64 subtractions are jac_reduce_kernel's (reduce_kernels.h, NK > 0).  Here:
//   nuis_project_kernel  d~ = d - Q^T (Q W d) of every row of a (n_data, out) data matrix, float64 sums, rounded to float32
//                        once: float32 cannot form r^T W r - |b|^2 from data that carry a foreground 10^4 times the signal,
//                        and W - W Q^T Q W annihilates whatever the projection removes, so the results do not change.
#pragma once
#include <hip/hip_runtime.h>

namespace v21 {

constexpr int kNuisMaxModes = 8;

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
