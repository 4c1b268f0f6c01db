// reduce_kernels.h -- the one reduction of a slice of rows' y and Jacobian (left in the likelihood workspace by the
// Jacobian kernels: fused_jac.h / jac_generic.h, Jacobian mode) to what leaves the device (api_jacobian.hip: reduce_run):
//   jac_reduce_kernel<NI, NK, FISHER>  per row ln L, its gradient, F = J W J^T (W = diag(inv_var); FISHER) and, with a
//                                      nuisance record (NK > 0; nuisance_kernels.h has the mathematics), their marginalised
//                                      forms and the sums b.
// Every consumer -- loglike on the fused route, fisher, fit, sample, the nuisance amplitudes -- is an instantiation of it.
#pragma once
#include <hip/hip_runtime.h>

namespace v21 {

// the nuisance sums of one lane: b = Q W r (nk) and B = Q W J^T (nk, din); nothing without a nuisance record
template <int NI, int NK>
struct NuisSums { float b[NK] = {}, B[NK][NI] = {}; };
template <int NI>
struct NuisSums<NI, 0> {};

// one wave per row (block 256 = 4 rows, grid ceil(n_rows / 4)), bins on the lanes (coalesced rows of jac), w == 0 bins
// skipped (whatever d holds there), shuffle reductions: no LDS, no barrier.  y: (n_rows, dout), jac: (n_rows, din, dout)
// of one slice whose first row is row0 of the call; row row0 + n reads data row (row0 + n) / rows_per_data of pitch
// ld_data (ld_data = 0: one shared record); data is read only for lnl / grad / bout (all nullable).
//   lnl[n] = -1/2 sum_k w_k r_k^2,  grad[n, j] = sum_k w_k r_k jac[n, j, k]  (r = d - y),
//   fisher[n, i, j] = sum_k w_k jac[n, i, k] jac[n, j, k]  (din x din, both triangles from one accumulator).
// NI: the largest din of the instantiation (8 or kJacMaxIn of routes.h); FISHER: F is formed (without it NI (NI + 1) / 2
// accumulators fewer: the log-likelihood entry).  NK: the largest nk (0, 4 or 8).  NK == 0: no nuisance record, q and
// bout are not read and lane 0 stores the float32 sums.  NK > 0: q (nk, dout) float32 is read from global memory (its
// 4 nk dout <= 14 KB stay in the vector cache for the four rows of a workgroup, and staging them in LDS would read as
// much per workgroup and add a barrier); B is summed only when F or the gradient is asked for; lane 0 forms F - B^T B,
// g - B^T b and lp - |b|^2 in float64 from the reduced float32 sums and rounds once; bout (n_rows, nk) = b.
template <int NI, int NK, bool FISHER>
__global__ void __launch_bounds__(256) jac_reduce_kernel(const float* __restrict__ y, const float* __restrict__ jac,
                                                         const float* __restrict__ data, long long ld_data, long long rows_per_data,
                                                         long long row0, const float* __restrict__ wv, const float* __restrict__ q, int nk,
                                                         float* __restrict__ fisher, float* __restrict__ lnl, float* __restrict__ grad,
                                                         float* __restrict__ bout, long long n_rows, int din, int dout) {
  constexpr int NP = FISHER ? NI * (NI + 1) / 2 : 1;
  // F and B use every Jacobian element more than once: a bin's column is loaded and weighted up front.  The gradient
  // alone uses each once, and reads it where it is used (NI registers fewer: the log-likelihood entry's occupancy)
  constexpr bool COLUMN = FISHER || NK > 0;
  const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (n >= n_rows) return;  // (whole waves: the shuffles below run with every lane of a live wave)
  const bool like = lnl || grad || (NK > 0 && bout);
  const bool need_B = FISHER || grad;  // (uniform: ln L and b alone do not read B)
  const float* d = like ? data + ((row0 + n) / rows_per_data) * ld_data : nullptr;
  float fp[NP] = {}, lp = 0.f, gp[NI] = {};
  NuisSums<NI, NK> ns;
  for (int k = lane; k < dout; k += 64) {
    const float w = wv[k];
    if (w == 0.f) continue;
    float jk[NI], wj[NI];
    if constexpr (COLUMN) {
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        jk[j] = j < din ? jac[(n * din + j) * dout + k] : 0.f;
        wj[j] = w * jk[j];
      }
    }
    float qk[NK > 0 ? NK : 1];
    if constexpr (NK > 0) {
#pragma unroll
      for (int m = 0; m < NK; ++m) qk[m] = m < nk ? q[(long long)m * dout + k] : 0.f;
    }
    if constexpr (FISHER) {
      int p = 0;
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = i; j < NI; ++j, ++p)
          if (j < din) fp[p] += wj[i] * jk[j];
    }
    if constexpr (NK > 0) {
      if (need_B) {
#pragma unroll
        for (int m = 0; m < NK; ++m)
#pragma unroll
          for (int j = 0; j < NI; ++j)
            if (m < nk && j < din) ns.B[m][j] += qk[m] * wj[j];
      }
    }
    if (like) {
      const float r = d[k] - y[n * dout + k], wr = w * r;
      lp += wr * r;
#pragma unroll
      for (int j = 0; j < NI; ++j)
        if (j < din) gp[j] += wr * (COLUMN ? jk[j] : jac[(n * din + j) * dout + k]);
      if constexpr (NK > 0) {
#pragma unroll
        for (int m = 0; m < NK; ++m)
          if (m < nk) ns.b[m] += qk[m] * wr;
      }
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
    if constexpr (NK > 0) {
      if (need_B) {
#pragma unroll
        for (int m = 0; m < NK; ++m)
#pragma unroll
          for (int j = 0; j < NI; ++j)
            if (m < nk && j < din) ns.B[m][j] += __shfl_xor(ns.B[m][j], o);
      }
    }
    if (like) {
      lp += __shfl_xor(lp, o);
#pragma unroll
      for (int j = 0; j < NI; ++j)
        if (j < din) gp[j] += __shfl_xor(gp[j], o);
      if constexpr (NK > 0) {
#pragma unroll
        for (int m = 0; m < NK; ++m)
          if (m < nk) ns.b[m] += __shfl_xor(ns.b[m], o);
      }
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
          float v = fp[p];
          if constexpr (NK > 0) {
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < NK; ++m)
              if (m < nk) s += (double)ns.B[m][i] * (double)ns.B[m][j];
            v = (float)((double)fp[p] - s);
          }
          F[i * din + j] = v;
          F[j * din + i] = v;
        }
  }
  if (lnl) {
    if constexpr (NK > 0) {
      double s = 0.0;
#pragma unroll
      for (int m = 0; m < NK; ++m)
        if (m < nk) s += (double)ns.b[m] * (double)ns.b[m];
      lnl[n] = (float)(-0.5 * ((double)lp - s));
    } else {
      lnl[n] = -0.5f * lp;
    }
  }
  if (grad)
#pragma unroll
    for (int j = 0; j < NI; ++j)
      if (j < din) {
        float v = gp[j];
        if constexpr (NK > 0) {
          double s = 0.0;
#pragma unroll
          for (int m = 0; m < NK; ++m)
            if (m < nk) s += (double)ns.B[m][j] * (double)ns.b[m];
          v = (float)((double)gp[j] - s);
        }
        grad[n * din + j] = v;
      }
  if constexpr (NK > 0) {
    if (bout)
#pragma unroll
      for (int m = 0; m < NK; ++m)
        if (m < nk) bout[n * nk + m] = ns.b[m];
  }
}

// The forward-only sibling (api_loglike.hip, the two-launch route): ln L of rows of y alone -- no Jacobian is read or
// exists.  The same lanes, bins, skip of w == 0 bins, arithmetic and shuffle order as jac_reduce_kernel's ln L, so that
// on equal y both give equal bits; with a nuisance record (NK > 0) lnl = -1/2 (r^T W r - b^T b) from the stored Q, the
// float32 sums combined in float64 and rounded once.  y: (n_rows, ldy) of one slice whose first row is row0 of the call.
template <int NK>
__global__ void __launch_bounds__(256) lnl_reduce_kernel(const float* __restrict__ y, long long ldy, const float* __restrict__ data,
                                                         long long ld_data, long long rows_per_data, long long row0,
                                                         const float* __restrict__ wv, const float* __restrict__ q, int nk,
                                                         float* __restrict__ lnl, long long n_rows, int dout) {
  const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (n >= n_rows) return;  // (whole waves)
  const float* d = data + ((row0 + n) / rows_per_data) * ld_data;
  float lp = 0.f;
  NuisSums<1, NK> ns;
  for (int k = lane; k < dout; k += 64) {
    const float w = wv[k];
    if (w == 0.f) continue;
    const float r = d[k] - y[n * ldy + k], wr = w * r;
    lp += wr * r;
    if constexpr (NK > 0) {
#pragma unroll
      for (int m = 0; m < NK; ++m)
        if (m < nk) ns.b[m] += q[(long long)m * dout + k] * wr;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    lp += __shfl_xor(lp, o);
    if constexpr (NK > 0) {
#pragma unroll
      for (int m = 0; m < NK; ++m)
        if (m < nk) ns.b[m] += __shfl_xor(ns.b[m], o);
    }
  }
  if (lane != 0) return;
  if constexpr (NK > 0) {
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < NK; ++m)
      if (m < nk) s += (double)ns.b[m] * (double)ns.b[m];
    lnl[n] = (float)(-0.5 * ((double)lp - s));
  } else {
    lnl[n] = -0.5f * lp;
  }
}

}  // namespace v21
