// jac_generic.h -- the parameter Jacobian's kernels outside the fused route (api_jacobian.hip):
//   jac_prep_kernel     the input transform of every route (par_transform.h, the forward's own functions: the primal
//                       sees the bits the forward's prologue computes) and its chain-rule factor per (row, column);
//   jac_generic_kernel  primal + tangents of ANY stack (any hidden_dims and in_dim, > 512 wide, V21_ACT_GAUSS heads
//                       evaluated as z = z_mean like the deterministic forward, the activations of act.h) in f32 arithmetic.  One workgroup per
//                       (row, group of up to 7 tangents); the G columns of a layer's activation live in LDS, every
//                       output unit is one thread's k-ordered fmaf chain per column.  Correct, not fast: every
//                       workgroup streams the whole weight set through L2.
#pragma once
#include <hip/hip_runtime.h>

#include "act.h"
#include "par_transform.h"

namespace v21 {

// d par_transform / dx at the floored value t: 2 / span, times 1 / (t ln 10) for a log column (float64, rounded once)
__device__ __forceinline__ float par_transform_grad(double t, int lm, double span) {
  double d = 2.0 / span;
  if (lm) d /= t * 2.302585092994045684;
  return (float)d;
}

// one thread per (row, column): xt = the transformed f32 parameter (or the plain value), fac = its derivative (1)
template <class SRC>
__global__ void jac_prep_kernel(float* __restrict__ xt, float* __restrict__ fac, const SRC* __restrict__ src, long long lds_,
                                long long n, int din, int tin_on, const v21_affine_in t) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * din) return;
  const long long row = i / din;
  const int j = (int)(i % din);
  const SRC x = src[row * lds_ + j];
  if (!tin_on) {
    xt[i] = (float)x;
    fac[i] = 1.f;
    return;
  }
  if constexpr (sizeof(SRC) == 8) {
    xt[i] = par_transform_f64(x, t.log_mask[j], t.zero_floor[j], t.lo[j], t.span[j]);
    const double tf = (t.zero_floor[j] > 0.0 && x == 0.0) ? t.zero_floor[j] : (double)x;
    fac[i] = par_transform_grad(tf, t.log_mask[j], t.span[j]);
  } else {
    xt[i] = par_transform_f32(x, t.log_mask[j], t.zero_floor[j], t.lo[j], t.span[j]);
    const float tf = (t.zero_floor[j] > 0.0 && x == 0.f) ? (float)t.zero_floor[j] : x;
    fac[i] = par_transform_grad((double)tf, t.log_mask[j], t.span[j]);
  }
}

constexpr int kJacGenCols = 8;  // primal + up to 7 tangents per workgroup
struct JacGenArgs {
  int L, in_dim, tc, maxw;      // tc: tangents per workgroup (<= kJacGenCols - 1); maxw: LDS row pitch
  int dims[17], act[16], nw[16];
  long long w_off[16], b_off[16];
  const float* w;               // the stack's parameter arena
  const float* xt;              // (n, in_dim) transformed rows
  const float* fac;             // (n, in_dim)
  long long n_rows;
  float* y; long long ldy;      // nullable
  float* jac;                   // (n, in_dim, out) -- Jacobian mode
  float* lnl; float* grad;      // likelihood mode (grad nullable)
  const float* data; const float* wv;
  int like;
  float out_std;
  const float* mean;            // nullable: no output transform
};

// grid (n_rows, ceil(in_dim / tc)); block 256; dynamic LDS 2 * (tc + 1) * maxw floats.  ACT: the instantiation for stacks
// with an activation of act.h; every other stack keeps the code it had (ACT = false)
template <bool ACT>
__global__ void __launch_bounds__(256) jac_generic_kernel(const JacGenArgs a) {
  extern __shared__ float jsh[];
  const long long n = blockIdx.x;
  const int t0 = blockIdx.y * a.tc;
  const int C = 1 + min(a.tc, a.in_dim - t0);  // columns: primal + tangents t0 .. t0 + C - 2
  float* buf[2] = {jsh, jsh + (size_t)(a.tc + 1) * a.maxw};
  for (int i = threadIdx.x; i < C * a.in_dim; i += blockDim.x) {
    const int c = i / a.in_dim, k = i % a.in_dim;
    buf[0][c * a.maxw + k] = c == 0 ? a.xt[n * a.in_dim + k] : (k == t0 + c - 1 ? 1.f : 0.f);
  }
  __syncthreads();
  float lp = 0.f, gp[kJacGenCols] = {};
  int cur = 0;
  for (int l = 0; l < a.L; ++l) {
    const int K = a.dims[l], N = a.dims[l + 1], nw = a.nw[l];
    const float* W = a.w + a.w_off[l];  // V21_ACT_GAUSS: the z_mean columns only (z = z_mean)
    const float* b = a.w + a.b_off[l];
    const float* in = buf[cur];
    float* out = buf[cur ^ 1];
    const bool last = l == a.L - 1;
    for (int o = threadIdx.x; o < N; o += blockDim.x) {
      float s[kJacGenCols];
      s[0] = b[o];
#pragma unroll
      for (int c = 1; c < kJacGenCols; ++c) s[c] = 0.f;
      for (int k = 0; k < K; ++k) {
        const float wk = W[(long long)k * nw + o];
#pragma unroll
        for (int c = 0; c < kJacGenCols; ++c)
          if (c < C) s[c] = __builtin_fmaf(in[c * a.maxw + k], wk, s[c]);
      }
      // ReLU on every layer that has it, the output layer included (a stack may end in one: the engine's Dense and
      // the forward routes accept it); the primal's z > 0 masks primal and tangents together
      if (a.act[l] == V21_ACT_RELU && !(s[0] > 0.f)) {
#pragma unroll
        for (int c = 0; c < kJacGenCols; ++c) s[c] = 0.f;
      }
      // an activation of act.h: the primal through act_apply, the tangents times dh/dz taken from z itself (it is in a
      // register here; 1 - h^2 of a saturated unit has no digits left, 4 e / (1 + e)^2 has)
      if (ACT && act_is_smooth(a.act[l])) {
        const float d = act_deriv_in_rt(a.act[l], s[0]);
        s[0] = act_apply_rt(a.act[l], s[0]);
#pragma unroll
        for (int c = 1; c < kJacGenCols; ++c) s[c] *= d;
      }
      if (!last) {
#pragma unroll
        for (int c = 0; c < kJacGenCols; ++c)
          if (c < C) out[c * a.maxw + o] = s[c];
        continue;
      }
      const float yv = a.mean ? s[0] * a.out_std + a.mean[o] : s[0];
      if (!a.like) {
        if (a.y && blockIdx.y == 0) a.y[n * a.ldy + o] = yv;
#pragma unroll
        for (int c = 1; c < kJacGenCols; ++c)
          if (c < C) {
            const int j = t0 + c - 1;
            a.jac[(n * a.in_dim + j) * N + o] = s[c] * a.out_std * a.fac[n * a.in_dim + j];
          }
      } else if (a.wv[o] != 0.f) {
        const float r = a.data[o] - yv, wr = a.wv[o] * r;
        lp += wr * r;
#pragma unroll
        for (int c = 1; c < kJacGenCols; ++c)
          if (c < C) gp[c] += wr * (s[c] * a.out_std);
      }
    }
    __syncthreads();
    cur ^= 1;
  }
  if (!a.like) return;
  // block sums of lp and gp[1 ..] (the activation buffers are free now)
  float* red = jsh;
  for (int c = 0; c < C; ++c) {
    red[threadIdx.x] = c == 0 ? lp : gp[c];
    __syncthreads();
    for (int st = blockDim.x / 2; st > 0; st >>= 1) {
      if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      if (c == 0) { if (blockIdx.y == 0) a.lnl[n] = -0.5f * red[0]; }
      else if (a.grad) {
        const int j = t0 + c - 1;
        a.grad[n * a.in_dim + j] = red[0] * a.fac[n * a.in_dim + j];
      }
    }
    __syncthreads();
  }
}

}  // namespace v21
