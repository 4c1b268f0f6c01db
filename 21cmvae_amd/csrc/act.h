// act.h -- the hidden-layer activations beside ReLU and linear (include/v21.h: V21_ACT_TANH .. V21_ACT_SOFTPLUS), with
// Keras' definitions (the reference's `activation_func`, emulator.py:12-48: "str or instance of tf.keras.activations"):
//
//   code  name      h = act(z)              dh/dz from the stored output h     dh/dz from z (act_deriv_in)
//   3     tanh      tanh z                  1 - h^2                            4 e / (1 + e)^2, e = exp(-2|z|)
//   4     sigmoid   1 / (1 + exp(-z))       h (1 - h)                          e / (1 + e)^2,   e = exp(-|z|)
//   5     elu       z > 0 ? z : exp(z) - 1  h > 0 ? 1 : h + 1                  z > 0 ? 1 : exp(z)       (alpha = 1)
//   6     softplus  ln(1 + exp(z))          1 - exp(-h)                        sigmoid(z)
//
// All four derivatives are functions of the OUTPUT: the per-layer trainer keeps h, not z (gemm_nt.h: NT_DX_ACT reads the
// array NT_DX_MASK reads).  Where z is in a register (jac_generic.h) the derivative is taken from z: 1 - h^2 loses every
// digit once h has rounded to +-1, 4 e / (1 + e)^2 keeps them down to the underflow of e.
//
// No formula overflows or produces a NaN for any finite z: every exponential has a non-positive argument (e in (0, 1];
// an underflow to 0 gives the saturated value itself: tanh = +-1, sigmoid = 0 or 1, elu = -1, softplus = max(z, 0)).
// A naive tanh = (e^z - e^-z) / (e^z + e^-z) is inf / inf from |z| = 89 on.
//
// Arithmetic: f32 throughout.  The device functions are the ROCm device library's expf, expm1f and log1pf (OCML:
// documented at 1 ulp each; the OpenCL bounds they are built to are 3, 3 and 2 ulp), never the __expf / __logf fast
// forms; the quotients are IEEE f32 divisions (the library builds without fast-math).  On top of the exponential's
// error a result carries 2-3 roundings: tanh and sigmoid <= ~4 ulp, softplus <= ~3 ulp, elu <= ~2 ulp.
// Codes 0 and 1 are NOT served here: linear and ReLU keep their own epilogues (bit masks and max), untouched.
// (Embedded, with fused_fwd.h, in the sources jit.hip hands to hiprtc: no #include "..." of its own.)
#pragma once
#ifndef __HIPCC_RTC__  // (hiprtc brings its own runtime header)
#include <hip/hip_runtime.h>
#endif

namespace v21 {

constexpr int kActLinear = 0, kActRelu = 1, kActGauss = 2, kActTanh = 3, kActSigmoid = 4, kActElu = 5, kActSoftplus = 6;
// a code of this file (host and device)
__host__ __device__ constexpr bool act_is_smooth(int code) { return code >= kActTanh && code <= kActSoftplus; }
inline const char* act_name(int code) {
  const char* names[] = {"linear", "relu", "gauss", "tanh", "sigmoid", "elu", "softplus"};
  return code >= 0 && code <= kActSoftplus ? names[code] : "?";
}

template <int CODE>
__device__ __forceinline__ float act_apply(float z) {
  static_assert(CODE >= kActTanh && CODE <= kActSoftplus, "act_apply: codes 3 .. 6 (linear and ReLU keep their own epilogues)");
  if constexpr (CODE == kActTanh) {
    const float e = expf(-2.f * fabsf(z));  // (0, 1]
    return copysignf((1.f - e) / (1.f + e), z);
  } else if constexpr (CODE == kActSigmoid) {
    const float e = expf(-fabsf(z));        // (0, 1]
    const float d = 1.f / (1.f + e);                            // sigmoid(|z|) in [0.5, 1)
    return z >= 0.f ? d : e * d;
  } else if constexpr (CODE == kActElu) {
    return z > 0.f ? z : expm1f(z);                   // (z <= 0: expm1 in (-1, 0])
  } else {
    return fmaxf(z, 0.f) + log1pf(expf(-fabsf(z)));
  }
}
// dh/dz from the stored output h = act(z)
template <int CODE>
__device__ __forceinline__ float act_deriv_out(float h) {
  static_assert(CODE >= kActTanh && CODE <= kActSoftplus, "act_deriv_out: codes 3 .. 6");
  if constexpr (CODE == kActTanh) return 1.f - h * h;
  else if constexpr (CODE == kActSigmoid) return h * (1.f - h);
  else if constexpr (CODE == kActElu) return h > 0.f ? 1.f : h + 1.f;
  else return -expm1f(-h);                            // 1 - exp(-h), h >= 0: in [0, 1)
}
// dh/dz from z itself (jac_generic.h)
template <int CODE>
__device__ __forceinline__ float act_deriv_in(float z) {
  static_assert(CODE >= kActTanh && CODE <= kActSoftplus, "act_deriv_in: codes 3 .. 6");
  if constexpr (CODE == kActTanh) {
    const float e = expf(-2.f * fabsf(z)), d = 1.f + e;
    return 4.f * e / (d * d);
  } else if constexpr (CODE == kActSigmoid) {
    const float e = expf(-fabsf(z)), d = 1.f + e;
    return e / (d * d);
  } else if constexpr (CODE == kActElu) {
    return z > 0.f ? 1.f : expf(z);
  } else {
    return act_apply<kActSigmoid>(z);
  }
}

// ---- the same by a run-time code, for the table-driven sites (gemm.h, gemm_nt.h, jac_generic.h).  The code is uniform
// over a launch's problem: a scalar branch, no divergence.  Any other code: the identity / 1.
__device__ __forceinline__ float act_apply_rt(int code, float z) {
  switch (code) {
    case kActTanh: return act_apply<kActTanh>(z);
    case kActSigmoid: return act_apply<kActSigmoid>(z);
    case kActElu: return act_apply<kActElu>(z);
    case kActSoftplus: return act_apply<kActSoftplus>(z);
  }
  return z;
}
__device__ __forceinline__ float act_deriv_out_rt(int code, float h) {
  switch (code) {
    case kActTanh: return act_deriv_out<kActTanh>(h);
    case kActSigmoid: return act_deriv_out<kActSigmoid>(h);
    case kActElu: return act_deriv_out<kActElu>(h);
    case kActSoftplus: return act_deriv_out<kActSoftplus>(h);
  }
  return 1.f;
}
__device__ __forceinline__ float act_deriv_in_rt(int code, float z) {
  switch (code) {
    case kActTanh: return act_deriv_in<kActTanh>(z);
    case kActSigmoid: return act_deriv_in<kActSigmoid>(z);
    case kActElu: return act_deriv_in<kActElu>(z);
    case kActSoftplus: return act_deriv_in<kActSoftplus>(z);
  }
  return 1.f;
}

}  // namespace v21
