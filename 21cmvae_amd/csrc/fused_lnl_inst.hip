// fused_lnl_inst.hip -- one translation unit per (architecture, precision) of the ln L variant of the fused forward
// kernel (fused_fwd.h: the traits with LNL); compiled with -DV21_ARCH=S1 -DV21_PREC=F16x2spLnl etc. (see Makefile).
#include "fused_fwd.h"
#include "archs.h"

#define V21_CAT3(a, b, c) a##b##c
#define V21_SYMNAME(a, p) V21_CAT3(launch_lnl_, a, _##p)
#define V21_XCAT(a, b) a##b
#define V21_ARCH_T(a) V21_XCAT(Arch, a)
#define V21_PREC_T(p) V21_XCAT(Prec, p)
#define V21_EXPAND_SYM(a, p) V21_SYMNAME(a, p)

namespace v21 {

hipError_t V21_EXPAND_SYM(V21_ARCH, V21_PREC)(const FusedArgs& a, hipStream_t st) {
  using A = V21_ARCH_T(V21_ARCH);
  using P = V21_PREC_T(V21_PREC);
  static_assert(lnl_of<P>::value, "fused_lnl_inst.hip instantiates the ln L variants only");
  auto kern = fused_fwd<A, P>;
  static bool attr_done_dev[64] = {};  // the attribute belongs to (function, device)
  int dev = 0;
  (void)hipGetDevice(&dev);
  bool& attr_done = attr_done_dev[dev & 63];
  if (!attr_done) {
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, fused_lds_alloc<P>());
    if (e != hipSuccess) return e;
    attr_done = true;
  }
  constexpr int rows = P::WAVES * P::CT * 32;
  const long long nwg = (a.n_rows + rows - 1) / rows;
  if (nwg <= 0) return hipSuccess;
  hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(64 * P::WAVES), fused_lds_alloc<P>(), st, a);
  return hipGetLastError();
}

}  // namespace v21
