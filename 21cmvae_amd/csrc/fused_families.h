// fused_families.h -- the five families of fused kernels, each described once: the argument block, the kernel template,
// its dynamic LDS, the threads of a workgroup, the rows a workgroup covers and the workgroups of a call.  fused_inst.hip
// makes the compiled kernels' launchers from these traits (launch<>, below); jit.hip takes the geometry of the run-time
// kernels from the same traits.  Host code only: this file is NOT among the sources embedded for hiprtc (Makefile:
// JIT_SRC / JIT_TRAIN_SRC) and none of those includes it.  Reading a family's geometry instantiates no kernel;
// kernel<A, P>() does.
#pragma once
#include "fused_jac.h"
#include "fused_train16.h"

namespace v21 {

// fused_fwd<A, P>: each of the P::WAVES waves takes P::CT column tiles of 32 rows
struct FamilyFwd {
  using Args = FusedArgs;
  template <class A, class P> static auto kernel() { return fused_fwd<A, P>; }
  template <class P> static constexpr int lds() { return fused_lds_alloc<P>(); }
  template <class P> static constexpr int threads() { return 64 * P::WAVES; }
  template <class P> static constexpr int rows_per_wg() { return P::WAVES * P::CT * 32; }
  template <class A> static long long rows(const Args& a) { return a.n_rows; }
  template <class P> static constexpr long long workgroups(long long rows) { return (rows + rows_per_wg<P>() - 1) / rows_per_wg<P>(); }
};
// its ln L variant: the same kernel on the traits with LNL
struct FamilyLnl : FamilyFwd {
  template <class P> static constexpr long long workgroups(long long rows) {
    static_assert(lnl_of<P>::value, "the ln L family instantiates the ln L variants only");
    return FamilyFwd::workgroups<P>(rows);
  }
};
// fused_jac<A, P>: the forward's geometry over jac_group virtual rows per row of the call, without the stamp area
struct FamilyJac : FamilyFwd {
  using Args = JacArgs;
  template <class A, class P> static auto kernel() { return fused_jac<A, P>; }
  template <class P> static constexpr int lds() { return fused_lds<P>(); }
  template <class A> static long long rows(const Args& a) { return a.n_rows * jac_group<A::dims[0]>(); }
};
// the training kernels: whole rounds of the 8 XCDs (the kernels map block numbers XCD-major and the surplus leaves)
template <int ROWS_PER_WG>
struct FamilyTrainGeometry {
  using Args = ChainArgs;
  template <class P> static constexpr int threads() { return 64 * P::WAVES; }
  template <class P> static constexpr int rows_per_wg() { return ROWS_PER_WG; }
  template <class A> static long long rows(const Args& a) { return a.rows; }
  template <class P> static constexpr long long workgroups(long long rows) { return ((rows + ROWS_PER_WG - 1) / ROWS_PER_WG + 7) / 8 * 8; }
};
struct FamilyTrain : FamilyTrainGeometry<kTrainRowsPerWg> {
  template <class A, class P> static auto kernel() { return fused_train<A, P>; }
  template <class P> static constexpr int lds() { return fused_train_lds<P>(); }
};
struct FamilyTrain16 : FamilyTrainGeometry<kTrain16RowsPerWg> {
  template <class A, class P> static auto kernel() { return fused_train16<A, P>; }
  template <class P> static constexpr int lds() { return fused_train16_lds<P>(); }
};

// One launch of family F's compiled kernel for (stack A, precision form P).  More than 64 KB of dynamic LDS needs the
// attribute, and the attribute belongs to (function, device): one process may drive several devices.
template <class F, class A, class P>
hipError_t launch(const typename F::Args& a, hipStream_t st) {
  auto kern = F::template kernel<A, P>();
  constexpr int lds = F::template lds<P>();
  static bool attr_done_dev[64] = {};
  int dev = 0;
  (void)hipGetDevice(&dev);
  bool& attr_done = attr_done_dev[dev & 63];
  if (!attr_done) {
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
    attr_done = true;
  }
  const long long nwg = F::template workgroups<P>(F::template rows<A>(a));
  if (nwg <= 0) return hipSuccess;
  hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(F::template threads<P>()), lds, st, a);
  return hipGetLastError();
}

}  // namespace v21
