// fused_inst.hip -- one translation unit per (family, stack, precision form) of the compiled fused kernels; compiled
// with -DV21_FAMILY=Fwd -DV21_ARCH=S1 -DV21_PREC=F16x2sp etc. (see Makefile).  It instantiates the family's kernel
// (fused_families.h) and defines the one launcher that compiled.h declares for it.
#include "compiled.h"
#include "fused_families.h"

#define V21_XCAT(a, b) a##b
#define V21_CAT(a, b) V21_XCAT(a, b)
#define V21_EXPAND_LAUNCHER(f, a, p) V21_LAUNCHER(f, a, p)

namespace v21 {

hipError_t V21_EXPAND_LAUNCHER(V21_FAMILY, V21_ARCH, V21_PREC)(const V21_CAT(Family, V21_FAMILY)::Args& a, hipStream_t st) {
  return launch<V21_CAT(Family, V21_FAMILY), V21_CAT(Arch, V21_ARCH), V21_CAT(Prec, V21_PREC)>(a, st);
}

}  // namespace v21
