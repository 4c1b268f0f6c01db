// compiled.h -- the registry of the fused kernels compiled into the library: which stacks (archs.h) and precision forms
// each family has, the launchers' names, and the two tables the api units launch through.  The launchers are defined
// by fused_inst.hip, one object per (family, stack, precision form): a form listed here without its object in the
// Makefile -- or with another argument block than fused_families.h gives its family -- does not link.  Declarations
// only: the api units do not see the kernel templates.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "archs.h"

namespace v21 {
struct FusedArgs;  // fused_fwd.h
struct JacArgs;    // fused_jac.h
struct ChainArgs;  // chain_types.h
template <class Args> using launcher = hipError_t (*)(const Args&, hipStream_t);

// the launcher of (family f, stack a, precision form p): FamilyFwd, ArchS1, PrecF16x2sp -> launch_Fwd_S1_F16x2sp
#define V21_LAUNCHER(f, a, p) launch_##f##_##a##_##p
#define V21_ARGS_Fwd FusedArgs
#define V21_ARGS_Lnl FusedArgs
#define V21_ARGS_Jac JacArgs
#define V21_ARGS_Train ChainArgs
#define V21_ARGS_Train16 ChainArgs
// The precision forms of each family, in the order of a table row.  Inference: V21_PREC_F32, F16, BF16 -- f32 is one
// wave per SIMD on the exact f32 MFMA; f16 / bf16 are two workgroups per CU, one column tile per wave, the ring refill
// spread over the block being consumed (fused_fwd.h: "x2sp").  Training: f16, bf16.
#define V21_FWD_FORMS(X, a) X(Fwd, a, F32) X(Fwd, a, F16x2sp) X(Fwd, a, BF16x2sp)
#define V21_LNL_FORMS(X, a) X(Lnl, a, F32Lnl) X(Lnl, a, F16x2spLnl) X(Lnl, a, BF16x2spLnl)
#define V21_JAC_FORMS(X, a) X(Jac, a, F32) X(Jac, a, F16x2sp) X(Jac, a, BF16x2sp)
#define V21_TRAIN_FORMS(X, a) X(Train, a, F16t) X(Train, a, BF16t)
#define V21_TRAIN16_FORMS(X, a) X(Train16, a, F16t16) X(Train16, a, BF16t16)

#define V21_DECL(f, a, p) hipError_t V21_LAUNCHER(f, a, p)(const V21_ARGS_##f&, hipStream_t);
#define V21_NAME(f, a, p) V21_LAUNCHER(f, a, p),
#define V21_INFER_DECL(a) V21_FWD_FORMS(V21_DECL, a) V21_LNL_FORMS(V21_DECL, a) V21_JAC_FORMS(V21_DECL, a)
#define V21_TRAIN_DECL(a) V21_TRAIN_FORMS(V21_DECL, a) V21_TRAIN16_FORMS(V21_DECL, a)
V21_ARCH_LIST(V21_INFER_DECL)
V21_TRAIN_ARCH_LIST(V21_TRAIN_DECL)
// the headline stack's 16-bit kernels with per-workgroup clock stamps (fused_fwd.h: CLOCK_STAMPS; v21_debug_forward_clocked)
V21_DECL(Fwd, S1, F16x2spClk)
V21_DECL(Fwd, S1, BF16x2spClk)

// a stack of V21_ARCH_LIST (v21_mlp::fused_id is its row): forward, ln L variant and Jacobian, per precision
struct InferEntry {
  int L;
  const int* dims;
  const int* act;
  launcher<FusedArgs> fwd[3], lnl[3];
  launcher<JacArgs> jac[3];
};
#define V21_INFER_ROW(a) \
  {Arch##a::L, Arch##a::dims, Arch##a::act, {V21_FWD_FORMS(V21_NAME, a)}, {V21_LNL_FORMS(V21_NAME, a)}, {V21_JAC_FORMS(V21_NAME, a)}},
inline const InferEntry g_infer[] = {V21_ARCH_LIST(V21_INFER_ROW)};
// a stack of V21_TRAIN_ARCH_LIST (TrainerKind::train_arch is its row): 32 and 16 rows per wave, per 16-bit precision
struct TrainEntry {
  int L;
  const int* dims;
  const int* act;
  launcher<ChainArgs> fn[2], fn16[2];
};
#define V21_TRAIN_ROW(a) {Arch##a::L, Arch##a::dims, Arch##a::act, {V21_TRAIN_FORMS(V21_NAME, a)}, {V21_TRAIN16_FORMS(V21_NAME, a)}},
inline const TrainEntry g_train[] = {V21_TRAIN_ARCH_LIST(V21_TRAIN_ROW)};
#undef V21_INFER_ROW
#undef V21_TRAIN_ROW
#undef V21_INFER_DECL
#undef V21_TRAIN_DECL
#undef V21_NAME
#undef V21_DECL

// the row of the stack (L, dims, act) in one of the tables, or -1
template <class Entry, size_t N>
int compiled_index(const Entry (&tab)[N], int L, const int* dims, const int* act) {
  for (size_t i = 0; i < N; ++i)
    if (tab[i].L == L && std::equal(dims, dims + L + 1, tab[i].dims) && std::equal(act, act + L, tab[i].act)) return (int)i;
  return -1;
}

}  // namespace v21
