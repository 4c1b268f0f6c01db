// routes.h -- WHICH kernels a call takes and in WHAT SHAPE a training launch goes out, decided in ONE place (r5).
//
// The library has several kernels for the same arithmetic (VERDICT r4 "route and switch sprawl": five forward routes, seven
// training routes, chosen from precision, row count, stack and rank count).  The dispatch sites of api_forward.hip /
// api_trainer.hip / api_sweep.hip / api_joint.hip ask the pure functions below (no HIP call, no handle) and switch on the
// answer -- also for rows per workgroup, workgroup counts and a sweep's shape: a launch site forms its grid from a
// ChainLaunch and decides nothing itself.  The same functions answer the queries of include/v21.h (v21_route_forward /
// v21_route_train: no GPU needed), which is what tests/test_routes.py checks against the table of INTEGRATION.md section 6
// -- on the CPU against the decision, on the GPU against what was launched (v21_trainer_last_route / v21_mlp_last_route
// are written by the launch sites themselves).
//
// Every environment switch that can change a route or a launch shape is read HERE (RouteEnv) and listed in INTEGRATION.md
// sections 5 and 6; the defaults are what ships, the switches exist for the tests (which force every kernel onto small
// cases) and for A/B measurements.  A step, an epoch of a sweep or joint pair and an evaluation pass read it once and hand
// it down.  Replaces nothing in the reference: Keras has one path (emulator.py:369-378, 402).
#pragma once
#include <cstdlib>

#include "act.h"
// internal forward flag (never part of include/v21.h; v21_mlp_forward masks caller flags to 0xFF): see decide_forward
#define V21_FWD_RT_LATCH_OFF 0x200

namespace v21 {

// ---- forward (v21_mlp_forward_dev)
enum FwdRoute {
  FWD_NONE = 0,
  FWD_SMALL = 1,     // few rows: one latency-oriented NT launch per layer (api_forward.hip: forward_small)
  FWD_FUSED = 2,     // fused_fwd<Arch, Prec> compiled into the library (archs.h S1-S4)
  FWD_FUSED_RT = 3,  // the same kernel instantiated at run time for this stack (jit.hip)
  FWD_TABLE = 4,     // table-driven one-launch forward: the chain kernels in FORWARD mode (train_chain.h / train_chain32.h)
  FWD_GENERIC = 5,   // per-layer K-loop GEMM (gemm.h): stacks wider than 512, f32 variational stacks
};
// ---- one optimizer step: the launch that carries forward pass, loss and activation gradients ...
enum TrainFwdRoute {
  TR_NONE = 0,
  TR_PER_LAYER = 1,   // one NT launch per layer and direction (gemm_nt.h)
  TR_CHAIN16 = 2,     // train_chain_kernel: 32-row blocks, activations in LDS, f16 / bf16
  TR_FUSED128 = 3,    // fused_train<Arch, Prec>: 128-row workgroups, 32 rows per wave (fused_train.h)
  TR_FUSED64 = 4,     // fused_train16<Arch, Prec>: 64-row workgroups, 16 rows per wave, two per CU (fused_train16.h)
  TR_CHAIN32 = 5,     // train_chain32_kernel: 16-row blocks, fp32 (train_chain32.h)
  TR_CHAIN32S_8 = 6,  // train_chain32s_kernel<8>: 8-row blocks, fp32, host-built job table (train_chain32s.h)
  TR_CHAIN32S_4 = 7,  // train_chain32s_kernel<4>
};
// ---- ... and what forms the weight gradients and applies Adam
enum TrainUpdRoute {
  UP_NONE = 0,
  UP_PER_LAYER = 1,     // NT launches per layer (+ slab sum) + [exchange] + adam_repack_kernel
  UP_DW16_ADAM = 2,     // dw16_adam_kernel: gradients + Adam + packed copies in ONE launch (dw_adam.h; one rank)
  UP_DW16_SPLITK = 3,   // gemm_dw16[_lds]_kernel grouped over the layers (+ slab sum) + [exchange] + adam_repack_kernel
  UP_DWADAM32 = 4,      // dwadam32_kernel: fp32 operands through LDS in whole rows, Adam in the epilogue (dw_adam32.h; one rank)
  UP_NT_DWADAM = 5,     // gemm_nt_dwadam_kernel: register operands, Adam in the epilogue (gemm_nt.h; one rank)
  UP_NT_SLICED = 6,     // grouped NT launch over batch slices (+ slab sum) + [exchange] + adam_repack_kernel (fp32 chain)
};
// fwd / upd: the routes.  The rest is how the step's weight gradients are cut up, for the routes that take an NT launch:
// the workgroup tile of the f32 one-launch update (32 or 64), and the batch slices of a sliced update (nslice slices of
// k_chunk rows; one slice: no slab to sum)
struct StepRoute { int fwd = TR_NONE, upd = UP_NONE; int tile = 32, nslice = 1, k_chunk = 0; };

// Every environment switch that changes a route or a launch shape.  Read per decision (a getenv is ~0.1 us; the tests set them per case).
struct RouteEnv {
  int train_chain = 1;        // V21_TRAIN_CHAIN=0: per-layer training path for every trainer
  int fused_train = 1;        // V21_FUSED_TRAIN=0: no fused training kernel
  int fused_train16 = -1;     // V21_FUSED_TRAIN16=0 / 1: which fused kernel a trainer commits to (-1: by max_batch)
  int fused_train_rows = -1;  // V21_FUSED_TRAIN_ROWS=n: steps of >= n rows take the fused kernel (-1: 8,193 / 16,384)
  int dw_split_rows = 8192;   // V21_DW_SPLIT_ROWS=n: one-rank 16-bit steps of >= n rows take split-K + Adam
  int chain32s = -1;          // V21_CHAIN32S=0 / 1: the small-batch fp32 chain (-1: by max_batch)
  int c32s_rows = 0;          // V21_C32S_ROWS=4 / 8: rows per workgroup of the small-batch fp32 chain (0: by rows)
  int dw32_lds = 1;           // V21_DW32_LDS=0: no LDS-staged fp32 gradient launch
  int dw32_adam = 1;          // V21_DW32_ADAM=0: no Adam in the fp32 gradient launch's epilogue
  int jit = 1;                // V21_JIT=0: no run-time compilation (cached code objects are still used)
  int dw_xrows = 0;           // V21_DW_XROWS=1: a fused large step does not flush its layer-0 operand, the gradient launch gathers the resident rows (fewer bytes, measured slower)
  int sweep_streams = 2;      // V21_SWEEP_STREAMS=1: a sweep's grouped launches on one stream (default 2: two half-groups, api_sweep.hip)
  int sweep32_group = 1;      // V21_SWEEP32_GROUP=0: f32 sweeps take one grouped launch per layer and phase
  int chain_plain = 1;        // V21_CHAIN_PLAIN=0: 16-bit trainers launch the chain's variational instantiation whatever the stack
  int chain_pref = -1;        // V21_CHAIN_PREF=n: prefetcher workgroups per XCD beside a chain's row blocks (-1: chain_prefetchers' own rule)
  int dw_blocks = 1;          // V21_DW_BLOCKS=0: dw16_adam_kernel walks contiguous tile runs per XCD (no dw_tile_order)
  int train_x16 = 1;          // V21_TRAIN_X16=0: the fused training kernels gather fp32 rows (no 16-bit copy of the training set)
  static RouteEnv read() {
    RouteEnv e;
    auto flag = [](const char* n, int dflt) { const char* v = getenv(n); return v ? (v[0] == '0' ? 0 : 1) : dflt; };
    auto num = [](const char* n, int dflt) { const char* v = getenv(n); return v ? atoi(v) : dflt; };
    e.train_chain = flag("V21_TRAIN_CHAIN", 1);
    e.fused_train = flag("V21_FUSED_TRAIN", 1);
    if (const char* v = getenv("V21_FUSED_TRAIN16")) e.fused_train16 = v[0] == '1' ? 1 : 0;
    e.fused_train_rows = num("V21_FUSED_TRAIN_ROWS", -1);
    e.dw_split_rows = num("V21_DW_SPLIT_ROWS", 8192);
    if (const char* v = getenv("V21_CHAIN32S")) e.chain32s = v[0] == '1' ? 1 : 0;
    e.c32s_rows = num("V21_C32S_ROWS", 0);
    e.dw32_lds = flag("V21_DW32_LDS", 1);
    e.dw32_adam = flag("V21_DW32_ADAM", 1);
    e.jit = flag("V21_JIT", 1);
    e.dw_xrows = flag("V21_DW_XROWS", 0);
    e.sweep_streams = num("V21_SWEEP_STREAMS", 2) == 1 ? 1 : 2;
    e.sweep32_group = flag("V21_SWEEP32_GROUP", 1);
    e.chain_plain = flag("V21_CHAIN_PLAIN", 1);
    if (const char* v = getenv("V21_CHAIN_PREF")) e.chain_pref = std::max(0, atoi(v));
    e.dw_blocks = flag("V21_DW_BLOCKS", 1);
    e.train_x16 = flag("V21_TRAIN_X16", 1);
    return e;
  }
};

// ---- the NT GEMM's cuts (gemm_nt.h), shared by every launch of it.  64 x 64 workgroup tiles once a launch has enough of
// them to fill the chip, 32 x 32 below.  `work`: the launch's 64 x 64 tiles, every batch slice counted.
inline int nt_tile(long long work) { return work >= 192 ? 64 : 32; }
// the weight gradient's contraction over `rows` batch rows in slices of at most kNtMaxKPerWg rows (whole 16-row steps;
// `whole`: one slice whatever the length).  kNtMaxKPerWg = 512 is the range a workgroup keeps in flight at once; a
// longer one (a layer fed by 600 features) is walked in rounds by the same loop.
struct NtSlices { int nslice, k_chunk; };
inline NtSlices nt_slices(int rows, bool whole) {
  int nslice = whole ? 1 : (rows + kNtMaxKPerWg - 1) / kNtMaxKPerWg;
  if (nslice < 1) nslice = 1;
  const int k_chunk = ((rows + nslice - 1) / nslice + 15) / 16 * 16;
  return NtSlices{(rows + k_chunk - 1) / k_chunk, k_chunk};
}
// a stack with an activation of act.h (tanh, sigmoid, elu, softplus) on any layer.  The chain kernels, the fused training
// kernels and the table-driven forward know ReLU and linear only (a `relu` flag, sign bits, bit masks): no route below
// may hand such a stack to them -- it trains per layer (gemm_nt.h: NT_FWD_ACT / NT_DX_ACT) and runs forward on
// fused_fwd instantiated at run time, the few-row route or the generic route
inline bool route_smooth(int L, const int* act) {
  for (int l = 0; l < L; ++l)
    if (act_is_smooth(act[l])) return true;
  return false;
}
inline int route_nw(const int* dims, const int* act, int l) { return act[l] == V21_ACT_GAUSS ? 2 * dims[l + 1] : dims[l + 1]; }
// the tile of a stack's f32 weight gradients in one launch: every layer's [dW; db] problem, one slice each
inline int dw32_tile(int L, const int* dims, const int* act) {
  long long work = 0;
  for (int l = 0; l < L; ++l) work += (long long)((dims[l] + 1 + 63) / 64) * ((route_nw(dims, act, l) + 63) / 64);
  return nt_tile(work);
}
// The update of an f32 chain step of `rows` rows.  One rank, a step of <= kDw32MaxRows rows, 32 x 32 tiles: gradients,
// Adam, packed streams and batch loss in ONE launch whose workgroups walk the whole batch in slabs of 256 rows
// (dw_adam32.h: UP_DWADAM32); one contraction slice with 64 x 64 tiles: gemm_nt_dwadam_kernel (UP_NT_DWADAM); larger
// steps and data-parallel ranks: sliced gradients, [slab sum, exchange], Adam (UP_NT_SLICED).  (Letting one workgroup
// walk 1,024 or 2,048 rows instead of the sliced three-launch form: 71.3 against 70.6 us and 96.7 against 92.8 us per
// step -- no gain.)
inline StepRoute plan_update32(int L, const int* dims, const int* act, int rows, int nranks, const RouteEnv& e) {
  StepRoute r;
  const bool single = nranks == 1;
  r.tile = dw32_tile(L, dims, act);
  const bool dw32 = single && e.dw32_adam && e.dw32_lds && L <= kNtMaxGroup && r.tile == 32 && rows <= kDw32MaxRows;
  const NtSlices sl = nt_slices(rows, dw32);
  if (single && sl.nslice <= 1 && L <= kNtMaxGroup && e.dw32_adam)
    r.upd = r.tile == 64 ? UP_NT_DWADAM : (rows <= kDw32MaxRows && e.dw32_lds ? UP_DWADAM32 : UP_NT_DWADAM);
  else
    r.upd = UP_NT_SLICED;
  if (r.upd == UP_NT_SLICED) { const NtSlices s = nt_slices(rows, false); r.nslice = s.nslice; r.k_chunk = s.k_chunk; }
  return r;
}

// ---- the shape of a chain-family launch.  The kernels map workgroup numbers XCD-major: a launch is whole rounds of the 8 XCDs
inline int xcd_rounds(long long blocks) { return (int)((blocks + 7) / 8 * 8); }
constexpr int kChipWgs = 256;  // one round of the chip: a workgroup per CU (train_chain32s.h: kC32sRows4Max = 4 kChipWgs)
// Rows per workgroup of train_chain32s_kernel and its forms: 4 while the 4-row blocks of all `models` models of the launch fit the
// chip in one round, else 8; V21_C32S_ROWS forces.  models: 1 trainer step / evaluation, G sweep, 2 joint epoch (1 joint evaluation: see there)
inline int c32s_rows(long long rows, int models, const RouteEnv& e) {
  if (e.c32s_rows == 4 || e.c32s_rows == 8) return e.c32s_rows;
  return (long long)models * ((rows + 3) / 4) <= kChipWgs ? 4 : 8;
}
// prefetcher workgroups per XCD beside `blocks` row-block workgroups: the CUs the row blocks leave idle
inline int chain_prefetchers(int blocks, const RouteEnv& e) {
  const int idle = kChipWgs - blocks;
  if (e.chain_pref >= 0) return std::max(0, std::min(e.chain_pref, idle / 8));  // (diagnosis)
  // (per XCD: none 45.6 us per f16 step at 4,096 rows, 2-4 43.4-43.6, 8 43.8-43.9, 16 44.2; f32 at batch 256: 46.4 / 42.6-42.8 / 42.9 / 43.4)
  return idle >= 8 ? std::min(4, idle / 8) : 0;
}
// ncons: row-block workgroups PER MODEL; npref: prefetcher workgroups per XCD.  One model's grid is ncons + 8 npref; the joint
// grids and a sweep's 8 ncons ceil(G / 8) are the launch sites' arithmetic on these.  pref_models: the models whose row blocks the
// prefetchers sit beside -- 1 in a trainer's own launch, 2 in the 16-bit joint launch, 0 = none: the f32 group and joint kernels have
// none, and a sweep of any size takes none (measured slower with them: 8 models, 24 prefetchers each: 106 k -> 95 k model-steps/s)
struct ChainLaunch { int rows_per_wg, ncons, npref; };
inline ChainLaunch chain_launch(long long rows, int rpw, int pref_models, const RouteEnv& e) {
  const int ncons = xcd_rounds((rows + rpw - 1) / rpw);
  return ChainLaunch{rpw, ncons, pref_models ? chain_prefetchers(pref_models * ncons, e) : 0};
}
// train_chain_kernel and its forms (32-row blocks), train_chain32_kernel (one model), train_chain32s_kernel and its forms
inline ChainLaunch plan_chain16(long long rows, int pref_models, const RouteEnv& e) { return chain_launch(rows, 32, pref_models, e); }
inline ChainLaunch plan_chain32(long long rows, const RouteEnv& e) { return chain_launch(rows, kC32Rows, 1, e); }
inline ChainLaunch plan_chain32s(long long rows, int models, int pref_models, const RouteEnv& e) {
  return chain_launch(rows, c32s_rows(rows, models, e), pref_models, e);
}

// ---- the shape of a sweep's or joint pair's epoch.  f32 models on the small-batch chain (a sweep: every member, at most
// kNtMaxGroup layers): one grouped chain launch + one grouped gradient / Adam launch per step (`enabled`: V21_SWEEP32_GROUP) -- the
// answer BEFORE the per-member tile check: a model whose gradient launch would take 64 x 64 tiles (refresh_dw32_table) ungroups the epoch
inline bool decide_group32(bool chain32s, int nranks, int batch, bool enabled = true) {
  return chain32s && nranks == 1 && batch <= kDw32MaxRows && enabled;
}
// grouped: the sweep's steps are grouped chain launches (16-bit members, or group32 after the tile check).  two_streams: as two
// half-groups on two streams (api_sweep.hip: v21_sweep::s2); small_slabs: the 128-row dwadam32_group_kernel (dw_adam32.h: SLAB)
struct SweepShape { bool two_streams, small_slabs; };
inline SweepShape decide_sweep(bool grouped, int members, int nranks, const RouteEnv& e) {
  // (below 16 members the second stream's hand-overs cost more than they hide: tiny members, 8 per group: 17.4 -> 23.6 us per step)
  // (dw_adam32.h: SLAB -- from 8 members on the gradient launch is deep enough for four or five workgroups per CU to pay: r5,
  //  f32, batch 256, 8 / 16 / 32 / 64 members 60 / 70-72 / 70 / 64-67 k -> 62-66 / 79 / 77-79 / 72-73 k model-steps/s)
  return SweepShape{nranks == 1 && grouped && members >= 16 && e.sweep_streams == 2, members >= 8};
}

// What a trainer commits to when it is created (buffers and packed stream formats depend on it).
struct TrainerKind {
  bool chain = false;     // 16-bit chain path (train_chain.h) -- otherwise per-layer
  bool chain32 = false;   // fp32 chain path
  bool chain32s = false;  // ... its small-batch kernel and stream format
  int train_arch = -1;    // index of the compiled fused training kernel (archs.h T1..), or -1
  bool train_rt = false;  // the fused training kernel may be instantiated at run time for this stack (jit.hip)
  bool train16 = false;   // the fused training kernel on 16 rows per wave
  int gl = -1;            // the V21_ACT_GAUSS layer or -1
  bool per_layer() const { return !chain && !chain32; }           // no chain kernel: one NT launch per layer and direction
  bool fused() const { return train_arch >= 0 || train_rt; }      // a fused training kernel, compiled in or instantiated at run time
};
// defined in api_trainer.hip: the registry of compiled fused training kernels / eligibility for run-time instantiation
int fused_train_arch_of(int L, const int* dims, const int* act);
bool fused_train_rt_eligible(int L, const int* dims, const int* act);


inline TrainerKind decide_trainer_kind(int L, const int* dims, const int* act, int precision, int max_batch, const RouteEnv& e) {
  TrainerKind k;
  for (int l = 0; l < L; ++l)
    if (act[l] == V21_ACT_GAUSS) k.gl = l;
  if (route_smooth(L, act)) return k;  // per-layer, for every precision and batch: no chain, no fused training kernel
  bool narrow = true;
  for (int l = 0; l <= L; ++l) narrow = narrow && dims[l] <= kChainMaxDim;
  if (precision != V21_PREC_F32) {
    bool ok = e.train_chain && narrow && (k.gl < 0 || dims[k.gl + 1] <= kChainMaxLatent);
    int mask_tiles = 0;
    for (int l = 0; l + 1 < L; ++l) mask_tiles += act[l] == V21_ACT_RELU ? (dims[l + 1] + 31) / 32 : 0;
    k.chain = ok && mask_tiles <= kChainMaskTiles;
    if (k.chain && k.gl < 0 && e.fused_train) {
      k.train_arch = fused_train_arch_of(L, dims, act);
      // (only the 16-rows-per-wave kernel is instantiated at run time: a stack outside archs.h takes it whatever max_batch is)
      k.train_rt = k.train_arch < 0 && e.fused_train16 != 0 && fused_train_rt_eligible(L, dims, act);
      // 16 rows per wave (64-row workgroups, two per CU) for trainers of fewer than 24,576 rows per step: a step of
      // 8,193 .. 24,575 rows does not fill the chip with 128-row workgroups; above, both take the same time and the
      // 128-row form has the evener workgroups
      if (k.train_arch >= 0) k.train16 = e.fused_train16 >= 0 ? e.fused_train16 == 1 : max_batch < 24576;
      if (k.train_rt) k.train16 = true;
    }
  } else {
    bool ok = e.train_chain && narrow;
    k.chain32s = e.chain32s >= 0 ? e.chain32s == 1 : max_batch <= kC32sMaxBatch;
    if (k.gl >= 0) ok = ok && k.chain32s && dims[k.gl + 1] <= kChainMaxLatent;
    int mask_tiles = 0;
    for (int l = 0; l + 1 < L; ++l)
      mask_tiles += act[l] == V21_ACT_RELU ? (k.chain32s ? (dims[l + 1] + 63) / 64 : (dims[l + 1] + 31) / 32) : 0;
    ok = ok && mask_tiles <= (k.chain32s ? kC32sMaskTiles : kC32MaskTiles);
    k.chain32 = ok;
    if (!ok) k.chain32s = false;
  }
  return k;
}

// One optimizer step of `rows` rows on this rank.  `fused_ready`: a fused training kernel can be launched now (compiled
// in, or its run-time code object has arrived); `capturing`: the step is being recorded into a hipGraph.
inline StepRoute decide_step(const TrainerKind& k, int L, const int* dims, const int* act, int rows, int nranks, bool capturing,
                             bool fused_ready, const RouteEnv& e) {
  StepRoute r;
  if (k.chain32) {
    r = plan_update32(L, dims, act, rows, nranks, e);
    if (k.chain32s) {
      r.fwd = c32s_rows(rows, 1, e) == 4 ? TR_CHAIN32S_4 : TR_CHAIN32S_8;
    } else {
      r.fwd = TR_CHAIN32;
    }
    return r;
  }
  if (k.per_layer()) {
    const NtSlices sl = nt_slices(rows, false);
    r.fwd = TR_PER_LAYER; r.upd = UP_PER_LAYER; r.nslice = sl.nslice; r.k_chunk = sl.k_chunk;
    return r;
  }
  // 16-bit chain trainers.  Steps of >= fused_rows rows of a stack with a fused training kernel take it: 8,193 rows for a
  // trainer on the 16-rows-per-wave kernel (the chain's second round of 256 workgroups starts there: 9,216 rows 67 against
  // 80 us, 12,288 rows 72 against 83, 16,384 rows 78-82 against 90-92), 16,384 rows for one on the 128-row kernel
  // (24,576 rows 101 against 127 us, 32,768 rows 123-130 against 152-160; autoencoder stack, f16, whole steps, r4)
  const int fused_rows = e.fused_train_rows >= 0 ? e.fused_train_rows : (k.train16 ? 8193 : 16384);
  const bool fused = k.fused() && fused_ready && rows >= fused_rows && !capturing;
  r.fwd = fused ? (k.train16 ? TR_FUSED64 : TR_FUSED128) : TR_CHAIN16;
  // one rank, nothing to exchange: gradients, Adam and the packed copies in one launch -- up to the batch where its
  // 32 x 32 tiles, each pulling its operands over the WHOLE batch through one CU, lose to the 128 x 128 LDS-staged
  // split-K kernel + an Adam launch that sums the slabs
  r.upd = (nranks == 1 && (rows < e.dw_split_rows || capturing) && !fused) ? UP_DW16_ADAM : UP_DW16_SPLITK;
  return r;
}

// ---- host-built tables of a 16-bit chain trainer (v21_trainer_create), pure functions of the stack
// The packed stream of the fused training kernels (fused_train.h / fused_train16.h): the virtual stack -- the L forward
// layers, then the L - 1 activation-gradient layers from the top down -- in fragments of 1,024 bytes.  Virtual layer v:
// K -> N over ks contraction steps (16 wide; 32 in the 16-rows-per-wave format) and nt feature tiles (32 wide; 16), its
// fragments from `first` on.  The trainer sizes its buffer from this table; the packer and the Adam pass write by it.
struct TrainStreamLayer { int K, N, ks, nt, first; };
struct TrainStream { std::vector<TrainStreamLayer> lt; int total = 0, padded = 0; };  // fragments; padded to whole rounds of 8
inline TrainStream train_stream_layout(int L, const int* dims, bool train16) {
  TrainStream s;
  for (int v = 0; v < 2 * L - 1; ++v) {
    const int l = v < L ? v : 2 * L - 1 - v;
    TrainStreamLayer y;
    y.K = v < L ? dims[l] : dims[l + 1]; y.N = v < L ? dims[l + 1] : dims[l];
    y.ks = train16 ? (y.K + 31) / 32 : (y.K + 15) / 16; y.nt = train16 ? (y.N + 15) / 16 : (y.N + 31) / 32;
    y.first = s.total;
    s.total += y.nt * (y.ks + 1);
    s.lt.push_back(y);
  }
  s.padded = (s.total + 7) / 8 * 8;
  return s;
}
// Tile order of dw16_adam_kernel: per layer the R x C grid of 32 x 32 tiles of [dW; db] in 8 blocks (rb x cb = 8, the shape
// with the least operand rows per block), the blocks handed to the XCDs largest first onto the least loaded XCD.
// Returns 8 runs of xper = size / 8 tile numbers (-1: none).
inline std::vector<int> dw_tile_order(int L, const int* dims, const int* act) {
  std::vector<std::vector<int>> per(8);
  int first = 0;
  for (int l = 0; l < L; ++l) {
    const int R = (dims[l] + 1 + 31) / 32, C = (route_nw(dims, act, l) + 31) / 32;
    int brb = 8, bcb = 1; double best = 1e30;
    for (int rb : {1, 2, 4, 8}) {
      const int cb = 8 / rb;
      const double cost = std::ceil((double)R / rb) + std::ceil((double)C / cb);
      if (cost < best) { best = cost; brb = rb; bcb = cb; }
    }
    std::vector<std::vector<int>> blocks(8);
    for (int i = 0; i < brb; ++i)
      for (int j = 0; j < bcb; ++j)
        for (int ti = R * i / brb; ti < R * (i + 1) / brb; ++ti)
          for (int tj = C * j / bcb; tj < C * (j + 1) / bcb; ++tj) blocks[i * bcb + j].push_back(first + ti * C + tj);
    std::sort(blocks.begin(), blocks.end(), [](const std::vector<int>& a, const std::vector<int>& b) { return a.size() > b.size(); });
    for (auto& b : blocks) {
      int xmin = 0;
      for (int x = 1; x < 8; ++x) if (per[x].size() < per[xmin].size()) xmin = x;
      per[xmin].insert(per[xmin].end(), b.begin(), b.end());
    }
    first += R * C;
  }
  size_t xper = 0;
  for (auto& v : per) xper = std::max(xper, v.size());
  std::vector<int> order(8 * xper, -1);
  for (int x = 0; x < 8; ++x) std::copy(per[x].begin(), per[x].end(), order.begin() + x * xper);
  return order;
}
// Feature K of a layer's input operand in the chain's fragment order (train_chain.h): the constant row of ones that turns
// [dW; db] into one contraction -- one feature tile of BS groups of 16 rows with element K % 32 of every row set to `one`
inline std::vector<unsigned short> ones_tile16(int K, long long BS, unsigned short one) {
  std::vector<unsigned short> tile((size_t)BS * 512, 0);
  for (long long b = 0; b < BS * 16; ++b) tile[(size_t)((b >> 4) * 64 + ((b >> 3) & 1) * 32 + (K & 31)) * 8 + (b & 7)] = one;
  return tile;  // (only element f % 32 == K % 32 of the last feature tile is set; the chain kernel writes features < K only)
}

// ---- forward.  jit: 0 = no run-time kernel for this stack (not eligible / switched off / failed), 1 = being compiled,
// 2 = ready.  `fused_compiled`: archs.h holds this stack.  Mirrors v21_mlp_forward_dev.
struct FwdQuery {
  int L; const int* dims; const int* act;
  bool fused_compiled; int jit; int precision; long long n; int flags; long long ldy;
};
inline bool route_chain_fwd_eligible(const FwdQuery& q) {
  if (q.flags & V21_FWD_FORCE_GENERIC) return false;
  if (route_smooth(q.L, q.act)) return false;  // (the chain kernels' `relu` flag cannot express them: V21_FWD_FORCE_CHAIN gives generic)
  for (int l = 0; l <= q.L; ++l)
    if (q.dims[l] > kChainMaxDim) return false;
  for (int l = 0; l < q.L; ++l)
    if (q.act[l] == V21_ACT_GAUSS && (q.precision == V21_PREC_F32 || q.dims[l + 1] > kChainMaxLatent || l == q.L - 1)) return false;
  if ((q.flags & V21_FWD_IN_TRANSFORM) && q.dims[0] > 8) return false;
  return true;
}
inline int decide_forward(const FwdQuery& q) {
  int maxdim = 0;
  for (int l = 0; l <= q.L; ++l) maxdim = q.dims[l] > maxdim ? q.dims[l] : maxdim;
  const bool tin_ok = !(q.flags & V21_FWD_IN_TRANSFORM) || q.dims[0] <= 8;
  const bool ldy_ok = q.ldy < (1ll << 21);
  const int force = q.flags & (V21_FWD_FORCE_GENERIC | V21_FWD_FORCE_CHAIN | V21_FWD_FORCE_JIT);
  const bool fused = q.fused_compiled && !force && tin_ok && ldy_ok;
  const bool fused_small = q.fused_compiled && !(q.flags & V21_FWD_FORCE_GENERIC) && tin_ok;
  const bool small = q.n <= V21_SMALL_BATCH_ROWS && !(q.flags & V21_FWD_NO_SMALL) && !force &&
                     (q.precision == V21_PREC_F32 || !fused_small) && tin_ok && maxdim <= kNtMaxKPerWg && ldy_ok;
  if (small) return FWD_SMALL;
  const bool jit_path = (!q.fused_compiled || (q.flags & V21_FWD_FORCE_JIT)) && !(q.flags & (V21_FWD_FORCE_GENERIC | V21_FWD_FORCE_CHAIN)) &&
                        ldy_ok && tin_ok && !(q.flags & V21_FWD_RT_LATCH_OFF);
  if (jit_path && q.jit == 2) return FWD_FUSED_RT;
  if (fused) return FWD_FUSED;
  if (route_chain_fwd_eligible(q) && q.n < (1ll << 30)) return FWD_TABLE;
  return FWD_GENERIC;
}

// ---- parameter Jacobian and Gaussian log-likelihood (v21_mlp_jacobian[_dev], v21_mlp_loglike[_dev]).  Its own enum:
// the forward's routes and their table are untouched.  ldy: the row pitch of y (fused_jac
// addresses a workgroup's rows with 32-bit offsets, as fused_fwd does).
enum JacRoute {
  JAC_NONE = 0,
  JAC_FUSED = 1,    // fused_jac<Arch, Prec> compiled into the library (archs.h S1-S4; fused_jac.h)
  JAC_GENERIC = 2,  // any other stack, any in_dim, variational stacks: jac_generic_kernel (jac_generic.h), f32 arithmetic
  JAC_FUSED_RT = 3, // fused_jac<this stack, Prec> instantiated at run time (jit.hip: kJitJac), for a handle that asked (K18)
};
constexpr int kJacMaxIn = 15;  // the fused Jacobian's in_dim limit, and that of the reduction of its rows (reduce_kernels.h)
// rt_ready: the handle asked for its run-time kernel (v21_mlp_jit_jacobian, or V21_FWD_FORCE_JIT on this call) and the
// code object is there.  The route is opt-in: a handle that never asked -- and every query without a handle -- passes
// false and gets what it always got.  A stack of archs.h keeps its compiled kernel unless the call forces the run-time one.
inline int decide_jacobian(bool fused_compiled, int in_dim, int flags, long long ldy, bool rt_ready) {
  const bool ok = in_dim <= kJacMaxIn && !(flags & V21_FWD_FORCE_GENERIC) && ldy < (1ll << 21);
  if (ok && rt_ready && (!fused_compiled || (flags & V21_FWD_FORCE_JIT))) return JAC_FUSED_RT;
  return ok && fused_compiled ? JAC_FUSED : JAC_GENERIC;
}

// ---- forward-only Gaussian log-likelihood (v21_mlp_loglike_fwd[_dev]): ln L without its gradient, the call an outside
// sampler makes.  Its own enum and counters: the Jacobian's routes above are untouched by it.
enum LnlRoute {
  LNL_NONE = 0,
  LNL_FUSED = 1,  // the ln L variant of fused_fwd<Arch, Prec> (fused_fwd.h: traits with LNL): chi-square reduced in the epilogue
  LNL_TWO = 2,    // the forward on its own route into the likelihood workspace, then lnl_reduce_kernel (reduce_kernels.h)
  LNL_FUSED_RT = 3,  // route 1's kernel instantiated for this stack at run time (jit.hip: kJitLnl), for a handle that asked (K19)
};
constexpr int kLnlWgRows = 128;  // rows per workgroup of the ln L variants: one data row per workgroup
// fused_compiled: archs.h holds the stack (no ReLU end, no Gauss layer); n_modes: the handle's nuisance modes; rpd: rows
// per data row of the call's data matrix (0: the record); n: the rows of the whole call.  Uniformity is decided HERE, once
// per call: the host form cuts a call into chunks of lnl_host_chunk rows, whole spectra that start on a workgroup boundary
// whenever rpd is a multiple of kLnlWgRows, so a chunk never needs a decision of its own.
inline long long lnl_host_chunk(long long chunk_rows, long long rpd) {
  return rpd > 0 && rpd <= chunk_rows ? chunk_rows / rpd * rpd : chunk_rows;
}
// rt_ready: the handle asked for its run-time ln L kernel (v21_mlp_jit_loglike) and the code object is loaded.  Opt-in, as
// decide_jacobian's: a handle that never asked -- and every query without a handle -- passes false and gets what it always
// got.  Route 3 stands exactly where route 1 would for a compiled stack; a stack of archs.h keeps its compiled kernel, and
// V21_FWD_FORCE_JIT here keeps its meaning: two-launch with the run-time FORWARD inside.
inline int decide_loglike_fwd(bool fused_compiled, int in_dim, int n_modes, long long rpd, long long n, int flags, bool rt_ready) {
  const bool forced = (flags & (V21_FWD_FORCE_GENERIC | V21_FWD_FORCE_CHAIN | V21_FWD_FORCE_JIT)) != 0;
  const bool tin_ok = !(flags & V21_FWD_IN_TRANSFORM) || in_dim <= 8;
  const bool uniform = rpd == 0 || rpd % kLnlWgRows == 0;  // one data row per workgroup
  const bool range = n / kLnlWgRows < (1ll << 31);         // (32-bit workgroup numbers)
  if (forced || !tin_ok || n_modes != 0 || !uniform || !range) return LNL_TWO;
  return fused_compiled ? LNL_FUSED : (rt_ready ? LNL_FUSED_RT : LNL_TWO);
}

// ---- the ensemble sampler (v21_mlp_sample_ensemble[_dev]): every evaluation of a call scores the n / 2 proposals of one
// half-move in their compacted layout (ensemble_kernels.h), on u.  One decision per call: the route is
// decide_loglike_fwd's for that half layout -- the record, or H (ensembles per spectrum) = rpd / 2 a multiple of
// kLnlWgRows -- and the host form's chunk is whole ensembles of W walkers, whole spectra when they fit; a fused call
// against a data matrix also needs every chunk's half layout to start on a workgroup boundary (chunks of whole multiples
// of lcm(W, 2 kLnlWgRows) rows): where no such chunk fits, the whole call goes two-launch.  rpd: rows per data row (0: the
// record); chunk_rows: the host forms' chunk (kJacHostChunk).  chunk: the rows of a host chunk (the _dev form: n).
constexpr int kEnsMaxWalkers = 512;  // an ensemble's two sets are decided and read inside one 256-thread workgroup
struct EnsRoute { int route; long long chunk; };
inline EnsRoute decide_ensemble(bool fused_compiled, int in_dim, int n_modes, long long rpd, long long n, int W, int flags, bool host_form,
                                long long chunk_rows, bool rt_ready) {
  EnsRoute r;
  r.route = decide_loglike_fwd(fused_compiled, in_dim, n_modes, rpd / 2, n / 2, flags & ~V21_FWD_IN_TRANSFORM, rt_ready);
  r.chunk = n;
  if (!host_form) return r;
  long long unit = W;
  if ((r.route == LNL_FUSED || r.route == LNL_FUSED_RT) && rpd > 0) {  // (the same kernel, the same workgroup boundaries)
    long long a = W, b = 2 * kLnlWgRows;
    while (b) { const long long t = a % b; a = b; b = t; }
    unit = (long long)W / a * (2 * kLnlWgRows);
    if (unit > chunk_rows) { r.route = LNL_TWO; unit = W; }
  }
  r.chunk = lnl_host_chunk(chunk_rows / unit * unit, rpd);
  return r;
}

}  // namespace v21
