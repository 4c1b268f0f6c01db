// nested_kernels.h -- the nested sampler on the device (api_nested.hip; include/v21.h: v21_mlp_sample_nested): evidence
// and weighted posterior samples from forward-only ln L, in the transformed coordinates u in [-1, 1]^din under the
// handle's prior on that box (rowmath.h: PriorArgs; uniform without a record).  N consecutive rows are one RUN, the live points of one spectrum; k = N / 2.  Iteration t
// ranks the run's ln L (ascending, ties on the row index), records the k lowest as DEAD, keeps the k highest -- the
// survivors, which then lie in rows k .. N - 1 in rank order --, restarts every dead row as a copy of a drawn survivor
// and moves those k rows n_repeats times by the difference move y = x + gamma (x_a - x_b), a and b distinct survivors,
// accepted iff y is inside the box and ln L(y) > L*, the ln L of rank k - 1.  Survivors do not move within an iteration.
// With a prior record (PRIOR) the move is a Metropolis move on the prior restricted to L > L*: it is accepted iff, beside
// the two conditions above, log(U) < ln p(y) - ln p(x); drawn starts are draws of the prior (below), and GIVEN starts are
// clamped into the box as they are -- that they are draws of the prior is the caller's business.  The shrinkage
// bookkeeping is the uniform prior's: the prior mass above L* shrinks as the volume did.
//   nested_step_kernel    one launch per evaluation of the n / 2 compacted proposals (row e k + j: moving slot j of run
//                         e): it DECIDES them, on an iteration boundary RANKS / RECORDS / RESTARTS, meets a barrier, then
//                         DRAWS the next proposals from the positions just settled;
//   nested_finish_kernel  the live points and the per-slot results.
// The opening launches pass the start rows through the same compacted layout in two halves (rows e N + h k + j, h = 0, 1),
// so that every ln L of a call comes from one route and one summation order.
// A 256-thread workgroup takes floor(256 / k) whole runs: thread (slot, j) owns moving slot j (row j of its run) and, on
// a boundary, ranks rows j and j + k.  Partners and restart sources are rows of the same run, written by threads of the
// same workgroup and read from global memory after a barrier, as the ensemble sampler's partners are
// (ensemble_kernels.h): writer and reader share a CU and its L1, the barrier's workgroup-scope release / acquire orders
// them.  No thread returns before a barrier, and the boundary's own barriers sit under a condition that is uniform over
// the launch; threads past the workgroup's runs or past n skip the work on every side of them.
// LDS: the ln L of the workgroup's runs for the ranking (at most 512 floats) and L* per run.  No atomics.
// Random numbers: Philox4x32-10 of sample_kernels.h keyed by the seed, counter (global row of the slot, step, block):
//   block 0, step = global move t n_repeats + s:  a = floor(k w0 / 2^32), b = (a + 1 + floor((k - 1) w1 / 2^32)) mod k;
//   block 1, step = global iteration t:           the restart source floor(k w0 / 2^32);
//   blocks 2 and 3, step 0:                       a drawn start, coordinate i from word i: float(2 U(w) - 1); a normal
//                                                 column of a prior record: float(mu + sd z), z the truncated standard
//                                                 normal's inverse CDF at U(w) (nest_tnorm_z);
//   block 4, step = that of block 0 (PRIOR only): the prior's acceptance uniform U(w0).
// With a hold record (HOLD; rowmath.h: HoldArgs) the start section writes the held float32 into given and drawn starts
// alike; a held column consumes no draw of its own (its word is left unused, the free columns keep theirs).  The
// difference move needs no change: every live point of a run carries the same float32 x in a held column, x_a - x_b is
// exactly 0 there and x + gamma 0 is x, bit for bit.  Ranking, shrinkage and the finish kernel are untouched: the prior
// mass is that of the free columns, whose record the launch site hands over with the held normal columns made uniform.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rowmath.h"
#include "sample_kernels.h"

namespace v21 {

// a workgroup's LDS holds L* of at most 256 / (kNestMinLive / 2) runs
constexpr int kNestMinLive = 16;

// per-row state; reject .. accepted are those of the moving slot j in row j < k of its run
struct NestRow {
  float u[kFitMaxIn];  // the point
  float lnl;           // ln L there, never NaN (a NaN evaluation is stored as -inf)
  float lstar;         // the iteration's threshold
  int reject;          // the pending proposal left the box: rejected unread
  int pa, pb;          // its partners, survivor indices (-1: none yet)
  int pad_;
  long long accepted;  // proposals accepted in this call
};

// what one call's step launches share
struct NestArgs {
  long long runs;      // of this call (or host chunk)
  int din, N, k, rpw;  // live points per run, N / 2, runs per workgroup
  int R;               // n_repeats
  float gamma;
  uint64_t seed, chain0;
  long long iter0;
  void* dead_u;        // (n_iter, runs, k, din), nullable
  float* dead_lnl;     // (n_iter, runs, k), nullable
  float* lstar;        // (n_iter, runs), nullable
};
// what one launch does, in this order (-1 / 0: not): take the evaluated start half; decide the pending move; the
// boundary of local iteration bt; draw local move dm; pass start half `start` on
struct NestLaunch {
  int take, decide, start, pad_;
  long long bt, dm;
};

__device__ inline float nest_key(float l) { return l != l ? -INFINITY : l; }

// z with Phi(z) = Phi(a) + U (Phi(b) - Phi(a)), a < b the standardised box ends, float64; where the box's middle lies
// above the mode (a + b > 0) the mirrored problem is solved, so that Phi is always taken in the tail nearer the mode
__device__ inline double nest_tnorm_z(double a, double b, double U) {
  const bool mirror = a + b > 0.0;
  const double pa = normcdf(mirror ? -a : a), pb = normcdf(mirror ? -b : b);
  const double z = normcdfinv(mirror ? pa - U * (pa - pb) : pa + U * (pb - pa));
  return mirror ? -z : z;
}

// one thread per (run, j).  start: the start rows (n, din) in u, or nullptr (drawn); prop: the compacted proposals
// (n / 2, din); lnl_new: their evaluation.  XT: the dead record's type; PRIOR: the handle holds a prior record, pr, and
// `dec` is the local move a deciding launch decides (neither is read without it).  HOLD: it holds a hold record; Hold:
// HoldArgs for HOLD = true, no argument for HOLD = false.
template <class XT, bool PRIOR, bool HOLD, class... Hold>
__global__ void __launch_bounds__(256) nested_step_kernel(NestRow* st, const float* __restrict__ start, float* __restrict__ prop,
                                                          const float* __restrict__ lnl_new, const NestLaunch l, const NestArgs a,
                                                          const PriorArgs pr, const long long dec, const Hold... hold) {
  static_assert(sizeof...(Hold) == (HOLD ? 1 : 0), "HOLD takes one HoldArgs, its absence nothing");
  [[maybe_unused]] const auto& ho = hold_of(hold...);
  constexpr int NI = kFitMaxIn;
  __shared__ float key[512];
  __shared__ float ls[256 / (kNestMinLive / 2)];
  const int din = a.din, k = a.k, N = a.N;
  const int slot = (int)threadIdx.x / k, j = (int)threadIdx.x % k;
  const long long e = (long long)blockIdx.x * a.rpw + slot;
  // (no thread returns before a barrier: one that is not `active` skips the work on every side of them)
  const bool active = slot < a.rpw && e < a.runs;
  const long long base = e * N, p = e * k + j;
  if (active && l.take >= 0) {
    // ---- the evaluated start half becomes state
    NestRow& s = st[base + (long long)l.take * k + j];
#pragma unroll
    for (int i = 0; i < NI; ++i) s.u[i] = i < din ? prop[p * din + i] : 0.f;
    s.lnl = nest_key(lnl_new[p]);
    s.lstar = -INFINITY;
    s.reject = 0;
    s.pa = s.pb = -1;
    s.accepted = 0;
  }
  if (active && l.decide) {
    // ---- decide the pending proposal of moving slot j: strictly above L*, on the float32 values; a NaN rejects
    NestRow& s = st[base + j];
    const float lnl_y = lnl_new[p];
    bool take = !s.reject && lnl_y > s.lstar;
    if constexpr (PRIOR) {
      if (take) {
        uint32_t w[4];
        sample_block(a.seed, a.chain0 + (uint64_t)(base + j), (uint32_t)(a.iter0 * a.R + dec), 4u, w);
        take = log(sample_uniform(w[0])) < prior_logp(pr, prop + p * din, din) - prior_logp(pr, s.u, din);
      }
    }
    if (take) {
#pragma unroll
      for (int i = 0; i < NI; ++i)
        if (i < din) s.u[i] = prop[p * din + i];
      s.lnl = lnl_y;
      s.accepted += 1;
    }
  }
  if (l.bt >= 0) {  // (uniform over the launch)
    // ---- rank rows j and j + k of the run by counting, record the dead, compact the survivors, restart
    float u0[NI], u1[NI], l0 = 0.f, l1 = 0.f;
    if (active) {
      const NestRow &s0 = st[base + j], &s1 = st[base + j + k];
#pragma unroll
      for (int i = 0; i < NI; ++i) { u0[i] = s0.u[i]; u1[i] = s1.u[i]; }
      l0 = s0.lnl; l1 = s1.lnl;
      key[slot * N + j] = l0;
      key[slot * N + j + k] = l1;
    }
    __syncthreads();  // (every row of the run is read and its ln L in LDS)
    if (active) {
      const float* kk = key + slot * N;
      int r0 = 0, r1 = 0;
      for (int q = 0; q < N; ++q) {
        const float v = kk[q];
        r0 += (v < l0 || (v == l0 && q < j)) ? 1 : 0;
        r1 += (v < l1 || (v == l1 && q < j + k)) ? 1 : 0;
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int r = h ? r1 : r0;
        const float lv = h ? l1 : l0;
        const float* uv = h ? u1 : u0;
        if (r < k) {
          const long long d = (l.bt * a.runs + e) * k + r;
          if (a.dead_u)
            for (int i = 0; i < din; ++i) ((XT*)a.dead_u)[d * din + i] = (XT)uv[i];
          if (a.dead_lnl) a.dead_lnl[d] = lv;
          if (r == k - 1) {
            ls[slot] = lv;
            if (a.lstar) a.lstar[l.bt * a.runs + e] = lv;
          }
        } else {
          NestRow& s = st[base + r];
#pragma unroll
          for (int i = 0; i < NI; ++i) s.u[i] = uv[i];
          s.lnl = lv;
        }
      }
    }
    __syncthreads();  // (the survivors lie in rows k .. N - 1 in rank order, L* in LDS)
    if (active) {
      uint32_t w[4];
      sample_block(a.seed, a.chain0 + (uint64_t)(base + j), (uint32_t)(a.iter0 + l.bt), 1u, w);
      const int c = (int)(((uint64_t)(uint32_t)k * (uint64_t)w[0]) >> 32);
      const NestRow& src = st[base + k + c];
      NestRow& s = st[base + j];
#pragma unroll
      for (int i = 0; i < NI; ++i) s.u[i] = src.u[i];
      s.lnl = src.lnl;
      s.lstar = ls[slot];
    }
  }
  __syncthreads();  // (the positions the work above settled are in place for this workgroup's readers)
  if (active && l.dm >= 0) {
    // ---- draw the next proposal of moving slot j, in float32: y = x + gamma (x_a - x_b)
    NestRow& s = st[base + j];
    uint32_t w[4];
    sample_block(a.seed, a.chain0 + (uint64_t)(base + j), (uint32_t)(a.iter0 * a.R + l.dm), 0u, w);
    const int pa = (int)(((uint64_t)(uint32_t)k * (uint64_t)w[0]) >> 32);
    const int pb = (pa + 1 + (int)(((uint64_t)(uint32_t)(k - 1) * (uint64_t)w[1]) >> 32)) % k;
    const float *xa = st[base + k + pa].u, *xb = st[base + k + pb].u;
    bool inside = true;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      if (i < din) {
        const float diff = xa[i] - xb[i];
        const float y = s.u[i] + a.gamma * diff;
        if (!(y >= -1.f && y <= 1.f)) inside = false;
        prop[p * din + i] = y;
      }
    }
    s.reject = inside ? 0 : 1;
    s.pa = pa;
    s.pb = pb;
  }
  if (active && l.start >= 0) {
    // ---- pass start half `start` on to its evaluation: given rows into the box, or drawn from the prior on it
    const long long row = base + (long long)l.start * k + j;
    if (start) {
      for (int i = 0; i < din; ++i) prop[p * din + i] = box_clamp1(start[row * din + i]);
    } else {
#pragma unroll
      for (int b = 0; b < NI / 4; ++b) {
        if (4 * b < din) {
          uint32_t w[4];
          sample_block(a.seed, a.chain0 + (uint64_t)row, 0u, 2u + (uint32_t)b, w);
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (4 * b + i < din) {
              const int c = 4 * b + i;
              float v = (float)(2.0 * sample_uniform(w[i]) - 1.0);
              if constexpr (PRIOR) {
                if (pr.kind[c]) {
                  const double sd = 1.0 / sqrt(pr.w[c]);
                  const double z = nest_tnorm_z((-1.0 - pr.mu[c]) / sd, (1.0 - pr.mu[c]) / sd, sample_uniform(w[i]));
                  v = box_clamp1((float)(pr.mu[c] + sd * z));
                }
              }
              prop[p * din + c] = v;
            }
        }
      }
    }
    hold_row<HOLD>(ho, din, prop + p * din);
  }
}

// one thread per row: the live points (u, type XT) with their ln L and, from row j < k of a run, moving slot j's results
// (all nullable but live_u; moves: the proposals a slot decided in this call)
struct NestOutDev {
  void* live_u;
  float* live_lnl;
  double* accept_rate;
  int* last_partner;
  float* last_prop_u;
};
template <class XT>
__global__ void __launch_bounds__(256) nested_finish_kernel(const NestRow* __restrict__ st, const float* __restrict__ prop, long long n, int din,
                                                            int N, long long moves, const NestOutDev o) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const NestRow& s = st[row];
  for (int i = 0; i < din; ++i) ((XT*)o.live_u)[row * din + i] = (XT)s.u[i];
  if (o.live_lnl) o.live_lnl[row] = s.lnl;
  const int k = N / 2, j = (int)(row % N);
  if (j >= k) return;
  const long long p = row / N * k + j;
  if (o.accept_rate) o.accept_rate[p] = moves > 0 ? (double)s.accepted / (double)moves : 0.0;
  if (o.last_partner) { o.last_partner[2 * p] = s.pa; o.last_partner[2 * p + 1] = s.pb; }
  if (o.last_prop_u)
    for (int i = 0; i < din; ++i) o.last_prop_u[p * din + i] = prop[p * din + i];
}

}  // namespace v21
