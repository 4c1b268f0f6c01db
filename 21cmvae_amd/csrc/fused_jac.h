// fused_jac.h -- forward-mode parameter Jacobian of a dense stack in ONE launch (gfx950).
//
// The fused forward kernel (fused_fwd.h) keeps signals on the accumulator's columns (lane % 32) through every hidden
// layer.  This kernel runs the SAME weight stream, ring, geometry and MFMA through the same stack, on "virtual rows":
// row n of the input becomes G consecutive columns -- the primal (column n*G) and in_dim tangents (columns n*G + 1 +
// j, the unit vector e_j of the TRANSFORMED input), zero-padded to G (G = 8 for in_dim <= 7, 16 for in_dim <= 15).  A
// 32-column tile therefore carries 32 / G signals.
//   * bias: added to primal columns only (the accumulator's initial value, as in fused_fwd).
//   * ReLU: the mask is the primal's f32 pre-activation z > 0 (the shipped ReLU's rule).  One __ballot per register,
//     ANDed with the primal-lane pattern (0x0101..01 for G = 8) and spread over each group of G lanes by one integer
//     multiply (x 0xFF); one select per register then applies the primal's ReLU and masks its tangents.  For the
//     primal this is bit for bit the forward's ReLU (pack + signed max with 0 in 16 bits, integer max in f32).
//   * output layer (swapped orientation, rows = virtual rows): primal rows get bias + std / mean exactly as
//     fused_fwd's epilogue and go to y; tangent rows are scaled by std and by the chain-rule factor of the input
//     transform (fac, f32, computed by jac_prep_kernel at the floored parameter value) and go to jac (n, in_dim, out).
// The primal therefore takes the same MFMA instruction, k-order and epilogue arithmetic as fused_fwd<Arch, P>: y is
// bit-identical to the forward's fused route (tests/test_jacobian_gpu.py).
#pragma once
#include "fused_fwd.h"

namespace v21 {

struct JacArgs {
  const float* x;     // transformed f32 parameter rows (n, in_dim), row pitch ldx
  long long ldx;
  const float* fac;   // (n, in_dim): d(transformed x_j) / d(raw x_j) -- 1 without an input transform
  float* y;           // (n, ldy), nullable
  long long ldy;
  float* jac;         // (n, in_dim, out_dim)
  long long n_rows;
  const unsigned char* stream;  // fused_fwd's packed weight stream of the same precision
  float out_std;
  float out_mean_scale;
};

// virtual rows per signal: the one rule, for the kernel (jac_group<IN>) and for the host's launch geometry (jit.hip)
constexpr int jac_group_of(int in_dim) { return in_dim <= 7 ? 8 : 16; }
template <int IN> constexpr int jac_group() {
  static_assert(IN >= 1 && IN <= 15, "fused Jacobian: at most 15 inputs");
  return jac_group_of(IN);
}

// The value of the first lane of each group of GR consecutive lanes (the primal's) in every lane of the group, by DPP:
// quad_perm [0, 0, 0, 0] fills each quad from its lane 0, then row_shr:4 into bank 1 [and 3] and, for GR = 16, row_shr:8
// into banks 2 and 3 copy the first quad over the group.  2 (3) VALU moves in the wave's own registers: no LDS-queue
// slot (ds_bpermute / __shfl take one, and the ring's LDS reads wait on that queue), no memory counter touched -- the
// ring's counted vmcnt waits stand as they are.  gfx950 has no DPP8 and no row_share; rows are 16 lanes, so a group
// never crosses one.
template <int GR>
__device__ __forceinline__ float jac_group_bcast(float v) {
  static_assert(GR == 8 || GR == 16, "groups of 8 or 16 lanes");
  int x = __builtin_bit_cast(int, v);
  x = __builtin_amdgcn_update_dpp(x, x, 0x000, 0xF, 0xF, false);  // quad_perm [0, 0, 0, 0]
  if constexpr (GR == 8) {
    x = __builtin_amdgcn_update_dpp(x, x, 0x114, 0xF, 0xA, false);  // row_shr:4 -> lanes 4-7 and 12-15
  } else {
    x = __builtin_amdgcn_update_dpp(x, x, 0x114, 0xF, 0x2, false);  // row_shr:4 -> lanes 4-7
    x = __builtin_amdgcn_update_dpp(x, x, 0x118, 0xF, 0xC, false);  // row_shr:8 -> lanes 8-15
  }
  return __builtin_bit_cast(float, x);
}

// grid.x = ceil(n_rows * G / (WAVES*CT*32)); block = 64*WAVES threads; dynamic LDS fused_lds<P>().
template <class Arch, class P>
__global__ void __launch_bounds__(64 * P::WAVES, P::WPS) fused_jac(const JacArgs a) {
  constexpr int kWaves = P::WAVES;
  constexpr int kBlkFrags = P::BLK, kRing = P::RING;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // fused_fwd's geometry.  A chunk of the output layer issues 2 or 3 stores where Geo counts 2: more younger
  // operations than the ring's counted waits assume only make those waits stricter.
  using G = Geo<Arch, P>;
  using frag = typename P::frag;
  using Item = typename G::Item;
  constexpr int L = G::L, CT = P::CT, EPI = P::EPI, FPI = P::FPI, IPT = G::IPT;
  constexpr int KSM = G::ks_max();
  constexpr int D = P::DEPTH;
  constexpr bool SPREAD = spread_of<P>::value;
  constexpr int TOTAL = G::total();
  constexpr int K0 = G::dim(0);
  constexpr int NOUT = G::dim(L);
  constexpr int NCH = CT * 8;
  constexpr int GR = jac_group<K0>();
  constexpr int SPW = 32 * CT / GR;  // signals per wave
  // primal lanes of a register (bit k = lane k) and the spread of one bit over its group of GR lanes
  constexpr unsigned long long PAT = GR == 8 ? 0x0101010101010101ull : 0x0001000100010001ull;
  constexpr unsigned long long SPR = GR == 8 ? 0xFFull : 0xFFFFull;
  static_assert(G::act(L - 1) == 0, "output layer must be linear");
  static_assert(G::nt_of(L - 1) == 1 || G::ks_of(L - 1) > P::DEPTH, "output layer: too few k-steps per tile for the aux double buffer");
  static_assert(D <= kBlkFrags, "read-ahead must stay within one block");

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int g_lane = r & (GR - 1);  // this lane's column: 0 = primal, j + 1 = tangent j
  const bool prim_lane = g_lane == 0;
  const long long wg_vrow0 = (long long)blockIdx.x * (kWaves * CT * 32);
  const long long vrow0 = wg_vrow0 + wave * (CT * 32);
  const long long n0 = wg_vrow0 / GR;  // first signal of the workgroup

  unsigned bufA[CT][KSM][4], bufB[CT][KSM][4];
  float fac[CT];  // chain-rule factor of this lane's tangent (hidden layout: lane r = virtual row)

  // ---- layer-0 operand: the primal's x row (already transformed, as the forward's prologue would), unit tangents
  static_for<CT>([&](auto ct_) __attribute__((always_inline)) {
    constexpr int ct = decltype(ct_)::value;
    const long long n = (vrow0 + ct * 32 + r) / GR;
    const bool ok = n < a.n_rows;
    const float* xr = a.x + (ok ? n : 0) * a.ldx;
    fac[ct] = (ok && g_lane >= 1 && g_lane <= K0) ? a.fac[n * K0 + g_lane - 1] : 0.f;
    static_for<G::ks_of(0)>([&](auto ks_) __attribute__((always_inline)) {
      constexpr int ks = decltype(ks_)::value;
      float v[EPI];
      static_for<EPI>([&](auto e_) __attribute__((always_inline)) {
        constexpr int e = decltype(e_)::value;
        constexpr int f0 = FPI * ks + 8 * (e >> 2) + (e & 3);
        constexpr int f1 = f0 + 4;
        float t = 0.f;
        if constexpr (f0 < K0) {
          const bool valid = ok && (h == 0 || f1 < K0);
          const int f = h ? f1 : f0;
          if (valid) t = prim_lane ? xr[f] : (f == g_lane - 1 ? 1.f : 0.f);
        }
        v[e] = t;
      });
#pragma unroll
      for (int wd = 0; wd < 4; ++wd) {
        if constexpr (EPI == 8) bufA[ct][ks][wd] = P::pack2(v[2 * wd], v[2 * wd + 1]);
        else bufA[ct][ks][wd] = __builtin_bit_cast(unsigned, v[wd]);
      }
    });
  });

  static_for<kRing>([&](auto b) __attribute__((always_inline)) {
    issue_block<G, decltype(b)::value>(a.stream, smem, wave, lane);
  });

  // output addressing: per-workgroup buffer resources (rows past n_rows, bins past out_dim and padding tangents are
  // dropped by the range check while the store still issues)
  long long wg_sig = a.n_rows - n0;
  if (wg_sig > kWaves * CT * 32 / GR) wg_sig = kWaves * CT * 32 / GR;
  if (wg_sig < 0) wg_sig = 0;
  __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(a.y ? a.y + n0 * a.ldy : a.jac), 0, a.y ? (unsigned)(wg_sig * a.ldy * 4) : 0u, 0x00020000);
  __amdgpu_buffer_rsrc_t jrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(a.jac + n0 * K0 * NOUT), 0, (unsigned)(wg_sig * K0 * NOUT * 4),
                                                                   0x00020000);
  const int nw0 = wave * SPW;  // first signal of this wave within the workgroup

  frag q[D + 1];
  f32x16 auxb[2];
  f32x16 acc[2][CT];

  // register i of column tile ct: virtual row ct*32 + base(i) + 4h of the wave; its column within the signal's group
  // is gbase(i) + 4h, its signal nw0 + ct*(32/GR) + sig(i)
  auto epilogue_chunk = [&](auto g_, auto c_) __attribute__((always_inline)) {
    constexpr int GT = decltype(g_)::value;
    constexpr int c = decltype(c_)::value;
    constexpr Item t = G::tile_at(GT);
    constexpr int l = t.l, nt = t.nt;
    constexpr int ct = c / 8, pr = c % 8;
    if constexpr (l < L - 1) {
      constexpr int item = IPT * nt + (2 * pr) / EPI, e0 = (2 * pr) % EPI;
      if constexpr (item < G::ks_of(l + 1)) {
        auto& out = (l & 1) ? bufA : bufB;
        float x0 = acc[GT & 1][ct][2 * pr], x1 = acc[GT & 1][ct][2 * pr + 1];
        if constexpr (G::act(l) >= 3) {
          // an activation of act.h (run-time instantiations only: archs.h has none); its own branch: the ReLU / linear
          // code below is what it was.  Primal lanes take act_apply on the f32 accumulator before the pack -- fused_fwd's
          // smooth branch, bit for bit; tangent lanes take t * act'(z) with act' from the PRIMAL's z (act.h: a saturated
          // unit has no digits left in 1 - h^2), brought from the group's first lane by jac_group_bcast.  |act'| <= 1.
          // Padding: the features >= dim(l + 1) of a partial tile hold act(0) on primal lanes afterwards (0.5 for sigmoid,
          // ln 2 for softplus) and meet only the ZERO weights pack_stream_kernel writes for them, as in fused_fwd; padding
          // virtual rows (g_lane > in_dim) carry zero tangents and 0 * act' stays 0; rows past n_rows are dropped by the
          // stores' range check.  (Both functions are also evaluated on tangent lanes, whose "z" is a tangent: whatever they
          // give there -- an inf included -- is dropped by the prim_lane selects and overwritten by the broadcast.)
          const float d0 = jac_group_bcast<GR>(act_deriv_in<G::act(l)>(x0));
          const float d1 = jac_group_bcast<GR>(act_deriv_in<G::act(l)>(x1));
          const float h0 = act_apply<G::act(l)>(x0), h1 = act_apply<G::act(l)>(x1);
          x0 = prim_lane ? h0 : x0 * d0;
          x1 = prim_lane ? h1 : x1 * d1;
        } else if constexpr (G::act(l) != 0) {
          const unsigned long long m0 = (__ballot(x0 > 0.f) & PAT) * SPR;
          const unsigned long long m1 = (__ballot(x1 > 0.f) & PAT) * SPR;
          x0 = __builtin_amdgcn_inverse_ballot_w64(m0) ? x0 : 0.f;
          x1 = __builtin_amdgcn_inverse_ballot_w64(m1) ? x1 : 0.f;
        }
        if constexpr (EPI == 8) {
          out[ct][item][e0 / 2] = P::pack2(x0, x1);
        } else {
          out[ct][item][e0] = __builtin_bit_cast(unsigned, x0);
          out[ct][item][e0 + 1] = __builtin_bit_cast(unsigned, x1);
        }
      }
    } else {
      const float obias = auxb[GT & 1][0], omean = auxb[GT & 1][1] * a.out_mean_scale;
      const int bin = 32 * nt + r;
      static_for<2>([&](auto u_) __attribute__((always_inline)) {
        constexpr int i = 2 * pr + decltype(u_)::value;
        constexpr int base = ct * 32 + (i & 3) + 8 * (i >> 2);
        constexpr int gbase = base & (GR - 1);
        const int nloc = nw0 + (base - gbase) / GR;  // signal within the workgroup
        const int g = gbase + 4 * h;
        if constexpr (gbase == 0) {  // h = 0: the primal row -> y, as fused_fwd stores it
          float yv;
          if constexpr (EPI == 8) yv = __builtin_fmaf(acc[GT & 1][ct][i], a.out_std, __builtin_fmaf(obias, a.out_std, omean));
          else yv = (acc[GT & 1][ct][i] + obias) * a.out_std + omean;
          const unsigned yoff = (h == 0 && bin < NOUT) ? ((unsigned)nloc * (unsigned)a.ldy + (unsigned)bin) * 4u : 0xFFFFFFF0u;
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, yv), yrsrc, yoff, 0, 0);
        }
        // tangent rows: d(out) / d(transformed x) x std x the input transform's factor of this row's column
        const float fv = __builtin_bit_cast(float, h ? __builtin_amdgcn_readlane(__builtin_bit_cast(int, fac[ct]), base + 4)
                                                   : __builtin_amdgcn_readlane(__builtin_bit_cast(int, fac[ct]), base));
        const float tv = acc[GT & 1][ct][i] * a.out_std;
        const unsigned joff = (g >= 1 && g <= K0 && bin < NOUT) ? (((unsigned)nloc * K0 + (unsigned)(g - 1)) * NOUT + (unsigned)bin) * 4u
                                                                : 0xFFFFFFF0u;
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, tv * fv), jrsrc, joff, 0, 0);
      });
    }
  };
  auto epilogue_range = [&](auto g_, auto lo_, auto hi_) __attribute__((always_inline)) {
    constexpr int LO = decltype(lo_)::value, HI = decltype(hi_)::value;
    static_for<(HI > LO ? HI - LO : 0)>([&](auto k) __attribute__((always_inline)) {
      epilogue_chunk(g_, std::integral_constant<int, LO + decltype(k)::value>{});
    });
  };
  auto operand = [&](auto& buf, int ct, int ks) __attribute__((always_inline)) {
    const u32x4 wds = {buf[ct][ks][0], buf[ct][ks][1], buf[ct][ks][2], buf[ct][ks][3]};
    return __builtin_bit_cast(frag, wds);
  };

  // ---- the stream: fused_fwd's schedule (load side D items ahead of the compute side, epilogue chunks spread over
  // the next tile's k-steps)
  static_for<TOTAL + D>([&](auto s_) __attribute__((always_inline)) {
    constexpr int S = decltype(s_)::value;
    if constexpr (S < TOTAL) {
      ring_boundary<G, CT, D, S, SPREAD>(a.stream, smem, wave, lane);
      if constexpr (SPREAD && S / kBlkFrags >= 2) {
        constexpr int Bc = S / kBlkFrags, o = S % kBlkFrags;
        if constexpr (o % G::WAVES == V21_SP_PHASE % G::WAVES)
          issue_piece<G, Bc + kRing - 2, o / G::WAVES>(a.stream, smem, wave, lane);
      }
      constexpr Item it = G::item_at(S);
      if constexpr (it.ks >= 0) {
        q[S % (D + 1)] = *(const frag*)frag_ptr<G, S>(smem, lane);
      } else {
        constexpr int GT = G::gtile(it.l, it.nt);
        const unsigned char* aux = frag_ptr<G, S>(smem, 0);
        if constexpr (it.l < L - 1) {
          const f32x4* bp = (const f32x4*)(aux + h * 64);
#pragma unroll
          for (int qd = 0; qd < 4; ++qd) {
            const f32x4 t = bp[qd];
            auxb[GT & 1][4 * qd + 0] = t[0]; auxb[GT & 1][4 * qd + 1] = t[1];
            auxb[GT & 1][4 * qd + 2] = t[2]; auxb[GT & 1][4 * qd + 3] = t[3];
          }
        } else {
          auxb[GT & 1][0] = ((const float*)aux)[r];
          auxb[GT & 1][1] = ((const float*)aux)[32 + r];
        }
      }
    }
    if constexpr (S >= D) {
      constexpr int C = S - D;
      constexpr Item it = G::item_at(C);
      if constexpr (it.ks >= 0) {
        constexpr int GT = G::gtile(it.l, it.nt);
        constexpr int GP = GT > 0 ? GT - 1 : 0;
        constexpr int CPK = G::chunks_per_kstep(GP, NCH);
        constexpr bool whole_first = (GT > 0) && (G::spread_limit(GP) == 0);
        if constexpr (whole_first && it.ks == 0) {
          epilogue_range(std::integral_constant<int, GP>{}, std::integral_constant<int, 0>{},
                         std::integral_constant<int, NCH>{});
        }
        auto& in = (it.l & 1) ? bufB : bufA;
        const frag w = q[C % (D + 1)];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          f32x16 c0;
          if constexpr (it.ks == 0) {
            if constexpr (it.l < L - 1) {
#pragma unroll
              for (int i = 0; i < 16; ++i) c0[i] = prim_lane ? auxb[GT & 1][i] : 0.f;  // bias: primal columns only
            } else {
#pragma unroll
              for (int i = 0; i < 16; ++i) c0[i] = 0.f;
            }
          } else {
            c0 = acc[GT & 1][ct];
          }
          acc[GT & 1][ct] = P::template mfma<(it.l == L - 1)>(w, operand(in, ct, it.ks), c0);
        }
        if constexpr (GT > 0 && !whole_first) {
          constexpr int lo = it.ks * CPK < NCH ? it.ks * CPK : NCH;
          constexpr int hi = (it.ks + 1) * CPK < NCH ? (it.ks + 1) * CPK : NCH;
          epilogue_range(std::integral_constant<int, GP>{}, std::integral_constant<int, lo>{},
                         std::integral_constant<int, hi>{});
        }
      }
    }
  });
  epilogue_range(std::integral_constant<int, G::n_tiles() - 1>{}, std::integral_constant<int, 0>{},
                 std::integral_constant<int, NCH>{});

}

}  // namespace v21
