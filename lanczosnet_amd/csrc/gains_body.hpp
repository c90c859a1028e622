// Device body of the spectral-gains MLP (R7a), shared by the standalone kernel of
// spectral_gains.hip and the fused batch-preparation launch of lanczos_ritz.hip.
#pragma once
#include "common.hpp"
#include <stdlib.h>
#include <type_traits>

namespace lnz_gains {

constexpr int HID = 128;           // hidden width of the reference's spectral_filter MLP
constexpr int HT = HID / 32;       // 4 feature tiles
constexpr int SMAX = 16;           // exponents supported (two k-halves of 8)
// pack layout (floats) per conv layer: scalars/biases first, then the three 128-wide weight
// streams CONTIGUOUS (W2 | W4 | W6) so the kernel reads them as one prefetched stream, then slack
// for the prefetch ring's over-read.
constexpr int OFF_W0 = 0;                       // [HT][8][64]          A scalars of Linear(S->128)
constexpr int OFF_B0 = OFF_W0 + HT * 8 * 64;    // [HT][64][16]
constexpr int OFF_B2 = OFF_B0 + HT * 1024;
constexpr int OFF_B4 = OFF_B2 + HT * 1024;
constexpr int OFF_B6 = OFF_B4 + HT * 1024;      // [1][64][16]
constexpr int OFF_W2 = OFF_B6 + 1024;           // rows_k8(128,128): [HT][16][64] float4
constexpr int OFF_W4 = OFF_W2 + HT * 16 * 256;
constexpr int OFF_W6 = OFF_W4 + HT * 16 * 256;  // rows_k8(32,128) (S rows zero padded to 32)
#ifndef LNZ_GAINS_RING
#define LNZ_GAINS_RING 8
#endif
#ifndef LNZ_GAINS_DIST
#define LNZ_GAINS_DIST (LNZ_GAINS_RING - 2)
#endif
constexpr int RING = LNZ_GAINS_RING;             // prefetch ring slots (distance LNZ_GAINS_DIST steps)
constexpr int PACK_V1 = OFF_W6 + 16 * 256 + RING * 256;   // end of the padded form's pack
// Behind the slack, the compact form's two images (nothing in front of them moves):
//   W0c[ot][u][lane]  = W0[32 ot + (lane & 31)][2 u + (lane >> 5)]   S <= 8: both k-halves of a
//                       first-layer MFMA carry a feature (zero beyond S)
//   W6c[grp][v][4 blk + i] = W6[4 grp + i][8 (2 v + (blk >> 3)) + rev3(blk & 7)]
//                       the A scalars of the 4x4x1 last layer, 16 k's per register: the MFMA
//                       broadcasts block `abid` of A to all 16 blocks (cbsz = 4), so register v
//                       serves stream steps q = 2v, 2v + 1 with abid = 8 (q & 1) + j, in the order
//                       the chains take the k's: j = 0..3 the k's of step q's .x and .z (lower
//                       k-half, then upper), j = 4..7 those of .y and .w
constexpr int OFF_W0C = PACK_V1;                 // [HT][4][64]
constexpr int OFF_W6C = OFF_W0C + HT * 4 * 64;   // [SMAX/4][8][64] (rows >= S zero)
constexpr int PACK_SIZE = OFF_W6C + (SMAX / 4) * 8 * 64;
constexpr int NSTEP = 2 * HT * 16 + 16;         // float4 steps of the W2|W4|W6 stream (144)

struct DistArr {
  int32_t v[SMAX];
};

// LNZ_GAINS_COMPACT=0 selects the padded form (the in-build reference); read once per process
inline bool compact_form() {
  static const bool on = [] {
    const char* e = getenv("LNZ_GAINS_COMPACT");
    return e ? atoi(e) != 0 : true;
  }();
  return on;
}

// source of pack float f of the compact images (OFF_W0C <= f < PACK_SIZE): the flat index into
// the raw row-major W0 [128,S] (*tensor = 0) or W6 [S,128] (*tensor = 6); *tensor = -1: a zero
__host__ __device__ inline int64_t compact_source(int S, int f, int* tensor) {
  *tensor = -1;
  if (f < OFF_W6C) {
    const int g = f - OFF_W0C;
    const int lane = g & 63, u = (g >> 6) & 3, ot = g >> 8;
    const int feat = 2 * u + (lane >> 5);
    if (feat >= S) return 0;
    *tensor = 0;
    return (int64_t)(32 * ot + (lane & 31)) * S + feat;
  }
  const int g = f - OFF_W6C;
  const int lane = g & 63, v = (g >> 6) & 7, grp = g >> 9;
  const int blk = lane >> 2, row = 4 * grp + (lane & 3);
  const int j = blk & 7, q = 2 * v + (blk >> 3);
  if (row >= S) return 0;
  *tensor = 6;
  return (int64_t)row * HID + 8 * q + (((j & 1) << 2) | (j & 2) | (j >> 2));
}

__device__ inline float powi(float x, int p) {
  // integer power in fp64, rounded once to fp32 (torch.pow(D, ii), model/lanczos_net.py:148,
  // is a <= 1 ulp powf; this is the correctly rounded value)
  double base = (double)x, acc = 1.0;
  int e = p < 0 ? -p : p;
  while (e) {
    if (e & 1) acc *= base;
    base *= base;
    e >>= 1;
  }
  return (float)(p < 0 ? 1.0 / acc : acc);
}

__device__ inline f32x16 load_bias_frag(const float* __restrict__ bp, int lane) {
  const float4* p = reinterpret_cast<const float4*>(bp) + lane * 4;
  f32x16 acc;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    float4 v = p[g];
    acc[4 * g + 0] = v.x;
    acc[4 * g + 1] = v.y;
    acc[4 * g + 2] = v.z;
    acc[4 * g + 3] = v.w;
  }
  return acc;
}

__device__ inline f32x16 relu_bias16(f32x16 v, f32x16 b) {
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = fmaxf(v[i] + b[i], 0.0f);
  return v;
}

// One 32-row output tile of a 128-wide layer for RT row tiles at once: 16 stream steps, each
// weight fragment feeding 4 MFMAs per row tile.  F0 = index of the tile's first step in the
// W2|W4|W6 stream (compile time => static ring slots / registers).
template <int F0, int RT>
__device__ inline void dense_tile(const float4* __restrict__ wstream, float4 (&ring)[RING],
                                  const f32x16 (&Hin)[RT][HT], f32x16 (&res)[RT]) {
  // two accumulator chains per row tile (even / odd k-steps): consecutive MFMAs never depend on
  // each other
  f32x16 acc[RT], acc1[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    acc[t] = lnz::splat16(0.0f);
    acc1[t] = lnz::splat16(0.0f);
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    constexpr int D = LNZ_GAINS_DIST;
#ifdef LNZ_GAINS_PROBE_NOLOAD   // probe: the MLP without its weight stream (what do the loads cost?)
    ring[(F0 + q + D) % RING] = make_float4(0.5f, 0.25f, 0.125f, 1.0f);
#else
    ring[(F0 + q + D) % RING] = wstream[(F0 + q + D) * 64];  // over-read lands in the slack
#endif
    __builtin_amdgcn_sched_barrier(0);
    const float4 a = ring[(F0 + q) % RING];
    const int ti = q >> 2, g = q & 3;
#pragma unroll
    for (int t = 0; t < RT; ++t) acc[t] = lnz::mfma32(a.x, Hin[t][ti][4 * g + 0], acc[t]);
#pragma unroll
    for (int t = 0; t < RT; ++t) acc1[t] = lnz::mfma32(a.y, Hin[t][ti][4 * g + 1], acc1[t]);
#pragma unroll
    for (int t = 0; t < RT; ++t) acc[t] = lnz::mfma32(a.z, Hin[t][ti][4 * g + 2], acc[t]);
#pragma unroll
    for (int t = 0; t < RT; ++t) acc1[t] = lnz::mfma32(a.w, Hin[t][ti][4 * g + 3], acc1[t]);
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int t = 0; t < RT; ++t) {
#pragma unroll
    for (int i = 0; i < 16; ++i) res[t][i] = acc[t][i] + acc1[t][i];
  }
}

// D[i] (lane) += A[lane 4 ABID + i] * B[lane]: the 16-block 4x4x1 MFMA with block ABID of A
// broadcast to every block
template <int ABID>
__device__ inline f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 4, ABID, 0);
}

// Stream step Q of Linear(128 -> S) for NG groups of four output features on
// v_mfma_f32_4x4x1_16b_f32: all 16 blocks multiply the same 4 weights (A: lane & 3 = feature of
// the group, W6c image) with the activations of their own 4 eigen rows (B: lane = eigen row), one k
// per instruction.  lo / hi hold feature cd_row(r, 0) / cd_row(r, 1) of tile ti in register r for
// all 64 lanes — after the swap of lane halves, which the first pass over the steps (SWAP) does on
// its way.  The order of the sums is dense_tile's: chain acc takes .x and .z of the step, acc1 .y
// and .w, the lower-half k before the upper-half k.
template <int Q, int NG, bool SWAP>
__device__ inline void last_linear_step(const float (&wa)[2][8], f32x16 (&lo)[HT], f32x16 (&hi)[HT],
                                        f32x4 (&acc)[NG], f32x4 (&acc1)[NG]) {
  constexpr int ti = Q >> 2, g = Q & 3, v = Q >> 1, A0 = 8 * (Q & 1);
  if constexpr (SWAP) {
#pragma unroll
    for (int r = 4 * g; r < 4 * g + 4; ++r) {
      const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(lo[ti][r]),
                                                       __float_as_uint(hi[ti][r]), false, false);
      lo[ti][r] = __uint_as_float(sw[0]);
      hi[ti][r] = __uint_as_float(sw[1]);
    }
  }
#pragma unroll
  for (int n = 0; n < NG; ++n) acc[n] = mfma4<A0 + 0>(wa[n][v], lo[ti][4 * g + 0], acc[n]);
#pragma unroll
  for (int n = 0; n < NG; ++n) acc1[n] = mfma4<A0 + 4>(wa[n][v], lo[ti][4 * g + 1], acc1[n]);
#pragma unroll
  for (int n = 0; n < NG; ++n) acc[n] = mfma4<A0 + 1>(wa[n][v], hi[ti][4 * g + 0], acc[n]);
#pragma unroll
  for (int n = 0; n < NG; ++n) acc1[n] = mfma4<A0 + 5>(wa[n][v], hi[ti][4 * g + 1], acc1[n]);
#pragma unroll
  for (int n = 0; n < NG; ++n) acc[n] = mfma4<A0 + 2>(wa[n][v], lo[ti][4 * g + 2], acc[n]);
#pragma unroll
  for (int n = 0; n < NG; ++n) acc1[n] = mfma4<A0 + 6>(wa[n][v], lo[ti][4 * g + 3], acc1[n]);
#pragma unroll
  for (int n = 0; n < NG; ++n) acc[n] = mfma4<A0 + 3>(wa[n][v], hi[ti][4 * g + 2], acc[n]);
#pragma unroll
  for (int n = 0; n < NG; ++n) acc1[n] = mfma4<A0 + 7>(wa[n][v], hi[ti][4 * g + 3], acc1[n]);
  if constexpr (Q + 1 < 16) last_linear_step<Q + 1, NG, SWAP>(wa, lo, hi, acc, acc1);
}

// the A registers of two groups; wl = this lane's float of register 0 of the first in the W6c image
// (the image holds SMAX/4 groups, those beyond S zero: an even count is always there)
__device__ inline void load_last_weights(const float* __restrict__ wl, float (&wa)[2][8]) {
#pragma unroll
  for (int n = 0; n < 2; ++n) {
#pragma unroll
    for (int v = 0; v < 8; ++v) wa[n][v] = wl[(n * 8 + v) * 64];
  }
}

template <int NG, bool SWAP>
__device__ inline void last_linear_groups(const float (&wa)[2][8], f32x16 (&lo)[HT],
                                          f32x16 (&hi)[HT], f32x4 (&out)[NG]) {
  f32x4 acc[NG], acc1[NG];
#pragma unroll
  for (int n = 0; n < NG; ++n) {
    acc[n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    acc1[n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  last_linear_step<0, NG, SWAP>(wa, lo, hi, acc, acc1);
#pragma unroll
  for (int n = 0; n < NG; ++n) out[n] = acc[n] + acc1[n];
}

// this lane's outputs 4 grp .. 4 grp + 3 (+ b6), straight to its eigen row's G
__device__ inline void store_group(const f32x4 v, const int grp, const int S, const int64_t K,
                                   const float* __restrict__ b6p, float* __restrict__ Gb) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int s = 4 * grp + i;
    // b6 of feature s in the cd_row image of lnz_pack_bias_rows: register (s&3) + 4 (s>>3) of
    // lane half (s>>2) & 1
    if (s < S) Gb[s * K] = v[i] + b6p[((s >> 2) & 1) * 512 + (s & 3) + 4 * (s >> 3)];
  }
}

// rows / n_rows (optional): compact list of the (b*K + k) eigen slots that carry a Ritz pair
// (k < min(n_b, K), lnz_plan_batch) — the slots of zero-padded eigen columns are skipped: their
// gains never reach an output (the V column is zero, model/lanczos_net.py:114-117).
// One wavefront = RT 32-row tiles of eigen slots through the MLP of conv layer l (every weight
// fragment it streams feeds all RT tiles; a row's arithmetic does not depend on RT).  `row[t]` is
// this lane's eigen slot b*K + k in tile t (both lane halves hold the same 32 rows), `valid[t]`
// masks the ragged tail.
// COMPACT = false is the padded form: 4 min(S, 8) + 64 MFMAs of 32x32x2 per tile in the first and
// the last Linear.  COMPACT = true issues 4 ceil(S/2) for the first (S <= 8) and ceil(S/4) * 128
// MFMAs of 4x4x1 per WAVE for the last; the sums and their order are the same, so are the bits.
template <int RT, bool COMPACT>
__device__ __forceinline__ void gains_mlp_tiles(const float* __restrict__ D, const int (&row)[RT],
                                                const bool (&valid)[RT], const int l,
                                                const int lane, int B, int K, const DistArr& dist,
                                                int S, const float* __restrict__ mlp_pack,
                                                float* __restrict__ G) {
  const int hh = lane >> 5;
  const float* pk = mlp_pack + (int64_t)l * PACK_SIZE;
#ifdef LNZ_GAINS_PROBE_STAGGER   // probe: de-phase the waves that stream the same weights in lockstep
  for (int i = 0; i < (int)((blockIdx.x & (LNZ_GAINS_PROBE_STAGGER_N - 1)) * LNZ_GAINS_PROBE_STAGGER); ++i)
    __builtin_amdgcn_s_sleep(16);   // 16 x 64 clocks
#endif

  // start the 128-wide weight stream right away: it is independent of the first layer
  const float4* __restrict__ wstream = reinterpret_cast<const float4*>(pk + OFF_W2) + lane;
  float4 ring[RING];
#pragma unroll
  for (int f = 0; f < LNZ_GAINS_DIST; ++f) ring[f] = wstream[f * 64];

  const int steps0 = S < 8 ? S : 8;
  f32x16 h1[RT][HT], h2[RT][HT];
  if (COMPACT && S <= 8) {
    // step u carries feature 2u on lanes 0..31 and 2u + 1 on lanes 32..63 (W0c image): the
    // accumulator takes the features in the padded form's order 0, 1, 2, .., whose other k-half
    // only added 0 * 0
    const int steps = (S + 1) >> 1;
    float w0[HT][4];
#pragma unroll
    for (int ot = 0; ot < HT; ++ot) {
#pragma unroll
      for (int u = 0; u < 4; ++u) w0[ot][u] = pk[OFF_W0C + (ot * 4 + u) * 64 + lane];
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const float dval = valid[rt] ? D[row[rt]] : 0.0f;
      float feat[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        // (only the power of this lane's k-half: the same value, half the fp64 loops)
        const int p = hh ? dist.v[2 * u + 1] : dist.v[2 * u];
        feat[u] = 2 * u + hh < S ? powi(dval, p) : 0.0f;
      }
#pragma unroll
      for (int ot = 0; ot < HT; ++ot) {
        f32x16 acc = lnz::splat16(0.0f);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (u < steps) acc = lnz::mfma32(w0[ot][u], feat[u], acc);
        }
        h1[rt][ot] = relu_bias16(acc, load_bias_frag(pk + OFF_B0 + ot * 1024, lane));
      }
    }
  } else {
    // first-layer A scalars (32 per lane) and features of this lane's k-half: f = 8 hh + t
    float w0[HT][8];
#pragma unroll
    for (int ot = 0; ot < HT; ++ot) {
#pragma unroll
      for (int t = 0; t < 8; ++t) w0[ot][t] = pk[OFF_W0 + (ot * 8 + t) * 64 + lane];
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const float dval = valid[rt] ? D[row[rt]] : 0.0f;
      float feat[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) {
#ifdef LNZ_GAINS_PROBE_NOPOW    // probe: the features without the fp64 power loops
        float lo = t < S ? dval : 0.0f;
        float hi = (8 + t) < S ? dval : 0.0f;
#else
        float lo = t < S ? powi(dval, dist.v[t]) : 0.0f;
        float hi = (8 + t) < S ? powi(dval, dist.v[8 + t]) : 0.0f;
#endif
        feat[t] = hh ? hi : lo;
      }
      // Linear(S -> 128) + ReLU
#pragma unroll
      for (int ot = 0; ot < HT; ++ot) {
        f32x16 acc = lnz::splat16(0.0f);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          if (t < steps0) acc = lnz::mfma32(w0[ot][t], feat[t], acc);
        }
        h1[rt][ot] = relu_bias16(acc, load_bias_frag(pk + OFF_B0 + ot * 1024, lane));
      }
    }
  }
  // Linear(128 -> 128) + ReLU, twice (stream steps 0..63 and 64..127), then Linear(128 -> S)
  f32x16 res[RT];
#define LNZ_DENSE(F0, IN, OUT, OT, BOFF)                                   \
  {                                                                        \
    const f32x16 bb = load_bias_frag(pk + (BOFF), lane);                   \
    dense_tile<F0, RT>(wstream, ring, IN, res);                            \
    _Pragma("unroll") for (int rt = 0; rt < RT; ++rt) OUT[rt][OT] = relu_bias16(res[rt], bb); \
  }
  LNZ_DENSE(0, h1, h2, 0, OFF_B2 + 0 * 1024)
  LNZ_DENSE(16, h1, h2, 1, OFF_B2 + 1 * 1024)
  LNZ_DENSE(32, h1, h2, 2, OFF_B2 + 2 * 1024)
  LNZ_DENSE(48, h1, h2, 3, OFF_B2 + 3 * 1024)
  LNZ_DENSE(64, h2, h1, 0, OFF_B4 + 0 * 1024)
  LNZ_DENSE(80, h2, h1, 1, OFF_B4 + 1 * 1024)
  LNZ_DENSE(96, h2, h1, 2, OFF_B4 + 2 * 1024)
  // (the last Linear's first A registers: in flight under the last dense tile)
  const float* wl = pk + OFF_W6C + lane;
  float wa0[2][8];
  if constexpr (COMPACT) load_last_weights(wl, wa0);
  LNZ_DENSE(112, h2, h1, 3, OFF_B4 + 3 * 1024)
#undef LNZ_DENSE
  if constexpr (COMPACT) {
    // (a use here keeps the compiler from sinking the loads into the branches below)
#pragma unroll
    for (int n = 0; n < 2; ++n) {
#pragma unroll
      for (int v = 0; v < 8; ++v) asm volatile("" : "+v"(wa0[n][v]));
    }
  }
  if constexpr (COMPACT) {
    static_assert(RT <= 2, "one lane half per tile");
    // B operands: the upper lane half of tile 0's register swaps with the lower half of the last
    // tile's, in place (h1 is dead).  One tile: with its own copy — lanes 32..63 then repeat
    // lanes 0..31 and are dropped.
    f32x16 self[HT];
    if constexpr (RT == 1) {
#pragma unroll
      for (int ti = 0; ti < HT; ++ti) self[ti] = h1[0][ti];
    }
    f32x16(&lo)[HT] = h1[0];
    f32x16(&hi)[HT] = *(RT == 1 ? &self : &h1[RT - 1]);
    const int mine = RT == 2 ? hh : 0;
    const bool ok = RT == 2 ? valid[mine] : (valid[0] && hh == 0);
    const int myrow = row[mine];
    const int b = myrow / K, k = myrow - b * K;
    float* Gb = G + (((int64_t)l * B + b) * S) * K + k;
    const int ng = (S + 3) >> 2;
    // two groups at a time: four independent chains
    auto pass = [&](auto swap, const float (&wa)[2][8], const int g0) {
      if (g0 + 1 < ng) {
        f32x4 o[2];
        last_linear_groups<2, decltype(swap)::value>(wa, lo, hi, o);
        if (ok) {
          store_group(o[0], g0, S, K, pk + OFF_B6, Gb);
          store_group(o[1], g0 + 1, S, K, pk + OFF_B6, Gb);
        }
      } else {
        f32x4 o[1];
        last_linear_groups<1, decltype(swap)::value>(wa, lo, hi, o);
        if (ok) store_group(o[0], g0, S, K, pk + OFF_B6, Gb);
      }
    };
    pass(std::true_type{}, wa0, 0);
    if (ng > 2) {
      float wa2[2][8];
      load_last_weights(wl + 2 * 512, wa2);
      pass(std::false_type{}, wa2, 2);
    }
  } else {
    const f32x16 b6 = load_bias_frag(pk + OFF_B6, lane);
    dense_tile<128, RT>(wstream, ring, h1, res);  // no activation (stream steps 128..143)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      if (valid[rt]) {
        const int b = row[rt] / K, k = row[rt] - b * K;
        float* Gb = G + (((int64_t)l * B + b) * S) * K + k;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int sidx = lnz::cd_row(r, hh);
          if (sidx < S) Gb[(int64_t)sidx * K] = res[rt][r] + b6[r];
        }
      }
    }
  }
}

template <bool COMPACT>
__device__ __forceinline__ void gains_mlp_tile(const float* __restrict__ D, const int row,
                                               const bool valid, const int l, const int lane,
                                               int B, int K, const DistArr& dist, int S,
                                               const float* __restrict__ mlp_pack,
                                               float* __restrict__ G) {
  const int rows1[1] = {row};
  const bool valid1[1] = {valid};
  gains_mlp_tiles<1, COMPACT>(D, rows1, valid1, l, lane, B, K, dist, S, mlp_pack, G);
}

}  // namespace lnz_gains
