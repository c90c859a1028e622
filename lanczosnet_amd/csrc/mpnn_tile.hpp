// The edge-network message block of the MPNN forward (mpnn.hip) and of one step of its backward
// (mpnn_grad.hip, which recomputes the step with the forward's arithmetic), written once: [P_c | Q_c], R_c
// and M_c of one channel on a tile of ggnn_tile.hpp.  What stands here is the arithmetic both kernels
// promise to share to the bit: change it here or nowhere.
#pragma once
#include "common.hpp"
#include "ggnn_tile.hpp"

namespace {

constexpr int MHID = 64;        // message hidden width (model/mpnn.py:60-62)
constexpr int RS = MHID + 4;    // row stride of R_c (floats)

// The LDS blocks of a tile that the message block works on: S, M_c [16 RT][D + 4], [P_c | Q_c] [16 RT][132],
// R_c [16 RT][68], bits and degrees [8][16 RT], rowbase [16 RT]
struct EdgeTile {
  const float* Sb;
  float *Mb, *Hb, *Rb;
  const unsigned* bits;
  const float* deg;
  const int* rowbase;
};

// Hb [row] = [P_c 0..63 | Q_c + b1_c 64..127], by the whole workgroup: ONE 128-column product, wave w the 16
// columns 16 w .. — waves 0 .. 3 the neighbour half of the rows of W1_c [64, 2 D] (columns 0 .. D-1 of the rows
// 16 w ..), waves 4 .. 7 the own half (columns D .. of the rows 16 (w - 4) ..).  No barrier.
template <int D, int RT>
__device__ __forceinline__ void edge_hidden(const EdgeTile t, const int c, const float* __restrict__ W1,
                                            const float* __restrict__ b1, const int wave, const int m,
                                            const int g) {
  constexpr int SS = D + 4, DB = D / 16;
  const int f0 = 16 * wave + 4 * g;
  const int hrow = 16 * (wave & 3) + m;
  const int hoff = wave < 4 ? 0 : D;
  f32x4 h[1][RT];
  zero_tiles(h);
  const float* const wp[1] = {W1 + ((int64_t)c * MHID + hrow) * (2 * D) + hoff + 4 * g};
  tile_gemm<1, DB, RT>(t.Sb + m * SS + 4 * g, SS, wp, h);
  f32x4 bv = {0.0f, 0.0f, 0.0f, 0.0f};
  if (wave >= 4) bv = *reinterpret_cast<const f32x4*>(b1 + c * MHID + 16 * (wave - 4) + 4 * g);
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) *reinterpret_cast<f32x4*>(t.Hb + (16 * rt + m) * HS + f0) = h[0][rt] + bv;
}

// Channel c of a step, by the whole workgroup: [P_c | Q_c] (edge_hidden), R_c[a] = sum over the set bits b of
// relu(Q_c[a] + P_c[b]) (four hidden columns of one row per task, b ascending), M_c = R_c W2_c^T + deg_c b2_c
// [/ (deg_c + EPS)] (owner waves: features 16 w ..).  A barrier after each.  with_r(r, q, s) sees the hidden
// columns 4 q .. of row r of R_c, with_m(rt, v) this lane's four features of row 16 rt + m of M_c, as they are
// stored: the backward keeps them, the forward passes nothing.
template <int D, int RT, class FR, class FM>
__device__ __forceinline__ void edge_message(const EdgeTile t, const int c, const float* __restrict__ W1,
                                             const float* __restrict__ b1, const float* __restrict__ W2,
                                             const float* __restrict__ b2, const int avg, const int wave,
                                             const int m, const int g, FR&& with_r, FM&& with_m) {
  constexpr int GR = 16 * RT, SS = D + 4, DB = D / 16, HQ = MHID / 4;
  const int f0 = 16 * wave + 4 * g;
  edge_hidden<D, RT>(t, c, W1, b1, wave, m, g);
  __syncthreads();
  for (int idx = threadIdx.x; idx < GR * HQ; idx += GNT) {
    const int r = idx / HQ, q = idx - r * HQ;
    unsigned bm = t.bits[c * GR + r];
    const f32x4 qv = *reinterpret_cast<const f32x4*>(t.Hb + r * HS + MHID + 4 * q);
    const float* const src = t.Hb + t.rowbase[r] * HS + 4 * q;
    f32x4 s = {0.0f, 0.0f, 0.0f, 0.0f};
    while (bm) {
      const int j = __ffs(bm) - 1;
      bm &= bm - 1;
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + j * HS);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] += fmaxf(qv[e] + v[e], 0.0f);
    }
    *reinterpret_cast<f32x4*>(t.Rb + r * RS + 4 * q) = s;
    with_r(r, q, s);
  }
  __syncthreads();
  if (wave < DB) {
    f32x4 mm[1][RT];
    zero_tiles(mm);
    const float* const wp[1] = {W2 + ((int64_t)c * D + 16 * wave + m) * MHID + 4 * g};
    tile_gemm<1, MHID / 16, RT>(t.Rb + m * RS + 4 * g, RS, wp, mm);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(b2 + c * D + f0);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const float dg = t.deg[c * GR + 16 * rt + m];
      f32x4 v = mm[0][rt] + dg * bv;
      if (avg) v = v / (dg + FLT_EPSILON);   // model/mpnn.py:172-177: the sum, then the division
      *reinterpret_cast<f32x4*>(t.Mb + (16 * rt + m) * SS + f0) = v;
      with_m(rt, v);
    }
  }
  __syncthreads();
}

}  // namespace
