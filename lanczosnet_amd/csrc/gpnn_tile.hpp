// What the GPNN forward (gpnn.hip) adds to the gated-propagation tile of ggnn_tile.hpp: the partition graphs'
// weights, the value-weighted aggregate, the partition step and the state MLP.  Everything else of a GPNN step
// (tile_gemm, the prologue, message_mlp, the gates, the GRU cell, LNZ_GGNN_TILE_STEP, the readout, the state store,
// the envelope) is ggnn_tile.hpp's.
#pragma once
#include "ggnn_tile.hpp"

namespace {

constexpr int GSH = 512;              // hidden width of state_func (model/gpnn.py:68-72)
constexpr int GSCH = GSH / GHID;      // its 128-column chunks through the H block

// wts[p][row][j], p = 0 cluster, 1 cut: the weight of column j in the row's aggregate, read once from Lp
// (element (b, i, j) at b sb + i sr + j sc floats), by value.  'sum': Lp[i, j].  'avg' (model/gpnn.py:202-203):
// Lp[i, j] / (sum_j Lp[i, j] + FLT_EPSILON), the row sum taken j ascending in float32.  Zeros beyond N and on
// the dead rows of the tile.
template <int RT>
__device__ __forceinline__ void load_partition_weights(float* wts, const float* __restrict__ Lcl, const int64_t cl_b,
                                                       const int64_t cl_r, const int64_t cl_c,
                                                       const float* __restrict__ Lct, const int64_t ct_b,
                                                       const int64_t ct_r, const int64_t ct_c, const TileSpan ts,
                                                       const int N, const int avg) {
  constexpr int GR = 16 * RT;
  for (int idx = threadIdx.x; idx < 2 * GR; idx += GNT) {
    const int p = idx / GR, r = idx - p * GR;
    float* const w = wts + (p * GR + r) * GMAXN;
    if (r < ts.rows) {
      const int ml = r / N, i = r - ml * N;
      const float* const Lr = p == 0 ? Lcl + (ts.mol0 + ml) * cl_b + i * cl_r : Lct + (ts.mol0 + ml) * ct_b + i * ct_r;
      const int64_t sc = p == 0 ? cl_c : ct_c;
      float sum = 0.0f;
      for (int j = 0; j < N; ++j) {
        const float v = Lr[j * sc];
        w[j] = v;
        sum += v;
      }
      if (avg) {
        const float denom = sum + FLT_EPSILON;
        for (int j = 0; j < N; ++j) w[j] = w[j] / denom;
      }
      for (int j = N; j < GMAXN; ++j) w[j] = 0.0f;
    } else {
      for (int j = 0; j < GMAXN; ++j) w[j] = 0.0f;
    }
  }
}

// dst = src for two state tiles [16 RT][D + 4]
template <int D, int RT>
__device__ __forceinline__ void copy_state_tile(float* dst, const float* src) {
  constexpr int Q = 16 * RT * (D + 4) / 4;
  for (int idx = threadIdx.x; idx < Q; idx += GNT)
    reinterpret_cast<f32x4*>(dst)[idx] = reinterpret_cast<const f32x4*>(src)[idx];
}

// A = Ŵ M per molecule with the row's N weights w[row][j] from LDS: four features of one row per task,
// j ascending, fmaf (a zero weight is a term like any other: Lp enters by value).  A dead row gets zeros.
// A barrier behind it.
template <int D, int RT>
__device__ __forceinline__ void weighted_aggregate(float* Ab, const float* Mb, const float* w, const int* rowbase,
                                                   const int N, const int rows) {
  constexpr int GR = 16 * RT, SS = D + 4, DQ = D / 4;
  for (int idx = threadIdx.x; idx < GR * DQ; idx += GNT) {
    const int r = idx / DQ, q = idx - r * DQ;
    f32x4 s = {0.0f, 0.0f, 0.0f, 0.0f};
    if (r < rows) {
      const float* const src = Mb + rowbase[r] * SS + 4 * q;
      const float* const wr = w + r * GMAXN;
      for (int j = 0; j < N; ++j) {
        const float wgt = wr[j];
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + j * SS);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] = fmaf(wgt, v[e], s[e]);
      }
    }
    *reinterpret_cast<f32x4*>(Ab + r * SS + 4 * q) = s;
  }
  __syncthreads();
}

// One partition step in place on the state tile Sb (model/gpnn.py:192-213): M = msg_func[0](S) (message_mlp on
// channel 0's weights: no bit-mask aggregate behind it), A = Ŵ M,
// S' = GRUCell_partition(A, S) with Wih [3 D][D] (gate_accumulate with C = 1, c = 0 is the cell's gi).
// On entry Sb is complete behind a barrier and M, A, H are free; on exit the same holds.
template <int D, int RT>
__device__ __forceinline__ void partition_step(float* Sb, float* Mb, float* Ab, float* Hb, const float* w,
                                               const int* rowbase, const int N, const int rows,
                                               const float* __restrict__ W1, const float* __restrict__ b1,
                                               const float* __restrict__ W2, const float* __restrict__ b2,
                                               const float* __restrict__ Wih, const float* __restrict__ bih,
                                               const float* __restrict__ Whh, const float* __restrict__ bhh,
                                               const int wave, const int m, const int g) {
  constexpr int SS = D + 4;
  const bool owner = wave < D / 16;
  message_mlp<D, RT>(Sb, Mb, Hb, W1, b1, W2, b2, wave, m, g, NoHook{});
  weighted_aggregate<D, RT>(Ab, Mb, w, rowbase, N, rows);
  f32x4 acc[3][RT], gh[3][RT];
  if (owner) {
    zero_tiles(acc);
    gate_accumulate<D, RT>(Ab + m * SS + 4 * g, Wih, 0, 1, wave, m, g, acc);
    hidden_gates<D, RT>(Sb + m * SS + 4 * g, Whh, wave, m, g, gh);
  }
  __syncthreads();
  if (owner) LNZ_GRU_CELL(D, RT);
  __syncthreads();
}

// S = relu([S | Sc | Sx] Ws1^T + bs1) Ws2^T + bs2 in place on Sb (model/gpnn.py:227-228; Ws1 [512][3 D],
// Ws2 [D][512]).  The [rows, 512] hidden goes through the H block in four 128-column chunks: wave w owns the 16
// hidden columns 128 k + 16 w .. of chunk k — one chain of 3 D terms over the three LDS tiles, S first — then the
// owner waves take a chain of 128 terms of their own per chunk and add the chunks in ascending order.  Sc / Sx
// may be Sb itself (a partition count of 0).  On entry the three tiles are complete behind a barrier and H is
// free; on exit Sb is complete behind a barrier.
template <int D, int RT>
__device__ __forceinline__ void state_mlp(float* Sb, const float* Scb, const float* Sxb, float* Hb,
                                          const float* __restrict__ Ws1, const float* __restrict__ bs1,
                                          const float* __restrict__ Ws2, const float* __restrict__ bs2,
                                          const int wave, const int m, const int g) {
  constexpr int SS = D + 4, DB = D / 16;
  const bool owner = wave < DB;
  const int f0 = 16 * wave + 4 * g, at = m * SS + 4 * g;
  f32x4 out[1][RT];
  zero_tiles(out);
  for (int k = 0; k < GSCH; ++k) {
    {
      f32x4 h[1][RT];
      zero_tiles(h);
      const float* const row = Ws1 + (int64_t)(GHID * k + 16 * wave + m) * (3 * D) + 4 * g;
      const float* const w0[1] = {row};
      const float* const w1[1] = {row + D};
      const float* const w2[1] = {row + 2 * D};
      tile_gemm<1, DB, RT>(Sb + at, SS, w0, h);
      tile_gemm<1, DB, RT>(Scb + at, SS, w1, h);
      tile_gemm<1, DB, RT>(Sxb + at, SS, w2, h);
      const f32x4 bv = *reinterpret_cast<const f32x4*>(bs1 + GHID * k + f0);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(h[0][rt][e] + bv[e], 0.0f);
        *reinterpret_cast<f32x4*>(Hb + (16 * rt + m) * HS + f0) = v;
      }
    }
    __syncthreads();
    if (owner) {
      f32x4 part[1][RT];
      zero_tiles(part);
      const float* const wp[1] = {Ws2 + (int64_t)(16 * wave + m) * GSH + GHID * k + 4 * g};
      tile_gemm<1, GHID / 16, RT>(Hb + m * HS + 4 * g, HS, wp, part);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) out[0][rt] += part[0][rt];
    }
    __syncthreads();   // H is read; after the last chunk every read of the three tiles lies behind it too
  }
  if (owner) {
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bs2 + f0);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) *reinterpret_cast<f32x4*>(Sb + (16 * rt + m) * SS + f0) = out[0][rt] + bv;
  }
  __syncthreads();
}

}  // namespace
