// The gated-propagation tile of the GGNN forward (ggnn.hip), of one step of its backward (ggnn_grad.hip,
// which recomputes the step with the forward's arithmetic), of the MPNN forward and backward step (mpnn.hip,
// mpnn_grad.hip) and of the GPNN forward (gpnn.hip): the envelope, the MFMA tile product, the prologue, the
// message MLP and the GGNN message block, the gates, the GRU cell, the whole GGNN step, the gated readout, the
// cell's backward and the state store, each written once.  What stands here is the arithmetic these kernels
// promise to share to the bit: change it here or nowhere.
#pragma once
#include <float.h>
#include <stdio.h>

#include "common.hpp"

namespace {

constexpr int GHID = 128;      // message hidden width (model/ggnn.py:59-61)
constexpr int GNW = 8;         // waves per workgroup
constexpr int GNT = 64 * GNW;  // threads
constexpr int GMAXN = 32, GMAXC = 8, GMAXP = 16, GMAXD = 128;
constexpr int HS = GHID + 4;   // row stride of H_c (floats): 16-byte rows, fragment reads spread over the banks

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// acc[t][rt] += (16 RT rows of the LDS operand, K = 16 KB columns) x (16 weight rows of tile t)^T.
// `as` = the operand's row (lane & 15) + 4 (lane >> 4) floats; wp[t] = the weight row of this lane
// + 4 (lane >> 4) floats.  Lane (m, g) multiplies k = 16 kb + 4 g + u in MFMA step u on both operands;
// register e of acc[t][rt] is row 16 rt + m, feature (tile base) + 4 g + e.  The weight fragments are
// loaded PF blocks ahead of the MFMAs that use them.
template <int NT, int KB, int RT>
__device__ __forceinline__ void tile_gemm(const float* as, const int lda, const float* const (&wp)[NT],
                                          f32x4 (*acc)[RT]) {
  constexpr int PF0 = NT >= 3 ? 2 : 4, PF = KB < PF0 ? KB : PF0;
  f32x4 w[KB][NT];
#pragma unroll
  for (int kb = 0; kb < PF; ++kb)
#pragma unroll
    for (int t = 0; t < NT; ++t) w[kb][t] = *reinterpret_cast<const f32x4*>(wp[t] + 16 * kb);
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    f32x4 a[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) a[rt] = *reinterpret_cast<const f32x4*>(as + 16 * rt * lda + 16 * kb);
    if (kb + PF < KB) {
#pragma unroll
      for (int t = 0; t < NT; ++t) w[kb + PF][t] = *reinterpret_cast<const f32x4*>(wp[t] + 16 * (kb + PF));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[t][rt] = mfma16(w[kb][t][u], a[rt][u], acc[t][rt]);
  }
}

template <int NT, int RT>
__device__ __forceinline__ void zero_tiles(f32x4 (&acc)[NT][RT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[t][rt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---------------------------------------------------------------------------------------- the prologue
// A workgroup's tile: floor(16 RT / N) whole molecules from mol0 on, packed densely; `rows` of its 16 RT
// rows are live, the others stay zero and unread.
struct TileSpan {
  int64_t mol0;
  int nm, rows;
};

template <int RT>
__device__ __forceinline__ TileSpan tile_span(const int B, const int N) {
  const int mpt = 16 * RT / N;                             // molecules per tile
  const int64_t mol0 = (int64_t)blockIdx.x * mpt;
  const int nm = (int)(B - mol0 < mpt ? B - mol0 : mpt);   // molecules of this tile
  return {mol0, nm, nm * N};
}

// Sb [16 RT][D + 4] = the tile's rows of the state (row0 = its first global row), zeros beyond `rows`
template <int D, int RT>
__device__ __forceinline__ void load_state_tile(float* Sb, const float* __restrict__ state, const int64_t row0,
                                                const int ld, const int rows) {
  constexpr int SS = D + 4, DQ = D / 4;
  for (int idx = threadIdx.x; idx < 16 * RT * DQ; idx += GNT) {
    const int r = idx / DQ, q = idx - r * DQ;
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (r < rows) v = *reinterpret_cast<const f32x4*>(state + (row0 + r) * (int64_t)ld + 4 * q);
    *reinterpret_cast<f32x4*>(Sb + r * SS + 4 * q) = v;
  }
}

// bits[c][row] = the row of L's channel c as a bit mask (bit j: L[row, j, c] != 0; NaN != 0: an edge), L read
// once through its four strides; with_degree(c 16 RT + row, popcount) leaves what the caller keeps of the
// degree (GGNN: the 'avg' reciprocal, MPNN: the degree itself)
template <int RT, class F>
__device__ __forceinline__ void load_edge_bits(unsigned* bits, const float* __restrict__ L, const int64_t stride_b,
                                               const int64_t stride_r, const int64_t stride_c,
                                               const int64_t stride_ch, const TileSpan ts, const int N,
                                               const int C, F&& with_degree) {
  constexpr int GR = 16 * RT;
  for (int idx = threadIdx.x; idx < GR * C; idx += GNT) {
    const int r = idx / C, c = idx - r * C;
    unsigned bm = 0;
    if (r < ts.rows) {
      const int ml = r / N, i = r - ml * N;
      const float* Lr = L + (ts.mol0 + ml) * stride_b + i * stride_r + c * stride_ch;
      for (int j = 0; j < N; ++j) bm |= (Lr[j * stride_c] != 0.0f ? 1u : 0u) << j;
    }
    bits[c * GR + r] = bm;
    with_degree(c * GR + r, __popc(bm));
  }
}

// model/ggnn.py:156-157: every entry of the row is 1 / (degree + EPS), in float32
__device__ __forceinline__ float ggnn_edge_weight(const int avg, const int degree) {
  return avg ? 1.0f / ((float)degree + FLT_EPSILON) : 1.0f;
}

// rowbase[row] = the first row of the row's molecule
template <int RT>
__device__ __forceinline__ void set_rowbase(int* rowbase, const int N, const int rows) {
  const int tid = threadIdx.x;
  if (tid < 16 * RT) rowbase[tid] = tid < rows ? (tid / N) * N : 0;
}

// ------------------------------------------------------------------------------- the GGNN message block
// The LDS blocks of a tile that the message block works on: S, M_c, A_c [16 RT][D + 4], H_c [16 RT][132],
// bits and weights [8][16 RT], rowbase [16 RT]
struct MessageTile {
  const float* Sb;
  float *Mb, *Ab, *Hb;
  const unsigned* bits;
  const float* inv;
  const int* rowbase;
};

// A hook that keeps nothing: what the forwards pass where the backward keeps H_c and A_c
struct NoHook {
  template <class... A>
  __device__ __forceinline__ void operator()(A&&...) const {}
};

// M = relu(X W1^T + b1) W2^T + b2 for one message function (W1 [128][D], b1 [128], W2 [D][128], b2 [D]) by the
// whole workgroup:  H = relu(X W1^T + b1) into Hb (wave w: hidden columns 16 w ..), M = H W2^T + b2 into Mb
// (owner waves: features 16 w ..).  A barrier after each half.  with_h(rt, v) sees this lane's four hidden
// values of row 16 rt + m as they are stored.
template <int D, int RT, class FH>
__device__ __forceinline__ void message_mlp(const float* Xb, float* Mb, float* Hb, const float* __restrict__ W1,
                                            const float* __restrict__ b1, const float* __restrict__ W2,
                                            const float* __restrict__ b2, const int wave, const int m, const int g,
                                            FH&& with_h) {
  constexpr int SS = D + 4, DB = D / 16;
  const int f0 = 16 * wave + 4 * g;
  {
    f32x4 h[1][RT];
    zero_tiles(h);
    const float* const wp[1] = {W1 + (int64_t)(16 * wave + m) * D + 4 * g};
    tile_gemm<1, DB, RT>(Xb + m * SS + 4 * g, SS, wp, h);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(b1 + f0);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaxf(h[0][rt][e] + bv[e], 0.0f);
      *reinterpret_cast<f32x4*>(Hb + (16 * rt + m) * HS + f0) = v;
      with_h(rt, v);
    }
  }
  __syncthreads();
  if (wave < DB) {
    f32x4 mm[1][RT];
    zero_tiles(mm);
    const float* const wp[1] = {W2 + (int64_t)(16 * wave + m) * GHID + 4 * g};
    tile_gemm<1, GHID / 16, RT>(Hb + m * HS + 4 * g, HS, wp, mm);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(b2 + f0);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) *reinterpret_cast<f32x4*>(Mb + (16 * rt + m) * SS + f0) = mm[0][rt] + bv;
  }
  __syncthreads();
}

// Channel c of a step, by the whole workgroup:  M_c = message_mlp of channel c's weights on S, then A_c = Â_c M_c
// (four features of one row per task, the set bits of the row in ascending j) and a barrier.  with_h: message_mlp's;
// with_a(r, q, s) sees the features 4 q .. of row r of A_c as they are stored: the backward keeps them, the
// forward passes NoHook.
template <int D, int RT, class FH, class FA>
__device__ __forceinline__ void ggnn_message(const MessageTile t, const int c, const float* __restrict__ W1,
                                             const float* __restrict__ b1, const float* __restrict__ W2,
                                             const float* __restrict__ b2, const int wave, const int m,
                                             const int g, FH&& with_h, FA&& with_a) {
  constexpr int GR = 16 * RT, SS = D + 4, DQ = D / 4;
  message_mlp<D, RT>(t.Sb, t.Mb, t.Hb, W1 + (int64_t)c * GHID * D, b1 + c * GHID, W2 + (int64_t)c * D * GHID,
                     b2 + c * D, wave, m, g, with_h);
  for (int idx = threadIdx.x; idx < GR * DQ; idx += GNT) {
    const int r = idx / DQ, q = idx - r * DQ;
    unsigned bm = t.bits[c * GR + r];
    const float wgt = t.inv[c * GR + r];
    const float* const src = t.Mb + t.rowbase[r] * SS + 4 * q;
    f32x4 s = {0.0f, 0.0f, 0.0f, 0.0f};
    while (bm) {
      const int j = __ffs(bm) - 1;
      bm &= bm - 1;
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + j * SS);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] = fmaf(wgt, v[e], s[e]);
    }
    *reinterpret_cast<f32x4*>(t.Ab + r * SS + 4 * q) = s;
    with_a(r, q, s);
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------- the gates and the cell
// gi += X_c W_ih[:, c D ..]^T for an owner wave (16 wave < D): tiles [0] r, [1] z, [2] gi_n of its features.
// frag = the wave's fragment of X_c [16 RT][D + 4].  A chain of D terms per channel, then one add: the error
// of a short sum.
template <int D, int RT>
__device__ __forceinline__ void gate_accumulate(const float* frag, const float* __restrict__ Wih, const int c,
                                                const int C, const int wave, const int m, const int g,
                                                f32x4 (&acc)[3][RT]) {
  const float* const row = Wih + (int64_t)(16 * wave + m) * ((int64_t)C * D) + c * D + 4 * g;
  const int64_t gate = (int64_t)D * C * D;
  const float* const wp[3] = {row, row + gate, row + 2 * gate};
  f32x4 part[3][RT];
  zero_tiles(part);
  tile_gemm<3, D / 16, RT>(frag, D + 4, wp, part);
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[t][rt] += part[t][rt];
}

// gh = S W_hh^T for an owner wave, the state still the step's input: r and z join gi, gh_n stays apart.
// Every wave reads ALL columns of S here: a barrier stands between this and the cell's writes.
template <int D, int RT>
__device__ __forceinline__ void hidden_gates(const float* s_frag, const float* __restrict__ Whh, const int wave,
                                             const int m, const int g, f32x4 (&gh)[3][RT]) {
  zero_tiles(gh);
  const int64_t at = (int64_t)(16 * wave + m) * D + 4 * g;   // this lane's fragment in a gate's [D, D] block
  const float* const wp[3] = {Whh + at, Whh + D * D + at, Whh + 2 * D * D + at};
  tile_gemm<3, D / 16, RT>(s_frag, D + 4, wp, gh);
}

// The biases of this lane's four features f0 ..: r and z take b_ih + b_hh, n keeps the two apart
struct GruBias {
  f32x4 r, z, in, hn;
};

template <int D>
__device__ __forceinline__ GruBias gru_bias(const float* __restrict__ bih, const float* __restrict__ bhh,
                                            const int f0) {
  return {*reinterpret_cast<const f32x4*>(bih + f0) + *reinterpret_cast<const f32x4*>(bhh + f0),
          *reinterpret_cast<const f32x4*>(bih + D + f0) + *reinterpret_cast<const f32x4*>(bhh + D + f0),
          *reinterpret_cast<const f32x4*>(bih + 2 * D + f0), *reinterpret_cast<const f32x4*>(bhh + 2 * D + f0)};
}

// The forward expressions of the cell for one element: the gates r, z and the candidate n
__device__ __forceinline__ float gru_gate(const float gi, const float gh, const float b) {
  return sigmoidf_((gi + gh) + b);
}
__device__ __forceinline__ float gru_candidate(const float gi_n, const float b_in, const float r, const float ghn) {
  return tanhf((gi_n + b_in) + r * ghn);
}

// The GRU cell on an owner wave's features, S' = (1 - z) n + z S in place, from the kernel's Sb, bih, bhh, wave,
// m, g, acc and gh.  A macro, not a function: the cell's products and sums are contracted by the compiler, and as
// an inlined function the vectoriser paired half of a row tile's elements differently from the other half
// (z S and (1 - z) n multiplied as a pair, then added unfused), so a row's bits came to depend on the tile height
// (measured: tests/test_gpu_ggnn.py failed its tile-height equality at D = 128).  Pasted text compiles to the
// cell both forwards always had.
#define LNZ_GRU_CELL(D, RT)                                                                  \
  do {                                                                                       \
    const int f0_ = 16 * wave + 4 * g;                                                       \
    const GruBias b_ = gru_bias<D>(bih, bhh, f0_);                                           \
    _Pragma("unroll") for (int rt = 0; rt < RT; ++rt) {                                      \
      float* const sp = Sb + (16 * rt + m) * (D + 4) + f0_;                                  \
      const f32x4 so = *reinterpret_cast<const f32x4*>(sp);                                  \
      f32x4 sn;                                                                              \
      _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                        \
        const float r = gru_gate(acc[0][rt][e], gh[0][rt][e], b_.r[e]);                      \
        const float z = gru_gate(acc[1][rt][e], gh[1][rt][e], b_.z[e]);                      \
        const float n = gru_candidate(acc[2][rt][e], b_.in[e], r, gh[2][rt][e] + b_.hn[e]);  \
        sn[e] = (1.0f - z) * n + z * so[e];                                                  \
      }                                                                                      \
      *reinterpret_cast<f32x4*>(sp) = sn;                                                    \
    }                                                                                        \
  } while (0)

// One GGNN step in place on the kernel's state tile Sb (= mt.Sb) by the whole workgroup: per channel the message
// block and the owner waves' gate product (three barriers per channel), gh = S W_hh^T, a barrier, the cell, a
// barrier.  On entry Sb is complete behind a barrier and M, A, H are free; on exit the same holds.  The forwards'
// step (ggnn.hip, gpnn.hip); ggnn_grad.hip keeps a loop of its own, with hooks and the backward in between.  From
// the MessageTile and the message and cell weights given and the kernel's Sb, wave, m, g.  A macro like
// LNZ_GRU_CELL: as an inlined function the step left every digest where it was but got another register
// allocation in ggnn.hip (ggnn_forward_kernel<128, 2> 165 -> 127 VGPRs) and the launch ran 9 % (B = 64) and 3 %
// (B = 1024) longer at the yaml shape; pasted, ggnn.hip keeps its registers and its time.
#define LNZ_GGNN_TILE_STEP(D, RT, mt, W1, b1, W2, b2, Wih, bih_, Whh, bhh_, C)                               \
  do {                                                                                                       \
    const float* const lnz_bih_ = (bih_);                                                                    \
    const float* const lnz_bhh_ = (bhh_);                                                                    \
    {                                                                                                        \
      const float* const bih = lnz_bih_; /* the names LNZ_GRU_CELL reads */                                  \
      const float* const bhh = lnz_bhh_;                                                                     \
      const bool owner = wave < D / 16; /* wave-uniform: this wave owns features 16 wave .. 16 wave + 15 */  \
      f32x4 acc[3][RT]; /* gate accumulators of this wave's feature block: [0] r, [1] z, [2] gi_n */         \
      zero_tiles(acc);                                                                                       \
      for (int c = 0; c < C; ++c) {                                                                          \
        ggnn_message<D, RT>(mt, c, W1, b1, W2, b2, wave, m, g, NoHook{}, NoHook{});                          \
        if (owner) gate_accumulate<D, RT>((mt).Ab + m * (D + 4) + 4 * g, Wih, c, C, wave, m, g, acc);        \
      }                                                                                                      \
      f32x4 gh[3][RT];                                                                                       \
      if (owner) hidden_gates<D, RT>(Sb + m * (D + 4) + 4 * g, Whh, wave, m, g, gh);                         \
      __syncthreads();                                                                                       \
      if (owner) LNZ_GRU_CELL(D, RT);                                                                        \
      __syncthreads();                                                                                       \
    }                                                                                                        \
  } while (0)

// The gated masked-mean readout of a tile's final state: y = (Wo s + bo) * sigmoid(wg s + bg) per live row,
// score = the mean of y over the molecule's rows with mask != 0 (all N rows without a mask).  ys [row][GMAXP + 1]
// is scratch LDS (the forwards pass the H block, dead by then): slot p < P: Wo[p] s + bo[p]; slot P:
// sigmoid(wg s + bg); d ascending.
template <int D>
__device__ __forceinline__ void gated_readout(const float* Sb, float* ys, const unsigned char* __restrict__ mask,
                                              const float* __restrict__ Wo, const float* __restrict__ bo,
                                              const float* __restrict__ wg, const float* __restrict__ bg,
                                              const TileSpan ts, const int N, const int P,
                                              float* __restrict__ score) {
  constexpr int SS = D + 4;
  const int tid = threadIdx.x;
  for (int idx = tid; idx < ts.rows * (P + 1); idx += GNT) {
    const int r = idx / (P + 1), p = idx - r * (P + 1);
    const float* const w = p < P ? Wo + (int64_t)p * D : wg;
    float a = 0.0f;
    for (int d = 0; d < D; ++d) a = fmaf(Sb[r * SS + d], w[d], a);
    a += p < P ? bo[p] : bg[0];
    ys[r * (GMAXP + 1) + p] = p < P ? a : sigmoidf_(a);
  }
  __syncthreads();
  for (int idx = tid; idx < ts.nm * P; idx += GNT) {
    const int ml = idx / P, p = idx - ml * P;
    float s = 0.0f, cnt = 0.0f;
    for (int i = 0; i < N; ++i) {
      if (mask == nullptr || mask[(ts.mol0 + ml) * N + i] != 0) {
        const int r = ml * N + i;
        s += ys[r * (GMAXP + 1) + p] * ys[r * (GMAXP + 1) + P];
        cnt += 1.0f;
      }
    }
    score[(ts.mol0 + ml) * P + p] = s / cnt;   // (no masked row: 0 / 0, the reference's mean of nothing)
  }
}

// ---------------------------------------------------------------------------------- the cell's backward
// bitsT[c][row] = the per-molecule transpose of bits: bit i = edge (i, row).  bits and rowbase complete behind a
// barrier; the caller's next barriers stand between this and the first read of bitsT.
template <int RT>
__device__ __forceinline__ void transpose_edge_bits(unsigned* bitsT, const unsigned* bits, const int* rowbase,
                                                    const int N, const int C, const int rows) {
  constexpr int GR = 16 * RT;
  for (int idx = threadIdx.x; idx < GR * C; idx += GNT) {
    const int r = idx / C, c = idx - r * C;
    unsigned bt = 0;
    if (r < rows) {
      const int base = rowbase[r], j = r - base;
      for (int i = 0; i < N; ++i) bt |= ((bits[c * GR + base + i] >> j) & 1u) << i;
    }
    bitsT[c * GR + r] = bt;
  }
}

// The GRU cell of a step recomputed and differentiated, by the whole workgroup.  From the step's input state Sb,
// the finished gate accumulators acc (gi without its bias) and dS' = dL/dS_{t+1} (dSn, the tile's rows from
// row0 on):
//     gh = S W_hh^T ; r, z, n as LNZ_GRU_CELL has them
//     dn = dS' (1 - z), dz = dS' (S - n), ds = dS' z
//     pn = dn (1 - n^2), pz = dz z (1 - z), pr = pn gh_n r (1 - r), pq = pn r
// The planes are written for every row of the tile (a dead row: dS' = 0, so zeros), dgi = [pr, pz, pn] and
// dghn = pq for the live rows; a barrier; then ds += dgh W_hh on the owner waves (feature k = row k of WhhT
// [D][3 D], the contraction over r, z, n in that order: a chain of D terms per gate, then the adds: short sums).
// ds = dS_t of this lane's four features so far; the planes are complete behind the barrier.  From the kernel's
// Sb, Pr, Pz, Pn, Pq, acc, bih, Whh, bhh, WhhT, dSn, ldd, row0, rows, dgi, dghn, wave, m, g, owner, f0, fo
// (= m SS + 4 g, the fragment offset in a plane) and ds.  A macro like LNZ_GRU_CELL, for its reason: as an
// inlined function the same text got another register allocation (ggnn_backward_step_kernel<128> 128 -> 130
// VGPRs, mpnn_backward_step_kernel<32> 122 -> 138: a wave per SIMD less in the occupancy table); pasted, both
// step kernels compile to what they were.
#define LNZ_GRU_CELL_BACKWARD(D, RT)                                                                       \
  do {                                                                                                     \
    zero_tiles(ds);                                                                                        \
    if (owner) {                                                                                           \
      f32x4 gh[3][RT];                                                                                     \
      hidden_gates<D, RT>(Sb + fo, Whh, wave, m, g, gh);                                                   \
      const GruBias b = gru_bias<D>(bih, bhh, f0);                                                         \
      _Pragma("unroll") for (int rt = 0; rt < RT; ++rt) {                                                  \
        const int rl = 16 * rt + m;                                                                        \
        const bool live = rl < rows;                                                                       \
        const f32x4 so = *reinterpret_cast<const f32x4*>(Sb + rl * SS + f0);                               \
        f32x4 dsn = {0.0f, 0.0f, 0.0f, 0.0f};                                                              \
        if (live) dsn = *reinterpret_cast<const f32x4*>(dSn + (row0 + rl) * (int64_t)ldd + f0);            \
        f32x4 pr, pz, pn, pq;                                                                              \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                    \
          const float r = gru_gate(acc[0][rt][e], gh[0][rt][e], b.r[e]);                                   \
          const float z = gru_gate(acc[1][rt][e], gh[1][rt][e], b.z[e]);                                   \
          const float ghn = gh[2][rt][e] + b.hn[e];                                                        \
          const float n = gru_candidate(acc[2][rt][e], b.in[e], r, ghn);                                   \
          const float dn = dsn[e] * (1.0f - z);                                                            \
          const float dz = dsn[e] * (so[e] - n);                                                           \
          ds[0][rt][e] = dsn[e] * z;                                                                       \
          pn[e] = dn * (1.0f - n * n);                                                                     \
          pz[e] = dz * (z * (1.0f - z));                                                                   \
          pr[e] = (pn[e] * ghn) * (r * (1.0f - r));                                                        \
          pq[e] = pn[e] * r;                                                                               \
        }                                                                                                  \
        *reinterpret_cast<f32x4*>(Pr + rl * SS + f0) = pr;                                                 \
        *reinterpret_cast<f32x4*>(Pz + rl * SS + f0) = pz;                                                 \
        *reinterpret_cast<f32x4*>(Pn + rl * SS + f0) = pn;                                                 \
        *reinterpret_cast<f32x4*>(Pq + rl * SS + f0) = pq;                                                 \
        if (live) {                                                                                        \
          float* const gp = dgi + (row0 + rl) * (int64_t)(3 * D) + f0;                                     \
          *reinterpret_cast<f32x4*>(gp) = pr;                                                              \
          *reinterpret_cast<f32x4*>(gp + D) = pz;                                                          \
          *reinterpret_cast<f32x4*>(gp + 2 * D) = pn;                                                      \
          *reinterpret_cast<f32x4*>(dghn + (row0 + rl) * (int64_t)D + f0) = pq;                            \
        }                                                                                                  \
      }                                                                                                    \
    }                                                                                                      \
    __syncthreads();                                                                                       \
    if (owner) {                                                                                           \
      const float* const row = WhhT + (int64_t)(16 * wave + m) * (3 * D) + 4 * g;                          \
      const float* const w0[1] = {row};                                                                    \
      const float* const w1[1] = {row + D};                                                                \
      const float* const w2[1] = {row + 2 * D};                                                            \
      f32x4 p0[1][RT], p1[1][RT], p2[1][RT];                                                               \
      zero_tiles(p0);                                                                                      \
      zero_tiles(p1);                                                                                      \
      zero_tiles(p2);                                                                                      \
      tile_gemm<1, DB, RT>(Pr + fo, SS, w0, p0);                                                           \
      tile_gemm<1, DB, RT>(Pz + fo, SS, w1, p1);                                                           \
      tile_gemm<1, DB, RT>(Pq + fo, SS, w2, p2);                                                           \
      _Pragma("unroll") for (int rt = 0; rt < RT; ++rt) ds[0][rt] += (p0[0][rt] + p1[0][rt]) + p2[0][rt];  \
    }                                                                                                      \
  } while (0)

// dst [rows][ld] = the live rows of Sb (dst = the tile's first row of the destination)
template <int D>
__device__ __forceinline__ void store_state_tile(float* __restrict__ dst, const int ld, const float* Sb,
                                                 const int rows) {
  constexpr int SS = D + 4, DQ = D / 4;
  for (int idx = threadIdx.x; idx < rows * DQ; idx += GNT) {
    const int r = idx / DQ, q = idx - r * DQ;
    *reinterpret_cast<f32x4*>(dst + (int64_t)r * ld + 4 * q) = *reinterpret_cast<const f32x4*>(Sb + r * SS + 4 * q);
  }
}

// ------------------------------------------------------------------------------------------ host side
inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
inline bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}
// bytes from the first to the last element of `rows` rows of `width` floats, `ld` floats apart
inline uint64_t span(uint64_t rows, int ld, int width) { return ((rows - 1) * (uint64_t)ld + width) * sizeof(float); }

inline int device_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
    (void)hipGetLastError();
    cus = 256;
  }
  return cus;
}

// tile_rows = 0: 32-row tiles while they all fit in one round of the compute units, 64-row tiles beyond
inline int choose_tile_rows(int B, int N, int tile_rows) {
  if (tile_rows != 0) return tile_rows;
  const int mpt32 = 32 / N;
  return ((int64_t)B + mpt32 - 1) / mpt32 <= device_cus() ? 32 : 64;
}

// What lnz_ggnn_forward*, lnz_mpnn_forward ask of the operands they share, after their null-pointer check:
// the envelope, the row strides, the strides of L, the alignment of the rows the kernels read as float4.
// P: the outputs of the readout, null for an entry point without one; state_out may be null where the entry
// point allows it.
inline int check_propagation(const char* who, const float* state0, int ld0, const float* state_out, int ldso,
                             int64_t stride_b, int64_t stride_r, int64_t stride_c, int64_t stride_ch,
                             const float* const (&w)[8], int B, int N, int C, int D, const int* P, int num_prop) {
  LNZ_REQUIRE(B > 0 && N > 0, LNZ_EINVAL, "%s: B = %d, N = %d must be positive", who, B, N);
  char p_is[24] = "";
  if (P) snprintf(p_is, sizeof p_is, ", P = %d", *P);
  LNZ_REQUIRE(N <= GMAXN && C >= 1 && C <= GMAXC && D >= 32 && D <= GMAXD && D % 32 == 0 &&
                  (!P || (*P >= 1 && *P <= GMAXP)) && num_prop >= 0,
              LNZ_ENOTSUP,
              "%s: N = %d, C = %d, D = %d%s, num_prop = %d outside 1 <= N <= 32, 1 <= C <= 8, "
              "D a multiple of 32 and <= 128%s, num_prop >= 0", who, N, C, D, p_is, num_prop,
              P ? ", 1 <= P <= 16" : "");
  LNZ_REQUIRE(ld0 >= D && (state_out == nullptr || ldso >= D), LNZ_EINVAL,
              "%s: ld0 = %d, ldso = %d below the width %d", who, ld0, ldso, D);
  LNZ_REQUIRE(stride_b >= 0 && stride_r >= 0 && stride_c >= 0 && stride_ch >= 0, LNZ_EINVAL,
              "%s: negative stride of L", who);
  bool weights_aligned = true;
  for (const float* p : w) weights_aligned = weights_aligned && aligned16(p);
  LNZ_REQUIRE(ld0 % 4 == 0 && (state_out == nullptr || ldso % 4 == 0) && aligned16(state0) && aligned16(state_out) &&
                  weights_aligned,
              LNZ_ENOTSUP, "%s: the rows of state0, state_out and of the weights must be 16-byte "
              "aligned (ld0 = %d, ldso = %d)", who, ld0, ldso);
  return LNZ_OK;
}

// What lnz_ggnn_forward*, lnz_gpnn_forward ask of their outputs, after check_propagation: score, state_out
// (may be null) and the trajectory `states` [num_prop + 1][B N][D] (null for an entry point without one) alias
// neither state0 nor each other, and tile_rows is 0 or a height; `heights` names the entry point's in words.
inline int check_outputs(const char* who, const float* state0, int ld0, const float* score, const float* state_out,
                         int ldso, const float* states, int B, int N, int D, int P, int num_prop, int tile_rows,
                         const char* heights) {
  const uint64_t rows = (uint64_t)B * N;
  const uint64_t n0 = span(rows, ld0, D), no = span(rows, ldso, D), nsc = (uint64_t)B * P * sizeof(float);
  LNZ_REQUIRE(!overlap(score, nsc, state0, n0), LNZ_EINVAL, "%s: score must not alias state0", who);
  LNZ_REQUIRE(state_out == nullptr || (!overlap(state_out, no, state0, n0) && !overlap(state_out, no, score, nsc)),
              LNZ_EINVAL, "%s: state_out must not alias state0 or score", who);
  if (states != nullptr) {
    const uint64_t nst = ((uint64_t)num_prop + 1) * rows * D * sizeof(float);
    LNZ_REQUIRE(aligned16(states), LNZ_ENOTSUP, "%s: states must be 16-byte aligned", who);
    LNZ_REQUIRE(!overlap(states, nst, state0, n0) && !overlap(states, nst, score, nsc) &&
                    (state_out == nullptr || !overlap(states, nst, state_out, no)),
                LNZ_EINVAL, "%s: states must not alias state0, score or state_out", who);
  }
  LNZ_REQUIRE(tile_rows == 0 || tile_rows == 32 || tile_rows == 64, LNZ_EINVAL, "%s: tile_rows = %d is not %s", who,
              tile_rows, heights);
  return LNZ_OK;
}

// `return LAUNCH(D)` for the width the envelope admits: 32, 64, 96 or 128
#define LNZ_GGNN_WIDTHS(D, LAUNCH) \
  switch (D) {                     \
    case 32: return LAUNCH(32);    \
    case 64: return LAUNCH(64);    \
    case 96: return LAUNCH(96);    \
    default: return LAUNCH(128);   \
  }

}  // namespace
