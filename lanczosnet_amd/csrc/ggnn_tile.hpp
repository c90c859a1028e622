// The gated-propagation tile of the GGNN forward (ggnn.hip), of one step of its backward (ggnn_grad.hip,
// which recomputes the step with the forward's arithmetic) and of the MPNN forward (mpnn.hip): the
// envelope, the MFMA tile product, the prologue, the GGNN message block, the gates, the GRU cell and the
// state store, each written once.  What stands here is the arithmetic all three kernels promise to share
// to the bit: change it here or nowhere.
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

// Channel c of a step, by the whole workgroup:  H_c = relu(S W1_c^T + b1_c) (wave w: hidden columns 16 w ..),
// M_c = H_c W2_c^T + b2_c (owner waves: features 16 w ..), A_c = Â_c M_c (four features of one row per task,
// the set bits of the row in ascending j).  A barrier after each.  with_h(rt, v) sees this lane's four hidden
// values of row 16 rt + m, with_a(r, q, s) the features 4 q .. of row r of A_c, as they are stored: the
// backward keeps them, the forward passes nothing.
template <int D, int RT, class FH, class FA>
__device__ __forceinline__ void ggnn_message(const MessageTile t, const int c, const float* __restrict__ W1,
                                             const float* __restrict__ b1, const float* __restrict__ W2,
                                             const float* __restrict__ b2, const int wave, const int m,
                                             const int g, FH&& with_h, FA&& with_a) {
  constexpr int GR = 16 * RT, SS = D + 4, DQ = D / 4, DB = D / 16;
  const int f0 = 16 * wave + 4 * g;
  {
    f32x4 h[1][RT];
    zero_tiles(h);
    const float* const wp[1] = {W1 + ((int64_t)c * GHID + 16 * wave + m) * D + 4 * g};
    tile_gemm<1, DB, RT>(t.Sb + m * SS + 4 * g, SS, wp, h);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(b1 + c * GHID + f0);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaxf(h[0][rt][e] + bv[e], 0.0f);
      *reinterpret_cast<f32x4*>(t.Hb + (16 * rt + m) * HS + f0) = v;
      with_h(rt, v);
    }
  }
  __syncthreads();
  if (wave < DB) {
    f32x4 mm[1][RT];
    zero_tiles(mm);
    const float* const wp[1] = {W2 + ((int64_t)c * D + 16 * wave + m) * GHID + 4 * g};
    tile_gemm<1, GHID / 16, RT>(t.Hb + m * HS + 4 * g, HS, wp, mm);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(b2 + c * D + f0);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) *reinterpret_cast<f32x4*>(t.Mb + (16 * rt + m) * SS + f0) = mm[0][rt] + bv;
  }
  __syncthreads();
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

// `return LAUNCH(D)` for the width the envelope admits: 32, 64, 96 or 128
#define LNZ_GGNN_WIDTHS(D, LAUNCH) \
  switch (D) {                     \
    case 32: return LAUNCH(32);    \
    case 64: return LAUNCH(64);    \
    case 96: return LAUNCH(96);    \
    default: return LAUNCH(128);   \
  }

}  // namespace
