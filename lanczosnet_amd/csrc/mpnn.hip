// The MPNN baseline (reference model/mpnn.py:125-212, model/set2set.py:60-100, config/qm8_mpnn.yaml): all
// num_prop edge-network propagation steps in ONE launch, the Set2Vec readout and output_func in another.
//
// lnz_mpnn_forward — the reference's default msg_func 'MLP' runs a 2D -> 64 -> D MLP on all N^2 ordered
// node pairs per channel and step.  Its first Linear splits over the concatenation [h_b, h_a] (h_b the
// neighbour, h_a the row the message is aggregated into), W1_c = [W1n_c | W1s_c], so per step on the
// state S [rows, D], channels c = 0 .. C-1 (C = num_bond_type + 1), hidden width 64:
//     P_c  = S W1n_c^T ;  Q_c = S W1s_c^T + b1_c                    [rows, 64] each
//     R_c[a] = sum over b with L[a, b, c] != 0 of relu(Q_c[a] + P_c[b])          (b ascending)
//     M_c[a] = R_c[a] W2_c^T + deg_c[a] b2_c                                      ('sum')
//     M_c[a] = (R_c[a] W2_c^T + deg_c[a] b2_c) / (deg_c[a] + FLT_EPSILON)         ('avg': divided AFTER the sum)
//     gi   = sum_c M_c W_ih[:, cD:(c+1)D]^T + b_ih ;  gh = S W_hh^T + b_hh        [rows, 3D]
//     r, z = sigmoid(gi_r + gh_r), sigmoid(gi_z + gh_z) ;  n = tanh(gi_n + r * gh_n)
//     S'   = (1 - z) * n + z * S
// Every one of the N rows of a molecule propagates: a padded row has degree 0, message exactly 0 and
// evolves under GRU(0, h).  L is only ever compared with zero (a NaN or a negative entry is an edge),
// never written.  The kernel leaves the final state; the readout is the second kernel.
// lnz_mpnn_forward_states is the same body (mpnn_forward_body) under a kernel with one more pointer: it also
// leaves the state trajectory [num_prop + 1][B N][D], all the backward (mpnn_grad.hip) keeps of the forward.
// The message block ([P_c | Q_c], R_c, M_c) stands in mpnn_tile.hpp, shared to the letter with that backward.
//
// Shape as built: ggnn.hip's.  A workgroup of eight waves owns a tile of floor(R / N) whole molecules,
// R = 64 or 32 rows, whose state stays in LDS for every step.  L is read once, through its four strides,
// into per-row bit masks and degrees.  The GEMMs run on v_mfma_f32_16x16x4_f32 through tile_gemm
// (ggnn_tile.hpp), weights streamed from L2.  [P_c | Q_c] is ONE 128-column product (wave w < 4: the 16
// columns 16 w .. of P_c, wave w >= 4: of Q_c — the two halves of the rows of W1_c, read where they
// lie), R_c runs on the VALU over the set bits only, M_c = R_c W2_c^T is a K = 64 product of the waves
// that own features, whose gate accumulators live across the channel loop as in ggnn.hip; the prologue,
// the gate products, gh, the GRU cell and the state store are ggnn_tile.hpp's routines, ggnn.hip's own.  Three barriers per channel, two per step.  LDS at D = 128, R = 64: S, M_c
// 64 x 132 floats each + [P|Q] 64 x 132 + R_c 64 x 68 + masks = 123,136 B.  No atomics, no
// cross-workgroup traffic, every sum in a fixed order: bit-reproducible, and a row's bits do not depend
// on the tile height.  The folded form W_ih[:, c] W2_c ([3D, 64] per channel) was not built.
//
// lnz_set2vec_readout — per molecule, X = the rows with mask != 0 (all N without a mask), q* [2D] = 0,
// mem [D] = 0; num_step times
//     f, i, o = sigmoid(W_f q* + b_f), sigmoid(W_i q* + b_i), sigmoid(W_o q* + b_o) ;  g = tanh(W_m q* + b_m)
//     mem = f mem + i g ;  q = o tanh(mem)
//     e_j = sum_f tanh((q W_1)_f + X_jf) W_2[f] ;  w = softmax_j(e) over the masked rows (max-subtracted)
//     q* = [q, sum_j w_j X_j]
// then score = W_out q* + b_out.  A workgroup batches up to 16 molecules as the 16 rows of an MFMA tile:
// wave w owns the features 16 w .. of all four gates (one tile_gemm with four weight tiles over K = 2D)
// and of q W_1 (W_1^T packed by the caller); a lane keeps `mem` of its (molecule, four features) in
// registers over the steps.  The energies take sixteen lanes per row (coalesced 16-byte reads of X, a
// fixed xor tree), the softmax one thread per molecule, the weighted sum one thread per (molecule, four
// features), j ascending.  X is re-read from L2 in every step: a full tile of sixteen 32-row molecules is
// 256 KB at D = 128, more than a workgroup's LDS, and a tile with fewer molecules would leave MFMA rows
// empty.  Rows outside the mask are never loaded; a molecule without a masked row reads exactly 0.
#include "common.hpp"
#include "ggnn_tile.hpp"
#include "mpnn_tile.hpp"

namespace {

constexpr int SMOL = 16;        // molecules per Set2Vec workgroup: the rows of one MFMA tile

// floats of dynamic LDS: S, M [GR][D + 4], [P|Q] [GR][132], R [GR][68], bits + deg [8][GR], rowbase [GR]
__host__ __device__ constexpr int mpnn_lds_floats(int D, int GR) {
  return 2 * GR * (D + 4) + GR * HS + GR * RS + 2 * GMAXC * GR + GR;
}

// The body of both kernels below.  TRAJ (lnz_mpnn_forward_states): also the state trajectory
// [num_prop + 1][B N][D] — S_t at the start of step t, S_T after the last —, a copy of the LDS rows that the
// arithmetic does not see; `states` is null and unread otherwise.
template <int D, int RT, bool TRAJ>
__device__ __forceinline__ void mpnn_forward_body(
    const float* __restrict__ state0, const int ld0, const float* __restrict__ L, const int64_t stride_b,
    const int64_t stride_r, const int64_t stride_c, const int64_t stride_ch, const float* __restrict__ W1,
    const float* __restrict__ b1, const float* __restrict__ W2, const float* __restrict__ b2,
    const float* __restrict__ Wih, const float* __restrict__ bih, const float* __restrict__ Whh,
    const float* __restrict__ bhh, const int B, const int N, const int C, const int num_prop, const int avg,
    float* __restrict__ state_out, const int ldso, float* __restrict__ states) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int GR = 16 * RT;    // rows per tile
  constexpr int SS = D + 4;      // row stride of S and M_c
  constexpr int DB = D / 16;     // 16-feature blocks of a state row: waves 0 .. DB-1 own one each
  float* const Sb = smem;
  float* const Mb = Sb + GR * SS;
  float* const Hb = Mb + GR * SS;                                       // [row][P_c 0..63 | Q_c 64..127]
  float* const Rb = Hb + GR * HS;
  unsigned* const bits = reinterpret_cast<unsigned*>(Rb + GR * RS);     // [c][row]
  float* const deg = reinterpret_cast<float*>(bits + GMAXC * GR);       // [c][row]
  int* const rowbase = reinterpret_cast<int*>(deg + GMAXC * GR);        // first row of the row's molecule

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 15, g = lane >> 4;
  const TileSpan ts = tile_span<RT>(B, N);
  const int64_t row0 = ts.mol0 * N;      // first global row of the tile
  const int rows = ts.rows;

  // ---- the state, the bit masks and degrees of L, the molecule of every row
  load_state_tile<D, RT>(Sb, state0, row0, ld0, rows);
  load_edge_bits<RT>(bits, L, stride_b, stride_r, stride_c, stride_ch, ts, N, C,
                     [&](const int at, const int degree) { deg[at] = (float)degree; });
  set_rowbase<RT>(rowbase, N, rows);
  __syncthreads();

  const bool owner = wave < DB;          // wave-uniform: this wave owns features 16 wave .. 16 wave + 15
  const float* const s_frag = Sb + m * SS + 4 * g;
  const float* const m_frag = Mb + m * SS + 4 * g;
  const EdgeTile et = {Sb, Mb, Hb, Rb, bits, deg, rowbase};
  const auto put_state = [&](const int t) {
    store_state_tile<D>(states + ((int64_t)t * B * N + row0) * D, D, Sb, rows);
  };

  for (int step = 0; step < num_prop; ++step) {
    if constexpr (TRAJ) put_state(step);
    // gate accumulators of this wave's feature block: [0] r, [1] z, [2] gi_n
    f32x4 acc[3][RT];
    zero_tiles(acc);
    for (int c = 0; c < C; ++c) {   // three barriers per channel
      edge_message<D, RT>(et, c, W1, b1, W2, b2, avg, wave, m, g, [](int, int, const f32x4&) {},
                          [](int, const f32x4&) {});
      if (owner) gate_accumulate<D, RT>(m_frag, Wih, c, C, wave, m, g, acc);
    }
    f32x4 gh[3][RT];
    if (owner) hidden_gates<D, RT>(s_frag, Whh, wave, m, g, gh);
    __syncthreads();
    if (owner) LNZ_GRU_CELL(D, RT);
    __syncthreads();
  }
  // ---- the final state
  if constexpr (TRAJ) put_state(num_prop);
  store_state_tile<D>(state_out + row0 * (int64_t)ldso, ldso, Sb, rows);
}

template <int D, int RT>
__global__ __launch_bounds__(GNT) void mpnn_forward_kernel(
    const float* __restrict__ state0, const int ld0, const float* __restrict__ L, const int64_t stride_b,
    const int64_t stride_r, const int64_t stride_c, const int64_t stride_ch, const float* __restrict__ W1,
    const float* __restrict__ b1, const float* __restrict__ W2, const float* __restrict__ b2,
    const float* __restrict__ Wih, const float* __restrict__ bih, const float* __restrict__ Whh,
    const float* __restrict__ bhh, const int B, const int N, const int C, const int num_prop, const int avg,
    float* __restrict__ state_out, const int ldso) {
  mpnn_forward_body<D, RT, false>(state0, ld0, L, stride_b, stride_r, stride_c, stride_ch, W1, b1, W2, b2, Wih, bih,
                                  Whh, bhh, B, N, C, num_prop, avg, state_out, ldso, nullptr);
}

template <int D, int RT>
__global__ __launch_bounds__(GNT) void mpnn_forward_states_kernel(
    const float* __restrict__ state0, const int ld0, const float* __restrict__ L, const int64_t stride_b,
    const int64_t stride_r, const int64_t stride_c, const int64_t stride_ch, const float* __restrict__ W1,
    const float* __restrict__ b1, const float* __restrict__ W2, const float* __restrict__ b2,
    const float* __restrict__ Wih, const float* __restrict__ bih, const float* __restrict__ Whh,
    const float* __restrict__ bhh, const int B, const int N, const int C, const int num_prop, const int avg,
    float* __restrict__ state_out, const int ldso, float* __restrict__ states) {
  mpnn_forward_body<D, RT, true>(state0, ld0, L, stride_b, stride_r, stride_c, stride_ch, W1, b1, W2, b2, Wih, bih,
                                 Whh, bhh, B, N, C, num_prop, avg, state_out, ldso, states);
}

template <int D, int RT>
int launch_mpnn(const float* state0, int ld0, const float* L, int64_t sb, int64_t sr, int64_t sc, int64_t sch,
                const float* W1, const float* b1, const float* W2, const float* b2, const float* Wih,
                const float* bih, const float* Whh, const float* bhh, int B, int N, int C, int num_prop, int avg,
                float* state_out, int ldso, float* states, int grid, hipStream_t s, const char* who) {
  const size_t lds = sizeof(float) * (size_t)mpnn_lds_floats(D, 16 * RT);
  if (states != nullptr) {
    auto kfn = mpnn_forward_states_kernel<D, RT>;
    LNZ_DYNAMIC_LDS(kfn, lds, "mpnn.hip");
    hipLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(GNT), lds, s, state0, ld0, L, sb, sr, sc, sch, W1, b1, W2, b2,
                       Wih, bih, Whh, bhh, B, N, C, num_prop, avg, state_out, ldso, states);
  } else {
    auto kfn = mpnn_forward_kernel<D, RT>;
    LNZ_DYNAMIC_LDS(kfn, lds, "mpnn.hip");
    hipLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(GNT), lds, s, state0, ld0, L, sb, sr, sc, sch, W1, b1, W2, b2,
                       Wih, bih, Whh, bhh, B, N, C, num_prop, avg, state_out, ldso);
  }
  return lnz::check_launch(who);
}

// ------------------------------------------------------------------------------------------ Set2Vec
template <int D>
__global__ __launch_bounds__(GNT) void set2vec_readout_kernel(
    const float* __restrict__ X, const int ld, const unsigned char* __restrict__ mask,
    const float* __restrict__ Wg, const float* __restrict__ bg, const float* __restrict__ W1T,
    const float* __restrict__ w2, const float* __restrict__ Wout, const float* __restrict__ bout, const int B,
    const int N, const int P, const int num_step, const int mpw, float* __restrict__ score) {
  constexpr int QS = 2 * D + 4;   // row stride of q* = [q | read]
  constexpr int US = D + 4;       // row stride of q W_1
  constexpr int DQ = D / 4;
  constexpr int DB = D / 16;
  __shared__ __attribute__((aligned(16))) float qs[SMOL * QS];
  __shared__ __attribute__((aligned(16))) float ub[SMOL * US];
  __shared__ float en[SMOL * GMAXN];    // energies, then softmax weights, [molecule][row]
  __shared__ unsigned mbits[SMOL];      // bit j: row j of the molecule is in the set

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 15, g = lane >> 4;
  const int64_t mol0 = (int64_t)blockIdx.x * mpw;
  const int nm = (int)(B - mol0 < mpw ? B - mol0 : mpw);   // molecules of this workgroup: rows 0 .. nm-1 of the tile

  for (int idx = tid; idx < SMOL * QS; idx += GNT) qs[idx] = 0.0f;
  if (tid < SMOL) {
    unsigned bm = 0;
    if (tid < nm) {
      if (mask == nullptr) {
        bm = N >= 32 ? 0xffffffffu : (1u << N) - 1u;
      } else {
        for (int j = 0; j < N; ++j) bm |= (mask[(mol0 + tid) * N + j] != 0 ? 1u : 0u) << j;
      }
    }
    mbits[tid] = bm;
  }
  __syncthreads();

  const bool owner = wave < DB;
  const int f0 = 16 * wave + 4 * g;      // this lane's four features of molecule m (owner waves)
  const float* const q_frag = qs + m * QS + 4 * g;
  f32x4 mem = {0.0f, 0.0f, 0.0f, 0.0f};
  const int grp = tid >> 4, gl = tid & 15;   // the sixteen-lane group of the energies and the lane in it

  for (int step = 0; step < num_step; ++step) {
    // the four gates of this wave's features: f, i, o, memory (model/set2set.py:49-55)
    f32x4 ga[4][1];
    if (owner) {
#pragma unroll
      for (int t = 0; t < 4; ++t) ga[t][0] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      const float* const row = Wg + (int64_t)(16 * wave + m) * (2 * D) + 4 * g;
      const float* const wp[4] = {row, row + 2 * D * D, row + 4 * D * D, row + 6 * D * D};
      tile_gemm<4, 2 * DB, 1>(q_frag, QS, wp, ga);
    }
    __syncthreads();   // every wave has read all of q*
    if (owner) {
      const f32x4 b_f = *reinterpret_cast<const f32x4*>(bg + f0);
      const f32x4 b_i = *reinterpret_cast<const f32x4*>(bg + D + f0);
      const f32x4 b_o = *reinterpret_cast<const f32x4*>(bg + 2 * D + f0);
      const f32x4 b_m = *reinterpret_cast<const f32x4*>(bg + 3 * D + f0);
      f32x4 qn;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float ft = sigmoidf_(ga[0][0][e] + b_f[e]);
        const float it = sigmoidf_(ga[1][0][e] + b_i[e]);
        const float ot = sigmoidf_(ga[2][0][e] + b_o[e]);
        const float ct = tanhf(ga[3][0][e] + b_m[e]);
        mem[e] = ft * mem[e] + it * ct;
        qn[e] = ot * tanhf(mem[e]);
      }
      *reinterpret_cast<f32x4*>(qs + m * QS + f0) = qn;
    }
    __syncthreads();
    if (owner) {   // u = q W_1: features 16 wave ..
      f32x4 u[1][1] = {{f32x4{0.0f, 0.0f, 0.0f, 0.0f}}};
      const float* const wp[1] = {W1T + (int64_t)(16 * wave + m) * D + 4 * g};
      tile_gemm<1, DB, 1>(q_frag, QS, wp, u);
      *reinterpret_cast<f32x4*>(ub + m * US + f0) = u[0][0];
    }
    __syncthreads();
    // e_j = sum_f tanh(u_f + X_jf) W_2[f]: sixteen lanes per row of the set, the others are not loaded
    for (int task = grp; task < nm * N; task += GNT / 16) {
      const int ml = task / N, j = task - ml * N;
      if ((mbits[ml] >> j) & 1u) {
        const float* const xr = X + ((mol0 + ml) * N + j) * (int64_t)ld;
        float s = 0.0f;
        for (int q = gl; q < DQ; q += 16) {
          const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + 4 * q);
          const f32x4 uv = *reinterpret_cast<const f32x4*>(ub + ml * US + 4 * q);
          const f32x4 wv = *reinterpret_cast<const f32x4*>(w2 + 4 * q);
#pragma unroll
          for (int e = 0; e < 4; ++e) s = fmaf(tanhf(uv[e] + xv[e]), wv[e], s);
        }
        s += __shfl_xor(s, 8, 16);
        s += __shfl_xor(s, 4, 16);
        s += __shfl_xor(s, 2, 16);
        s += __shfl_xor(s, 1, 16);
        if (gl == 0) en[ml * GMAXN + j] = s;
      }
    }
    __syncthreads();
    if (tid < nm) {   // softmax over the set, max-subtracted; an empty set has no weights
      const unsigned bm0 = mbits[tid];
      float* const e = en + tid * GMAXN;
      float mx = -FLT_MAX, sum = 0.0f;
      for (unsigned bm = bm0; bm; bm &= bm - 1) mx = fmaxf(mx, e[__ffs(bm) - 1]);
      for (unsigned bm = bm0; bm; bm &= bm - 1) {
        const int j = __ffs(bm) - 1;
        const float p = expf(e[j] - mx);
        e[j] = p;
        sum += p;
      }
      for (unsigned bm = bm0; bm; bm &= bm - 1) e[__ffs(bm) - 1] /= sum;
    }
    __syncthreads();
    // read = sum_j w_j X_j over the set, j ascending: four features of one molecule per task
    for (int idx = tid; idx < nm * DQ; idx += GNT) {
      const int ml = idx / DQ, q = idx - ml * DQ;
      const float* const xm = X + (mol0 + ml) * N * (int64_t)ld + 4 * q;
      f32x4 s = {0.0f, 0.0f, 0.0f, 0.0f};
      for (unsigned bm = mbits[ml]; bm; bm &= bm - 1) {
        const int j = __ffs(bm) - 1;
        const float wj = en[ml * GMAXN + j];
        const f32x4 xv = *reinterpret_cast<const f32x4*>(xm + j * (int64_t)ld);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] = fmaf(wj, xv[e], s[e]);
      }
      *reinterpret_cast<f32x4*>(qs + ml * QS + D + 4 * q) = s;
    }
    __syncthreads();
  }

  // ---- output_func: score = W_out q* + b_out, k ascending
  for (int idx = tid; idx < nm * P; idx += GNT) {
    const int ml = idx / P, p = idx - ml * P;
    const float* const w = Wout + (int64_t)p * (2 * D);
    float a = 0.0f;
    for (int k = 0; k < 2 * D; ++k) a = fmaf(qs[ml * QS + k], w[k], a);
    score[(mol0 + ml) * P + p] = a + bout[p];
  }
}

template <int D>
int launch_set2vec(const float* X, int ld, const uint8_t* mask, const float* Wg, const float* bg, const float* W1T,
                   const float* w2, const float* Wout, const float* bout, int B, int N, int P, int num_step, int mpw,
                   float* score, hipStream_t s) {
  const int64_t grid = ((int64_t)B + mpw - 1) / mpw;
  hipLaunchKernelGGL(set2vec_readout_kernel<D>, dim3((unsigned)grid), dim3(GNT), 0, s, X, ld, mask, Wg, bg, W1T, w2,
                     Wout, bout, B, N, P, num_step, mpw, score);
  return lnz::check_launch("lnz_set2vec_readout");
}

int mpnn_forward_impl(const char* who, const float* state0, int ld0, const float* L, int64_t stride_b,
                      int64_t stride_r, int64_t stride_c, int64_t stride_ch, const float* W1, const float* b1,
                      const float* W2, const float* b2, const float* Wih, const float* bih, const float* Whh,
                      const float* bhh, int B, int N, int C, int D, int num_prop, int avg, float* state_out, int ldso,
                      float* states, int tile_rows, lnz_stream_t stream) {
  {
    const float* const w[8] = {W1, b1, W2, b2, Wih, bih, Whh, bhh};
    const int rc = check_propagation(who, state0, ld0, state_out, ldso, stride_b, stride_r, stride_c, stride_ch, w, B,
                                     N, C, D, nullptr, num_prop);
    if (rc != LNZ_OK) return rc;
  }
  const uint64_t rows = (uint64_t)B * N;
  const uint64_t n0 = span(rows, ld0, D), no = span(rows, ldso, D);
  LNZ_REQUIRE(state_out == nullptr || !overlap(state_out, no, state0, n0), LNZ_EINVAL,
              "%s: state_out must not alias state0", who);
  if (states != nullptr) {
    const uint64_t nst = ((uint64_t)num_prop + 1) * rows * D * sizeof(float);
    LNZ_REQUIRE(aligned16(states), LNZ_ENOTSUP, "%s: states must be 16-byte aligned", who);
    LNZ_REQUIRE(!overlap(states, nst, state0, n0) && (state_out == nullptr || !overlap(states, nst, state_out, no)),
                LNZ_EINVAL, "%s: states must not alias state0 or state_out", who);
    if (state_out == nullptr) {   // the final state goes where the trajectory keeps it
      state_out = states + (uint64_t)num_prop * rows * D;
      ldso = D;
    }
  }
  LNZ_REQUIRE(tile_rows == 0 || tile_rows == 32 || tile_rows == 64, LNZ_EINVAL,
              "%s: tile_rows = %d is not 0 (chosen by the batch), 32 or 64", who, tile_rows);
  const int rows_per_tile = choose_tile_rows(B, N, tile_rows);
  const int mpt = rows_per_tile / N;
  const int64_t grid = ((int64_t)B + mpt - 1) / mpt;
  hipStream_t s = (hipStream_t)stream;
  lnz::note_kernel(states ? "mpnn_forward_states_kernel<%d, %d>" : "mpnn_forward_kernel<%d, %d>", D,
                   rows_per_tile / 16);
#define LNZ_MPNN_LAUNCH_(DD, RTT)                                                                                  \
  launch_mpnn<DD, RTT>(state0, ld0, L, stride_b, stride_r, stride_c, stride_ch, W1, b1, W2, b2, Wih, bih, Whh, bhh, \
                       B, N, C, num_prop, avg ? 1 : 0, state_out, ldso, states, (int)grid, s, who)
#define LNZ_MPNN_LAUNCH(DD) (rows_per_tile == 32 ? LNZ_MPNN_LAUNCH_(DD, 2) : LNZ_MPNN_LAUNCH_(DD, 4))
  LNZ_GGNN_WIDTHS(D, LNZ_MPNN_LAUNCH)
#undef LNZ_MPNN_LAUNCH
#undef LNZ_MPNN_LAUNCH_
}

}  // namespace

extern "C" int lnz_mpnn_forward(const float* state0, int ld0, const float* L, int64_t stride_b, int64_t stride_r,
                                int64_t stride_c, int64_t stride_ch, const float* W1, const float* b1,
                                const float* W2, const float* b2, const float* Wih, const float* bih,
                                const float* Whh, const float* bhh, int B, int N, int C, int D, int num_prop, int avg,
                                float* state_out, int ldso, int tile_rows, lnz_stream_t stream) {
  const char* const who = "lnz_mpnn_forward";
  LNZ_REQUIRE(state0 && L && W1 && b1 && W2 && b2 && Wih && bih && Whh && bhh && state_out, LNZ_EINVAL,
              "%s: null pointer", who);
  return mpnn_forward_impl(who, state0, ld0, L, stride_b, stride_r, stride_c, stride_ch, W1, b1, W2, b2, Wih, bih, Whh,
                           bhh, B, N, C, D, num_prop, avg, state_out, ldso, nullptr, tile_rows, stream);
}

extern "C" int lnz_mpnn_forward_states(const float* state0, int ld0, const float* L, int64_t stride_b,
                                       int64_t stride_r, int64_t stride_c, int64_t stride_ch, const float* W1,
                                       const float* b1, const float* W2, const float* b2, const float* Wih,
                                       const float* bih, const float* Whh, const float* bhh, int B, int N, int C,
                                       int D, int num_prop, int avg, float* state_out, int ldso, float* states,
                                       int tile_rows, lnz_stream_t stream) {
  const char* const who = "lnz_mpnn_forward_states";
  LNZ_REQUIRE(state0 && L && W1 && b1 && W2 && b2 && Wih && bih && Whh && bhh && states, LNZ_EINVAL,
              "%s: null pointer", who);
  return mpnn_forward_impl(who, state0, ld0, L, stride_b, stride_r, stride_c, stride_ch, W1, b1, W2, b2, Wih, bih, Whh,
                           bhh, B, N, C, D, num_prop, avg, state_out, ldso, states, tile_rows, stream);
}

extern "C" int lnz_set2vec_readout(const float* X, int ld, const uint8_t* mask, const float* Wg, const float* bg,
                                   const float* W1T, const float* w2, const float* Wout, const float* bout, int B,
                                   int N, int D, int P, int num_step, float* score, int mols_per_group,
                                   lnz_stream_t stream) {
  const char* const who = "lnz_set2vec_readout";
  LNZ_REQUIRE(X && Wg && bg && W1T && w2 && Wout && bout && score, LNZ_EINVAL, "%s: null pointer", who);
  LNZ_REQUIRE(B > 0 && N > 0, LNZ_EINVAL, "%s: B = %d, N = %d must be positive", who, B, N);
  LNZ_REQUIRE(N <= GMAXN && D >= 32 && D <= GMAXD && D % 32 == 0 && P >= 1 && P <= GMAXP && num_step >= 0,
              LNZ_ENOTSUP,
              "%s: N = %d, D = %d, P = %d, num_step = %d outside 1 <= N <= 32, D a multiple of 32 and <= 128, "
              "1 <= P <= 16, num_step >= 0", who, N, D, P, num_step);
  LNZ_REQUIRE(ld >= D, LNZ_EINVAL, "%s: ld = %d below the width %d", who, ld, D);
  LNZ_REQUIRE(ld % 4 == 0 && aligned16(X) && aligned16(Wg) && aligned16(bg) && aligned16(W1T) && aligned16(w2),
              LNZ_ENOTSUP, "%s: the rows of X and of the weights must be 16-byte aligned (ld = %d)", who, ld);
  LNZ_REQUIRE(!overlap(score, (uint64_t)B * P * sizeof(float), X, span((uint64_t)B * N, ld, D)), LNZ_EINVAL,
              "%s: score must not alias X", who);
  LNZ_REQUIRE(mols_per_group >= 0 && mols_per_group <= SMOL, LNZ_EINVAL,
              "%s: mols_per_group = %d is not 0 (chosen by the batch) or 1 .. 16", who, mols_per_group);
  // molecules per workgroup: as few as spread the batch over the compute units, at most the 16 rows of a tile
  int mpw = mols_per_group;
  if (mpw == 0) {
    const int cus = device_cus();
    mpw = (int)(((int64_t)B + cus - 1) / cus);
    mpw = mpw < 1 ? 1 : mpw > SMOL ? SMOL : mpw;
  }
  hipStream_t s = (hipStream_t)stream;
  lnz::note_kernel("set2vec_readout_kernel<%d> x %d", D, mpw);
#define LNZ_SET2VEC_LAUNCH(DD) \
  launch_set2vec<DD>(X, ld, mask, Wg, bg, W1T, w2, Wout, bout, B, N, P, num_step, mpw, score, s)
  LNZ_GGNN_WIDTHS(D, LNZ_SET2VEC_LAUNCH)
#undef LNZ_SET2VEC_LAUNCH
}
