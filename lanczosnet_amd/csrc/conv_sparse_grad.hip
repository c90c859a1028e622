// Backward of the large-graph layer on the nonzeros of its symmetric operators, exact fp32
// (`_LargeSparseFusedFunction`, model/_large.py).  With ONE operator a layer of the forward is
//
//     X' = relu( L Z + V T + b ),   Z = X Wn^T,   Y = V^T X,   T = sum_s diag(g_s) Y W_s^T
//
// (reference model/lanczos_net_general.py:157-182 with one edge type: Wn = the sum of the two
// edge-channel column blocks of the mix weight).  With dX' the gradient of its output:
//
//   lnz_large_grad_project   dP = dX' * (X' > 0) in place (rows at or beyond a graph's node count:
//                            exactly zero), db = sum_rows dP, A = V^T dP [B,K,128] — one pass over
//                            dX', X' and V; A on v_mfma_f32_16x16x4_f32 per chunk of 256 rows, the
//                            chunks' partials added in ascending order by a second launch (no atomics:
//                            two identical calls give the same bits).
//   (dZ = L dP: L is symmetric, so the forward's own gather lnz_large_sparse_conv_f32 with relu = 0
//    onto a zeroed buffer is L^T dP.)
//   lnz_large_grad_spectral  one workgroup per graph: U_s = A W_s on the matrix pipe, then
//                            dG[k][s] = <U_s[k], Y[k]>, dY[k] = sum_s g_s[k] U_s[k], Q[k][s] = g_s[k] Y[k].
//   lnz_large_grad_input     dX = [dZ | V] [Wn ; dY]: ONE fp32 GEMM over the depth 128 + K whose lower K
//                            operand rows are per graph, written at leading dimension 128 (columns
//                            beyond the layer's input width zero) — the next layer's dX'.
//
// R = 2 .. 8 symmetric operators (a typed batch: the same Function):  X' = relu( sum_c
// L_c Z_c + V T + b ),  Z_c = X Wn_c^T.  dZ_c = L_c dP is lnz_large_sparse_conv_split_f32 (csrc/conv_sparse.hip: R
// results gathered from one source), dWn_c = dZ_c^T X one library GEMM per block, and
//   lnz_large_grad_input_channels   dX = sum_c dZ_c Wn_c + V dY: the same GEMM over the depth R 128 + K — the same
//                            kernel: lnz_large_grad_input is its R = 1.
//
// MFMA operand maps (v_mfma_f32_16x16x4_f32): lane l holds A[i = l & 15][k = l >> 4] and
// B[k = l >> 4][j = l & 15]; C/D register j of lane l is row 4 (l >> 4) + j, column l & 15.  The LDS
// tiles are padded so that a wave's ds_read_b32 of either operand is conflict free (32 lanes per LDS
// cycle, bank = dword address mod 32): tiles read as B[k][j] (k = 2 rows, j = 16 columns per lane
// group) have a row stride of 16 mod 32 dwords, tiles read as A[i][k] (i = 16 rows, k = 2 columns) a
// row stride of 2 mod 32.
#include "common.hpp"
#include "wave.hpp"

namespace {

constexpr int DH = 128;          // hidden width
constexpr int KMAX = 64;         // LARGE_MAX_K
constexpr int SMAX = 16;         // gains_kernel_max_scales
constexpr int RMAX = 8;          // LARGE_MAX_OPERATORS
constexpr int CHUNK = 256;       // rows of a graph per workgroup of the projection
constexpr int STEP = 32;         // ... staged in LDS at a time
constexpr int PART_ROWS = KMAX + 1;   // a chunk's partial: 64 rows of A, then the bias row

__device__ inline f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// ---- dP, bias partial and A partial of one chunk of 256 rows -----------------------------------
// 4 waves; wave w owns feature columns [32 w, 32 w + 32) of A (two 16-column tiles) for all four
// 16-row tiles of eigen directions: 8 accumulators.
constexpr int SP_LD = DH + 16, SV_LD = KMAX + 16;
__global__ __launch_bounds__(256) void large_grad_project_kernel(
    float* __restrict__ dX, const float* __restrict__ Xout, const float* __restrict__ V,
    const int32_t* __restrict__ n_nodes, int B, int N, int K, int chunks, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float sP[STEP][SP_LD];
  __shared__ float sV[STEP][SV_LD];
  __shared__ float sDb[2][DH];
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int rbeg = chunk * CHUNK, rend = min(N, rbeg + CHUNK);
  int n = N;
  if (n_nodes) n = min(max(n_nodes[b], 0), N);
  n = __builtin_amdgcn_readfirstlane(n);
  const int ktiles = (K + 15) >> 4;
  f32x4 acc[4][2];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
    for (int c = 0; c < 2; ++c) acc[kt][c] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  float dbacc = 0.0f;
  const int li = lane & 15, lk = lane >> 4;
  for (int r0 = rbeg; r0 < rend; r0 += STEP) {
    // the gradient tile, masked by the activation and the node count, back to memory and into LDS
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = t + 256 * u, row = idx >> 5, c4 = idx & 31, r = r0 + row;
      f32x4 p = {0.0f, 0.0f, 0.0f, 0.0f};
      if (r < rend) {
        const int64_t off = ((int64_t)b * N + r) * DH + 4 * c4;
        if (r < n) {
          const f32x4 g = *reinterpret_cast<const f32x4*>(dX + off);
          const f32x4 x = *reinterpret_cast<const f32x4*>(Xout + off);
#pragma unroll
          for (int e = 0; e < 4; ++e) p[e] = x[e] > 0.0f ? g[e] : 0.0f;
        }
        *reinterpret_cast<f32x4*>(dX + off) = p;
      }
      *reinterpret_cast<f32x4*>(&sP[row][4 * c4]) = p;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = t + 256 * u, row = idx >> 6, k = idx & 63, r = r0 + row;
      sV[row][k] = (r < n && k < K) ? V[((int64_t)b * N + r) * K + k] : 0.0f;
    }
    __syncthreads();
    if (r0 < n) {   // (uniform) a step of padding rows adds nothing
#pragma unroll
      for (int k0 = 0; k0 < STEP; k0 += 4) {
        float bq[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) bq[c] = sP[k0 + lk][(2 * w + c) * 16 + li];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
          if (kt < ktiles) {
            const float a = sV[k0 + lk][kt * 16 + li];
#pragma unroll
            for (int c = 0; c < 2; ++c) acc[kt][c] = mfma16(a, bq[c], acc[kt][c]);
          }
        }
      }
      const int col = t & 127, half = t >> 7;
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) dbacc += sP[half * 16 + rr][col];
    }
    __syncthreads();
  }
  float* pp = part + ((int64_t)b * chunks + chunk) * PART_ROWS * DH;
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        pp[(kt * 16 + 4 * lk + j) * DH + (2 * w + c) * 16 + li] = acc[kt][c][j];
  sDb[t >> 7][t & 127] = dbacc;
  __syncthreads();
  if (t < DH) pp[KMAX * DH + t] = sDb[0][t] + sDb[1][t];
}

// ---- second stage: the chunks' partials in ascending order -> A [B][K][128], db [B][128] -------
__global__ __launch_bounds__(256) void large_grad_project_reduce_kernel(
    const float* __restrict__ part, int K, int chunks, float* __restrict__ A, float* __restrict__ db) {
  const int b = blockIdx.x;
  const float* pp = part + (int64_t)b * chunks * PART_ROWS * DH;
  for (int e = threadIdx.x; e < PART_ROWS * DH; e += 256) {
    const int row = e / DH, col = e - row * DH;
    if (row >= K && row < KMAX) continue;
    float s = 0.0f;
    for (int c = 0; c < chunks; ++c) s += pp[(int64_t)c * PART_ROWS * DH + e];
    if (row < K) A[((int64_t)b * K + row) * DH + col] = s;
    else db[(int64_t)b * DH + col] = s;
  }
}

// ---- eigen space: U_s = A W_s for every long scale, its three contractions ------------------------
// One workgroup per graph, 4 waves; wave w owns input columns [32 w, 32 w + 32) of U_s for all four
// 16-row tiles of eigen directions.  A [64][128] in LDS (read as the MFMA's A operand), W_s read in
// place from the mix weight W [128][ldw] (column block s: W_s[o][i] = W[o ldw + s d + i]), the lane's
// elements of Y in registers at the accumulator positions.
constexpr int SA_LD = DH + 2;
__global__ __launch_bounds__(256) void large_grad_spectral_kernel(
    const float* __restrict__ A, const float* __restrict__ Y, int ldy, const float* __restrict__ G,
    const float* __restrict__ W, int ldw, int K, int S, int d, float* __restrict__ dG,
    float* __restrict__ Q, float* __restrict__ dY) {
  __shared__ float sA[KMAX][SA_LD];
  __shared__ float sG[SMAX][KMAX];
  __shared__ float sdG[4][SMAX][KMAX];
  const int b = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int li = lane & 15, lk = lane >> 4;
  for (int e = t; e < KMAX * DH; e += 256) {
    const int k = e >> 7, o = e & 127;
    sA[k][o] = k < K ? A[((int64_t)b * K + k) * DH + o] : 0.0f;
  }
  for (int e = t; e < SMAX * KMAX; e += 256) {
    const int s = e >> 6, k = e & 63;
    sG[s][k] = (s < S && k < K) ? G[((int64_t)b * S + s) * K + k] : 0.0f;
  }
  f32x4 Yr[4][2], dYa[4][2];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      dYa[kt][c] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      const int i = (2 * w + c) * 16 + li;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = kt * 16 + 4 * lk + j;
        Yr[kt][c][j] = (k < K && i < d) ? Y[((int64_t)b * K + k) * ldy + i] : 0.0f;
      }
    }
  __syncthreads();
  for (int s = 0; s < S; ++s) {
    f32x4 U[4][2];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
      for (int c = 0; c < 2; ++c) U[kt][c] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const float* Ws = W + (int64_t)s * d;
#pragma unroll 4
    for (int o0 = 0; o0 < DH; o0 += 4) {
      float bq[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int i = (2 * w + c) * 16 + li;
        bq[c] = i < d ? Ws[(int64_t)(o0 + lk) * ldw + i] : 0.0f;
      }
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const float a = sA[kt * 16 + li][o0 + lk];
#pragma unroll
        for (int c = 0; c < 2; ++c) U[kt][c] = mfma16(a, bq[c], U[kt][c]);
      }
    }
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = kt * 16 + 4 * lk + j;
        const float g = sG[s][k];
        float pd = U[kt][0][j] * Yr[kt][0][j];
        pd = fmaf(U[kt][1][j], Yr[kt][1][j], pd);
        pd = lnz::row16_sum(pd);   // over the 16 columns of both tiles: the same bits in all 16 lanes
        if (li == 0) sdG[w][s][k] = pd;
#pragma unroll
        for (int c = 0; c < 2; ++c) dYa[kt][c][j] = fmaf(g, U[kt][c][j], dYa[kt][c][j]);
      }
  }
  __syncthreads();
  if (dG)
    for (int e = t; e < K * S; e += 256) {
      const int k = e / S, s = e - k * S;
      dG[((int64_t)b * K + k) * S + s] = (sdG[0][s][k] + sdG[1][s][k]) + (sdG[2][s][k] + sdG[3][s][k]);
    }
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = kt * 16 + 4 * lk + j;
        if (k < K) dY[((int64_t)b * K + k) * DH + (2 * w + c) * 16 + li] = dYa[kt][c][j];
      }
  const int per = S * d;
  for (int e = t; e < K * per; e += 256) {
    const int k = e / per, rem = e - k * per, s = rem / d, i = rem - s * d;
    Q[((int64_t)b * K + k) * per + rem] = sG[s][k] * Y[((int64_t)b * K + k) * ldy + i];
  }
}

// ---- dX = sum_c dZ_c Wn_c + V dY over R operator channels: 64 rows of one graph per workgroup -------
// ONE kernel for one operator (R = 1: dX = dZ Wn + V dY) and for the R = 2 .. 8 channels of a typed batch (X' =
// relu( sum_c L_c Z_c + V T + b ), Z_c = X Wn_c^T).  Wave w owns rows [16 w, 16 w + 16)
// and all column tiles below the input width.  The row tile [64][R 128 + K] = [dZ_0 | .. | dZ_{R-1} | V] (the
// MFMA's A operand) does not fit LDS at R = 8, so the [64][128] tile of dZ_c is restaged once per channel —
// requested from memory before the previous channel's MFMAs, written to LDS behind them — and the V tile is
// staged once, in the same padded rows (row stride 2 mod 32: the A operand's ds_read_b32 stays conflict free).
// The second operand is read in place: Wn [R][128][128] is ONE matrix of R 128 rows (row 128 c + o = Wn_c[o],
// columns >= d zero), then the K rows of the graph's dY [K][128].  Its next PF steps are requested before this
// turn's MFMAs: the L2 latency is hidden behind them (read at use, one step at a time, the launch was latency
// bound: 1.03 ms per layer at config 5 against 0.16 ms of MFMA issue).  Ascending depth into one accumulator
// per column tile.
constexpr int IN_ROWS = 64, ST_LD = DH + KMAX + 2;
__global__ __launch_bounds__(256) void large_grad_input_channels_kernel(
    const float* __restrict__ dZ, const float* __restrict__ Wn, const float* __restrict__ V,
    const float* __restrict__ dY, int B, int N, int K, int R, int d, float* __restrict__ dX) {
  __shared__ float sT[IN_ROWS][ST_LD];
  const int b = blockIdx.y, r0 = blockIdx.x * IN_ROWS;
  const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int Kp = (K + 3) & ~3;
  const int64_t rows = (int64_t)B * N;
  f32x4 z[8];   // the next channel's tile of dZ, on its way
  auto fetch = [&](const int c) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = t + 256 * u, row = idx >> 5, c4 = idx & 31, r = r0 + row;
      z[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      if (r < N) z[u] = *reinterpret_cast<const f32x4*>(dZ + ((int64_t)c * rows + (int64_t)b * N + r) * DH + 4 * c4);
    }
  };
  fetch(0);
  for (int idx = t; idx < IN_ROWS * Kp; idx += 256) {
    const int row = idx / Kp, k = idx - row * Kp, r = r0 + row;
    sT[row][DH + k] = (r < N && k < K) ? V[((int64_t)b * N + r) * K + k] : 0.0f;
  }
  const int nct = (d + 15) >> 4;
  f32x4 acc[8];
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) acc[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  // depth index dep < R 128: row dep of the stacked Wn; R 128 + k: row k of the graph's dY (k >= K: padding,
  // zero).  The look-ahead runs across the channel seams: the operand rows do not wait for the restaging.
  const int RD = R * DH;
  auto load = [&](float (&v)[8], const int k0) {
    const int dep = k0 + lk;
    const float* p = nullptr;
    if (dep < RD) p = Wn + (int64_t)dep * DH + li;
    else if (dep - RD < K) p = dY + ((int64_t)b * K + (dep - RD)) * DH + li;
#pragma unroll
    for (int ct = 0; ct < 8; ++ct) v[ct] = (p && ct < nct) ? p[ct * 16] : 0.0f;
  };
  constexpr int PF = 2;
  float cur[PF][8], nxt[PF][8];
#pragma unroll
  for (int u = 0; u < PF; ++u) load(cur[u], 4 * u);
  // one turn of 4 PF depth steps: operand rows g0 .., the A operand from columns a0 .. of the tile, `n` live
  auto turn = [&](const int g0, const int a0, const int n) {
#pragma unroll
    for (int u = 0; u < PF; ++u) load(nxt[u], g0 + 4 * PF + 4 * u);
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      if (4 * u < n) {   // (uniform; n is a multiple of 4)
        const float a = sT[16 * w + li][a0 + 4 * u + lk];
#pragma unroll
        for (int ct = 0; ct < 8; ++ct)
          if (ct < nct) acc[ct] = mfma16(a, cur[u][ct], acc[ct]);
      }
    }
#pragma unroll
    for (int u = 0; u < PF; ++u)
#pragma unroll
      for (int ct = 0; ct < 8; ++ct) cur[u][ct] = nxt[u][ct];
  };
  for (int c = 0; c < R; ++c) {
    if (c > 0) __syncthreads();   // every wave is done with channel c - 1's tile
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = t + 256 * u, row = idx >> 5, c4 = idx & 31;
#pragma unroll
      for (int e = 0; e < 4; ++e) sT[row][4 * c4 + e] = z[u][e];
    }
    __syncthreads();
    if (c + 1 < R) fetch(c + 1);
    for (int k0 = 0; k0 < DH; k0 += 4 * PF) turn(c * DH + k0, k0, DH - k0);
  }
  for (int k0 = 0; k0 < Kp; k0 += 4 * PF) turn(RD + k0, DH + k0, Kp - k0);
#pragma unroll
  for (int ct = 0; ct < 8; ++ct)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = r0 + 16 * w + 4 * lk + j;
      if (r < N) dX[((int64_t)b * N + r) * DH + ct * 16 + li] = ct * 16 + li < d ? acc[ct][j] : 0.0f;
    }
}

}  // namespace

extern "C" int lnz_large_grad_project(float* dX, const float* Xout, const float* V, const int32_t* n_nodes,
                                      int B, int N, int K, float* part, float* A, float* db,
                                      lnz_stream_t stream) {
  LNZ_REQUIRE(dX && Xout && V && part && A && db && B > 0 && N > 0, LNZ_EINVAL,
              "lnz_large_grad_project: bad arguments (B=%d N=%d)", B, N);
  LNZ_REQUIRE(K >= 1 && K <= KMAX, LNZ_ENOTSUP, "lnz_large_grad_project: K=%d: 1 .. %d eigen directions", K, KMAX);
  LNZ_REQUIRE(B <= 65535, LNZ_ENOTSUP, "lnz_large_grad_project: B=%d > 65535 graphs", B);
  LNZ_REQUIRE(((((uintptr_t)dX) | ((uintptr_t)Xout)) & 15) == 0, LNZ_EINVAL,
              "lnz_large_grad_project: dX / Xout must be 16-byte aligned");
  const int chunks = (N + CHUNK - 1) / CHUNK;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(large_grad_project_kernel, dim3((unsigned)chunks, (unsigned)B), dim3(256), 0, s, dX, Xout,
                     V, n_nodes, B, N, K, chunks, part);
  hipLaunchKernelGGL(large_grad_project_reduce_kernel, dim3((unsigned)B), dim3(256), 0, s, part, K, chunks, A, db);
  lnz::note_kernel("large_grad_project_kernel");
  return lnz::check_launch("lnz_large_grad_project");
}

extern "C" int lnz_large_grad_spectral(const float* A, const float* Y, int ldy, const float* G, const float* W,
                                       int ldw, int B, int K, int S, int d, float* dG, float* Q, float* dY,
                                       lnz_stream_t stream) {
  LNZ_REQUIRE(A && Y && G && W && Q && dY && B > 0, LNZ_EINVAL, "lnz_large_grad_spectral: bad arguments");
  LNZ_REQUIRE(K >= 1 && K <= KMAX && S >= 1 && S <= SMAX && d >= 1 && d <= DH, LNZ_ENOTSUP,
              "lnz_large_grad_spectral: K=%d S=%d d=%d: K <= %d, S <= %d, d <= %d", K, S, d, KMAX, SMAX, DH);
  LNZ_REQUIRE(ldy >= d && ldw >= S * d, LNZ_EINVAL, "lnz_large_grad_spectral: ldy=%d / ldw=%d too small", ldy, ldw);
  hipLaunchKernelGGL(large_grad_spectral_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, A, Y, ldy,
                     G, W, ldw, K, S, d, dG, Q, dY);
  lnz::note_kernel("large_grad_spectral_kernel");
  return lnz::check_launch("lnz_large_grad_spectral");
}

// The two dX entries over the one kernel.  CHANNELS: the caller gives R and the [R][B][N][128] block of dZ, no
// channel of which dX may overlap; otherwise R = 1 and the entry's own check (dX is not dZ) is all there is.
template <bool CHANNELS>
static int launch_grad_input(const char* who, const float* dZ, const float* Wn, const float* V, const float* dY, int B,
                             int N, int K, int R, int d, float* dX, lnz_stream_t stream) {
  LNZ_REQUIRE(dZ && Wn && dX && dZ != dX && B > 0 && N > 0, LNZ_EINVAL,
              "%s: bad arguments (B=%d N=%d; dX must not alias dZ)", who, B, N);
  if (CHANNELS)
    LNZ_REQUIRE(R >= 1 && R <= RMAX && K >= 0 && K <= KMAX && d >= 1 && d <= DH, LNZ_ENOTSUP,
                "%s: R=%d K=%d d=%d: 1 <= R <= %d, K <= %d, 1 <= d <= %d", who, R, K, d, RMAX, KMAX, DH);
  else
    LNZ_REQUIRE(K >= 0 && K <= KMAX && d >= 1 && d <= DH, LNZ_ENOTSUP, "%s: K=%d d=%d: K <= %d, 1 <= d <= %d", who, K,
                d, KMAX, DH);
  LNZ_REQUIRE(K == 0 || (V && dY), LNZ_EINVAL, "%s: K=%d needs V and dY", who, K);
  LNZ_REQUIRE(B <= 65535, LNZ_ENOTSUP, "%s: B=%d > 65535 graphs", who, B);
  if (CHANNELS) {
    const uintptr_t block = (uintptr_t)B * N * DH * sizeof(float), z0 = (uintptr_t)dZ, x0 = (uintptr_t)dX;
    LNZ_REQUIRE(x0 + block <= z0 || z0 + (uintptr_t)R * block <= x0, LNZ_EINVAL,
                "%s: dX must not alias any channel of dZ", who);
  }
  LNZ_REQUIRE((((uintptr_t)dZ) & 15) == 0, LNZ_EINVAL, "%s: dZ must be 16-byte aligned", who);
  hipLaunchKernelGGL(large_grad_input_channels_kernel, dim3((unsigned)((N + IN_ROWS - 1) / IN_ROWS), (unsigned)B),
                     dim3(256), 0, (hipStream_t)stream, dZ, Wn, V, dY, B, N, K, R, d, dX);
  lnz::note_kernel("%s_kernel", who + sizeof("lnz_") - 1);
  return lnz::check_launch(who);
}

extern "C" int lnz_large_grad_input(const float* dZ, const float* Wn, const float* V, const float* dY, int B,
                                    int N, int K, int d, float* dX, lnz_stream_t stream) {
  return launch_grad_input<false>("lnz_large_grad_input", dZ, Wn, V, dY, B, N, K, 1, d, dX, stream);   // Wn [1][128][128]
}

extern "C" int lnz_large_grad_input_channels(const float* dZ, const float* Wn, const float* V, const float* dY,
                                             int B, int N, int K, int R, int d, float* dX, lnz_stream_t stream) {
  return launch_grad_input<true>("lnz_large_grad_input_channels", dZ, Wn, V, dY, B, N, K, R, d, dX, stream);
}
