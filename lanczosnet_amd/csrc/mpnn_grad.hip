// The backward of the MPNN baseline's edge-network propagation (mpnn.hip; reference model/mpnn.py:136-196
// under loss.backward()): one step of backpropagation through time per launch.
//
// lnz_mpnn_backward_step — from S_t (the trajectory of lnz_mpnn_forward_states) and dS' = dL/dS_{t+1}: the
// step is recomputed on chip with the forward's arithmetic ([P_c | Q_c], R_c, M_c: mpnn_tile.hpp's message
// block, the forward's own; gi, gh, r, z, n: ggnn_tile.hpp's gates and the cell's three expressions), then
//     dn = dS' (1 - z), dz = dS' (S - n), dS = dS' z
//     pn = dn (1 - n^2), pz = dz z (1 - z), pr = pn gh_n r (1 - r), pq = pn r
//     dgi = [pr, pz, pn], dgh = [pr, pz, pq], dS += dgh W_hh
//     per channel c: dM_c = dgi W_ih[:, cD:(c+1)D]  ('avg': divided by deg_c[a] + FLT_EPSILON) ;
//     dR_c = dM_c W2_c ; act_c[a, b, h] = edge (a, b, c) and Q_c[a, h] + P_c[b, h] > 0 ;
//     dQ_c[a, h] = dR_c[a, h] #{b : act_c[a, b, h]} ; dP_c[b, h] = sum over a ascending with act_c[a, b, h] of
//     dR_c[a, h] ; dS += dP_c W1n_c + dQ_c W1s_c
// Out: dS_t and the row-space operands of the step's weight gradients (dgi, the n part of dgh, cat_c M_c,
// cat_c R_c, the scaled dM, [dP_c | dQ_c]), which the caller contracts over all rows with the library GEMM —
// per-workgroup partials of the weights would be gigabytes.
//
// Shape as built: ggnn_grad.hip's.  A workgroup of eight waves owns floor(32 / N) whole molecules = at most
// 32 rows.  L is read once into the forward's row bit masks and degrees, plus the per-molecule transposes of
// the masks (bitsT: bit a of row b = edge (a, b)).  dgi is known only after all channels, so there are two
// channel loops: the first is the forward's (M_c and R_c also to global memory), the second recomputes
// [P_c | Q_c] — one 128-column product per channel; kept for all channels it would be 118 KB — next to dM_c,
// then dR_c (wave w: the hidden columns 16 (w & 3) .. of the row tile w >> 2), then the two masked sums on the
// VALU (one task per row and four hidden columns: its dQ over the row's bits, its dP over the row's transposed
// bits, a ascending), then the two products back into dS.  The data-gradient products contract over the OUTPUT
// index of a forward weight, so they read the transposed packs the caller makes once per weight version
// (W1T [C][2][D][64], W2T [C][64][D], WihT [C][D][3 D], WhhT [D][3 D]): tile_gemm wants weight rows contiguous
// along the contraction.  Every product is a k-ordered chain of its own (D or 64 terms) that is then added, as
// the forward adds its per-channel gi products (ggnn_grad.hip's header: one chain through all terms of dS
// measured 10 e32); dS accumulates in registers in the order dS' z, W_hh, channels ascending (dP, then dQ).
// Three barriers per channel in either loop.  LDS at D = 128: S, M_c / dM_c and the four planes pr, pz, pn, pq,
// 32 x 132 floats each, [P_c | Q_c] 32 x 132, R_c / dR_c 32 x 68, [dP_c | dQ_c] 32 x 132, bits, bitsT, degrees,
// rowbase: 147,072 B, one workgroup per CU.  No atomics, every sum in a fixed order: bit-reproducible.  The
// derivative factors z (1 - z), r (1 - r), 1 - n^2 are products of the forward's finite values: exact zeros at
// saturation, never inf - inf.  A row of degree 0 under 'avg' has dM / FLT_EPSILON, finite, and meets only
// R_c = 0, deg_c = 0 and a count of 0.
#include "common.hpp"
#include "ggnn_tile.hpp"
#include "mpnn_tile.hpp"

namespace {

constexpr int BRT = 2, BGR = 16 * BRT;   // row tiles and rows of a backward tile

// floats of dynamic LDS: S, M, four planes [BGR][D + 4], [P|Q] and [dP|dQ] [BGR][132], R [BGR][68],
// bits + bitsT + deg [8][BGR], rowbase
__host__ __device__ constexpr int mpnn_bwd_lds_floats(int D) {
  return 6 * BGR * (D + 4) + 2 * BGR * HS + BGR * RS + 3 * GMAXC * BGR + BGR;
}

template <int D>
__global__ __launch_bounds__(GNT) void mpnn_backward_step_kernel(
    const float* __restrict__ S, const int lds_, const float* __restrict__ dSn, const int ldd,
    const float* __restrict__ L, const int64_t stride_b, const int64_t stride_r, const int64_t stride_c,
    const int64_t stride_ch, const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ Wih,
    const float* __restrict__ bih, const float* __restrict__ Whh, const float* __restrict__ bhh,
    const float* __restrict__ W1T, const float* __restrict__ W2T, const float* __restrict__ WihT,
    const float* __restrict__ WhhT, const int B, const int N, const int C, const int avg,
    float* __restrict__ dS, const int ldo, float* __restrict__ dgi, float* __restrict__ dghn,
    float* __restrict__ Mcat, float* __restrict__ Rcat, float* __restrict__ dM, float* __restrict__ dPQ) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int RT = BRT, GR = BGR;
  constexpr int SS = D + 4;
  constexpr int DB = D / 16;
  constexpr int HQ = MHID / 4;
  float* const Sb = smem;
  float* const Mb = Sb + GR * SS;    // M_c, then dM_c
  float* const Pr = Mb + GR * SS;    // dr_pre
  float* const Pz = Pr + GR * SS;    // dz_pre
  float* const Pn = Pz + GR * SS;    // dn_pre
  float* const Pq = Pn + GR * SS;    // dn_pre r
  float* const Hb = Pq + GR * SS;    // [row][P_c 0..63 | Q_c 64..127]
  float* const Gb = Hb + GR * HS;    // [row][dP_c 0..63 | dQ_c 64..127]
  float* const Rb = Gb + GR * HS;    // R_c, then dR_c
  unsigned* const bits = reinterpret_cast<unsigned*>(Rb + GR * RS);   // [c][row]: bit j = edge (row, j)
  unsigned* const bitsT = bits + GMAXC * GR;                           // [c][row]: bit i = edge (i, row)
  float* const deg = reinterpret_cast<float*>(bitsT + GMAXC * GR);     // [c][row]
  int* const rowbase = reinterpret_cast<int*>(deg + GMAXC * GR);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 15, g = lane >> 4;
  const TileSpan ts = tile_span<RT>(B, N);
  const int rows = ts.rows;
  const int64_t row0 = ts.mol0 * N;   // first global row of the tile

  // ---- the state, the bit masks and degrees of L: the forward's prologue
  load_state_tile<D, RT>(Sb, S, row0, lds_, rows);
  load_edge_bits<RT>(bits, L, stride_b, stride_r, stride_c, stride_ch, ts, N, C,
                     [&](const int at, const int degree) { deg[at] = (float)degree; });
  set_rowbase<RT>(rowbase, N, rows);
  __syncthreads();
  transpose_edge_bits<RT>(bitsT, bits, rowbase, N, C, rows);
  // (the barriers of the first channel loop stand between this and the first read of bitsT)

  const bool owner = wave < DB;
  const int f0 = 16 * wave + 4 * g;
  const float* const m_frag = Mb + m * SS + 4 * g;
  const int fo = m * SS + 4 * g;   // the fragment offset in a plane
  const EdgeTile et = {Sb, Mb, Hb, Rb, bits, deg, rowbase};

  // ---- the step, recomputed: the forward's channel loop, R_c and M_c also to global memory
  f32x4 acc[3][RT];
  zero_tiles(acc);
  for (int c = 0; c < C; ++c) {
    edge_message<D, RT>(
        et, c, W1, b1, W2, b2, avg, wave, m, g,
        [&](const int r, const int q, const f32x4& s) {
          if (r < rows) *reinterpret_cast<f32x4*>(Rcat + (row0 + r) * ((int64_t)C * MHID) + c * MHID + 4 * q) = s;
        },
        [&](const int rt, const f32x4& v) {
          if (16 * rt + m < rows)
            *reinterpret_cast<f32x4*>(Mcat + (row0 + 16 * rt + m) * ((int64_t)C * D) + c * D + f0) = v;
        });
    if (owner) gate_accumulate<D, RT>(m_frag, Wih, c, C, wave, m, g, acc);
  }
  // ---- the cell and its backward (ggnn_tile.hpp): the planes, dgi, dghn, and dS_t = dS' z + dgh W_hh so far
  f32x4 ds[1][RT];   // dS_t of this lane's four features
  LNZ_GRU_CELL_BACKWARD(D, RT);
  const int cb = wave & 3, hrt = wave >> 2;   // dR_c: this wave's block of 16 hidden columns and its row tile
  for (int c = 0; c < C; ++c) {
    // [P_c | Q_c] again (every wave has passed the barrier behind the last read of Hb and Mb)
    edge_hidden<D, RT>(et, c, W1, b1, wave, m, g);
    if (owner) {   // dM_c = dgi W_ih[:, cD ..]: feature k = row k of WihT[c]; 'avg': the forward's division
      f32x4 da[1][RT], da1[1][RT], da2[1][RT];
      zero_tiles(da), zero_tiles(da1), zero_tiles(da2);
      const float* const row = WihT + ((int64_t)c * D + 16 * wave + m) * (3 * D) + 4 * g;
      const float* const w0[1] = {row};
      const float* const w1[1] = {row + D};
      const float* const w2[1] = {row + 2 * D};
      tile_gemm<1, DB, RT>(Pr + fo, SS, w0, da);
      tile_gemm<1, DB, RT>(Pz + fo, SS, w1, da1);
      tile_gemm<1, DB, RT>(Pn + fo, SS, w2, da2);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const int rl = 16 * rt + m;
        f32x4 v = (da[0][rt] + da1[0][rt]) + da2[0][rt];
        if (avg) v = v / (deg[c * GR + rl] + FLT_EPSILON);
        *reinterpret_cast<f32x4*>(Mb + rl * SS + f0) = v;
        if (rl < rows) *reinterpret_cast<f32x4*>(dM + (row0 + rl) * ((int64_t)C * D) + c * D + f0) = v;
      }
    }
    __syncthreads();
    {   // dR_c = dM_c W2_c: hidden column h = row h of W2T[c]
      f32x4 dr[1][1] = {{f32x4{0.0f, 0.0f, 0.0f, 0.0f}}};
      const float* const wp[1] = {W2T + ((int64_t)c * MHID + 16 * cb + m) * D + 4 * g};
      tile_gemm<1, DB, 1>(Mb + (16 * hrt + m) * SS + 4 * g, SS, wp, dr);
      *reinterpret_cast<f32x4*>(Rb + (16 * hrt + m) * RS + 16 * cb + 4 * g) = dr[0][0];
    }
    __syncthreads();
    // the two masked sums of a row: dQ_c over its bits, dP_c over its transposed bits (a ascending)
    for (int idx = tid; idx < GR * HQ; idx += GNT) {
      const int r = idx / HQ, q = idx - r * HQ;
      const int base = rowbase[r];
      const f32x4 pv = *reinterpret_cast<const f32x4*>(Hb + r * HS + 4 * q);
      const f32x4 qv = *reinterpret_cast<const f32x4*>(Hb + r * HS + MHID + 4 * q);
      const f32x4 dr = *reinterpret_cast<const f32x4*>(Rb + r * RS + 4 * q);
      f32x4 cnt = {0.0f, 0.0f, 0.0f, 0.0f}, dp = {0.0f, 0.0f, 0.0f, 0.0f};
      for (unsigned bm = bits[c * GR + r]; bm; bm &= bm - 1) {
        const int j = __ffs(bm) - 1;
        const f32x4 v = *reinterpret_cast<const f32x4*>(Hb + (base + j) * HS + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) cnt[e] += qv[e] + v[e] > 0.0f ? 1.0f : 0.0f;
      }
      for (unsigned bm = bitsT[c * GR + r]; bm; bm &= bm - 1) {
        const int i = __ffs(bm) - 1;
        const f32x4 qa = *reinterpret_cast<const f32x4*>(Hb + (base + i) * HS + MHID + 4 * q);
        const f32x4 da = *reinterpret_cast<const f32x4*>(Rb + (base + i) * RS + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) dp[e] += qa[e] + pv[e] > 0.0f ? da[e] : 0.0f;
      }
      f32x4 dq;
#pragma unroll
      for (int e = 0; e < 4; ++e) dq[e] = dr[e] * cnt[e];
      *reinterpret_cast<f32x4*>(Gb + r * HS + 4 * q) = dp;
      *reinterpret_cast<f32x4*>(Gb + r * HS + MHID + 4 * q) = dq;
      if (r < rows) {
        float* const gp = dPQ + (row0 + r) * ((int64_t)C * 2 * MHID) + c * (2 * MHID) + 4 * q;
        *reinterpret_cast<f32x4*>(gp) = dp;
        *reinterpret_cast<f32x4*>(gp + MHID) = dq;
      }
    }
    __syncthreads();
    if (owner) {   // dS += dP_c W1n_c + dQ_c W1s_c: feature k = row k of W1T[c][0] and of W1T[c][1]
      const float* const row = W1T + ((int64_t)c * 2 * D + 16 * wave + m) * MHID + 4 * g;
      const float* const wn[1] = {row};
      const float* const ws[1] = {row + D * MHID};
      f32x4 pp[1][RT], pq[1][RT];
      zero_tiles(pp), zero_tiles(pq);
      tile_gemm<1, MHID / 16, RT>(Gb + m * HS + 4 * g, HS, wn, pp);
      tile_gemm<1, MHID / 16, RT>(Gb + m * HS + MHID + 4 * g, HS, ws, pq);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) ds[0][rt] += pp[0][rt] + pq[0][rt];
    }
  }
  if (owner) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
      if (16 * rt + m < rows)
        *reinterpret_cast<f32x4*>(dS + (row0 + 16 * rt + m) * (int64_t)ldo + f0) = ds[0][rt];
  }
}

template <int D>
int launch_step(const float* S, int lds_, const float* dSn, int ldd, const float* L, int64_t sb, int64_t sr,
                int64_t sc, int64_t sch, const float* W1, const float* b1, const float* W2, const float* b2,
                const float* Wih, const float* bih, const float* Whh, const float* bhh, const float* W1T,
                const float* W2T, const float* WihT, const float* WhhT, int B, int N, int C, int avg, float* dS,
                int ldo, float* dgi, float* dghn, float* Mcat, float* Rcat, float* dM, float* dPQ, int grid,
                hipStream_t s) {
  const size_t lds = sizeof(float) * (size_t)mpnn_bwd_lds_floats(D);
  auto kfn = mpnn_backward_step_kernel<D>;
  LNZ_DYNAMIC_LDS(kfn, lds, "mpnn_grad.hip");
  hipLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(GNT), lds, s, S, lds_, dSn, ldd, L, sb, sr, sc, sch, W1, b1, W2,
                     b2, Wih, bih, Whh, bhh, W1T, W2T, WihT, WhhT, B, N, C, avg, dS, ldo, dgi, dghn, Mcat, Rcat, dM,
                     dPQ);
  return lnz::check_launch("lnz_mpnn_backward_step");
}

}  // namespace

extern "C" int lnz_mpnn_backward_step(const float* S, int lds, const float* dSnext, int ldd, const float* L,
                                      int64_t stride_b, int64_t stride_r, int64_t stride_c, int64_t stride_ch,
                                      const float* W1, const float* b1, const float* W2, const float* b2,
                                      const float* Wih, const float* bih, const float* Whh, const float* bhh,
                                      const float* W1T, const float* W2T, const float* WihT, const float* WhhT,
                                      int B, int N, int C, int D, int avg, float* dS, int ldo, float* dgi,
                                      float* dghn, float* M, float* R, float* dM, float* dPQ,
                                      lnz_stream_t stream) {
  LNZ_REQUIRE(S && dSnext && L && W1 && b1 && W2 && b2 && Wih && bih && Whh && bhh && W1T && W2T && WihT && WhhT &&
                  dS && dgi && dghn && M && R && dM && dPQ,
              LNZ_EINVAL, "lnz_mpnn_backward_step: null pointer");
  LNZ_REQUIRE(B > 0 && N > 0, LNZ_EINVAL, "lnz_mpnn_backward_step: B = %d, N = %d must be positive", B, N);
  LNZ_REQUIRE(N <= GMAXN && C >= 1 && C <= GMAXC && D >= 32 && D <= GMAXD && D % 32 == 0, LNZ_ENOTSUP,
              "lnz_mpnn_backward_step: N = %d, C = %d, D = %d outside 1 <= N <= 32, 1 <= C <= 8, D a multiple of 32 "
              "and <= 128", N, C, D);
  LNZ_REQUIRE(lds >= D && ldd >= D && ldo >= D, LNZ_EINVAL,
              "lnz_mpnn_backward_step: lds = %d, ldd = %d, ldo = %d below the width %d", lds, ldd, ldo, D);
  LNZ_REQUIRE(stride_b >= 0 && stride_r >= 0 && stride_c >= 0 && stride_ch >= 0, LNZ_EINVAL,
              "lnz_mpnn_backward_step: negative stride of L");
  LNZ_REQUIRE(lds % 4 == 0 && ldd % 4 == 0 && ldo % 4 == 0 && aligned16(S) && aligned16(dSnext) && aligned16(dS) &&
                  aligned16(W1) && aligned16(b1) && aligned16(W2) && aligned16(b2) && aligned16(Wih) &&
                  aligned16(bih) && aligned16(Whh) && aligned16(bhh) && aligned16(W1T) && aligned16(W2T) &&
                  aligned16(WihT) && aligned16(WhhT) && aligned16(dgi) && aligned16(dghn) && aligned16(M) &&
                  aligned16(R) && aligned16(dM) && aligned16(dPQ),
              LNZ_ENOTSUP, "lnz_mpnn_backward_step: the rows of S, dSnext, dS, of the weights and of the row-space "
              "buffers must be 16-byte aligned (lds = %d, ldd = %d, ldo = %d)", lds, ldd, ldo);
  {
    const uint64_t rows = (uint64_t)B * N;
    const void* in[2] = {S, dSnext};
    const uint64_t nin[2] = {span(rows, lds, D), span(rows, ldd, D)};
    const void* out[7] = {dS, dgi, dghn, M, R, dM, dPQ};
    const uint64_t nout[7] = {span(rows, ldo, D),         span(rows, 3 * D, 3 * D),       span(rows, D, D),
                              span(rows, C * D, C * D),   span(rows, C * MHID, C * MHID), span(rows, C * D, C * D),
                              span(rows, 2 * C * MHID, 2 * C * MHID)};
    for (int o = 0; o < 7; ++o) {
      for (int i = 0; i < 2; ++i)
        LNZ_REQUIRE(!overlap(out[o], nout[o], in[i], nin[i]), LNZ_EINVAL,
                    "lnz_mpnn_backward_step: an output aliases S or dSnext");
      for (int p = 0; p < o; ++p)
        LNZ_REQUIRE(!overlap(out[o], nout[o], out[p], nout[p]), LNZ_EINVAL,
                    "lnz_mpnn_backward_step: two outputs alias each other");
    }
  }
  const int mpt = BGR / N;
  const int64_t grid = ((int64_t)B + mpt - 1) / mpt;
  hipStream_t s = (hipStream_t)stream;
  lnz::note_kernel("mpnn_backward_step_kernel<%d>", D);
#define LNZ_MPNN_STEP(DD)                                                                                      \
  launch_step<DD>(S, lds, dSnext, ldd, L, stride_b, stride_r, stride_c, stride_ch, W1, b1, W2, b2, Wih, bih, Whh, \
                  bhh, W1T, W2T, WihT, WhhT, B, N, C, avg ? 1 : 0, dS, ldo, dgi, dghn, M, R, dM, dPQ, (int)grid, s)
  LNZ_GGNN_WIDTHS(D, LNZ_MPNN_STEP)
#undef LNZ_MPNN_STEP
}
