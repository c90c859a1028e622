// The backward of the GGNN baseline's gated propagation (ggnn.hip; reference model/ggnn.py:137-197 under
// loss.backward()): one step of backpropagation through time per launch, and the readout's backward.
//
// lnz_ggnn_backward_step — from S_t (the trajectory of lnz_ggnn_forward_states) and dS' = dL/dS_{t+1}: the
// step is recomputed on chip with the forward's arithmetic (H_c, M_c, A_c, gi, gh, r, z, n: the forward's own
// routines of ggnn_tile.hpp — its prologue, message block, gates and the cell's three expressions), then
//     dn = dS' (1 - z), dz = dS' (S - n), dS = dS' z
//     dn_pre = dn (1 - n^2), dz_pre = dz z (1 - z), dr_pre = dn_pre gh_n r (1 - r)
//     dgi = [dr_pre, dz_pre, dn_pre], dgh = [dr_pre, dz_pre, dn_pre r]
//     dS += dgh W_hh
//     per channel c: dA_c = dgi W_ih[:, cD:(c+1)D] ; dM_c = Â_c^T dA_c per molecule ('avg': scaled by
//     the reciprocal of the DESTINATION row i, set bits in ascending i) ; dHpre_c = (dM_c W2_c) [H_c > 0] ;
//     dS += dHpre_c W1_c
// Out: dS_t and the row-space operands of the step's weight gradients (dgi, the n part of dgh, cat_c A_c,
// dM, H, dHpre), which the caller contracts over all rows with the library GEMM — per-workgroup partials of
// 2.5 MB of weights would be gigabytes.
//
// Shape as built.  The forward's tile at its lower height: a workgroup of eight waves owns floor(32 / N)
// whole molecules = at most 32 rows (N <= 32 fits no lower height, and 64 rows would need 16 buffers:
// 270 KB).  L is read once into the forward's row bit masks and 'avg' reciprocals, plus their per-molecule
// transposes.  The data-gradient products contract over the OUTPUT index of a forward weight, so they
// read the transposed weights the caller packs once per weight version (W1T [C][D][128], W2T [C][128][D],
// WihT [C][D][3 D], WhhT [D][3 D]): tile_gemm wants weight rows contiguous along the contraction.  A
// contraction over 3 D is three calls over the r, z and n planes.  Wave w owns the hidden columns 16 w ..
// and, where 16 w < D, the features 16 w ..; the sign of H_c lives in a 64-bit register mask across the two
// channel loops (bit 8 c + 4 rt + e), dS accumulates in registers in the order dS' z, W_hh, channels
// ascending.  Every product is a k-ordered chain of its own (D or 128 terms) that is then added, as the
// forward adds its per-channel gi products: one chain through all 3 D + C 128 terms of dS measured 10 e32 at
// D = 128, C = 7.  LDS at D = 128: S, M_c, A_c and the four planes dr_pre, dz_pre, dn_pre, dn_pre r, 32 x 132
// floats each, H_c 32 x 132, masks: 138,368 B, one workgroup per CU.  No atomics, every sum in a fixed
// order: bit-reproducible.  The derivative factors z (1 - z), r (1 - r), 1 - n^2 are products of the
// forward's finite values: exact zeros at saturation, never inf - inf.
//
// lnz_ggnn_readout_backward — lnz_gat_readout_backward's scheme (a workgroup per molecule, per-molecule
// partials in a workspace, added in a fixed order by a second launch) at the GGNN's width D <= 128.
#include "common.hpp"
#include "ggnn_tile.hpp"
#include "partial_sum.hpp"

namespace {

constexpr int BRT = 2, BGR = 16 * BRT;   // row tiles and rows of a backward tile

// floats of dynamic LDS: S, M, A, four planes [BGR][D + 4], H [BGR][132], bits + bitsT + inv [8][BGR], rowbase
__host__ __device__ constexpr int ggnn_bwd_lds_floats(int D) {
  return 7 * BGR * (D + 4) + BGR * HS + 3 * GMAXC * BGR + BGR;
}

template <int D>
__global__ __launch_bounds__(GNT) void ggnn_backward_step_kernel(
    const float* __restrict__ S, const int lds_, const float* __restrict__ dSn, const int ldd,
    const float* __restrict__ L, const int64_t stride_b, const int64_t stride_r, const int64_t stride_c,
    const int64_t stride_ch, const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ Wih,
    const float* __restrict__ bih, const float* __restrict__ Whh, const float* __restrict__ bhh,
    const float* __restrict__ W1T, const float* __restrict__ W2T, const float* __restrict__ WihT,
    const float* __restrict__ WhhT, const int B, const int N, const int C, const int avg,
    float* __restrict__ dS, const int ldo, float* __restrict__ dgi, float* __restrict__ dghn,
    float* __restrict__ Acat, float* __restrict__ dM, float* __restrict__ Hcat, float* __restrict__ dHpre) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int RT = BRT, GR = BGR;
  constexpr int SS = D + 4;
  constexpr int DQ = D / 4;
  constexpr int DB = D / 16;
  float* const Sb = smem;
  float* const Mb = Sb + GR * SS;
  float* const Ab = Mb + GR * SS;
  float* const Pr = Ab + GR * SS;    // dr_pre
  float* const Pz = Pr + GR * SS;    // dz_pre
  float* const Pn = Pz + GR * SS;    // dn_pre
  float* const Pq = Pn + GR * SS;    // dn_pre r
  float* const Hb = Pq + GR * SS;
  unsigned* const bits = reinterpret_cast<unsigned*>(Hb + GR * HS);   // [c][row]: bit j = edge (row, j)
  unsigned* const bitsT = bits + GMAXC * GR;                           // [c][row]: bit i = edge (i, row)
  float* const inv = reinterpret_cast<float*>(bitsT + GMAXC * GR);     // [c][row]
  int* const rowbase = reinterpret_cast<int*>(inv + GMAXC * GR);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 15, g = lane >> 4;
  const TileSpan ts = tile_span<RT>(B, N);
  const int rows = ts.rows;
  const int64_t row0 = ts.mol0 * N;   // first global row of the tile

  // ---- the state, the bit masks and denominators of L: the forward's prologue
  load_state_tile<D, RT>(Sb, S, row0, lds_, rows);
  load_edge_bits<RT>(bits, L, stride_b, stride_r, stride_c, stride_ch, ts, N, C,
                     [&](const int at, const int degree) { inv[at] = ggnn_edge_weight(avg, degree); });
  set_rowbase<RT>(rowbase, N, rows);
  __syncthreads();
  transpose_edge_bits<RT>(bitsT, bits, rowbase, N, C, rows);
  // (the barriers of the channel loop stand between this and the first read of bitsT)

  const bool owner = wave < DB;
  const int f0 = 16 * wave + 4 * g;
  const float* const h_frag = Hb + m * HS + 4 * g;
  const float* const a_frag = Ab + m * SS + 4 * g;
  const float* const m_frag = Mb + m * SS + 4 * g;
  const int fo = m * SS + 4 * g;   // the fragment offset in a plane

  // ---- the step, recomputed: the forward's channel loop, H_c and A_c also to global memory
  unsigned long long hpos = 0;     // bit 8 c + 4 rt + e: H_c > 0 at (row 16 rt + m, hidden column f0 + e)
  const MessageTile mt = {Sb, Mb, Ab, Hb, bits, inv, rowbase};
  f32x4 acc[3][RT];
  zero_tiles(acc);
  for (int c = 0; c < C; ++c) {
    ggnn_message<D, RT>(
        mt, c, W1, b1, W2, b2, wave, m, g,
        [&](const int rt, const f32x4& v) {
#pragma unroll
          for (int e = 0; e < 4; ++e) hpos |= (unsigned long long)(v[e] > 0.0f ? 1u : 0u) << (8 * c + 4 * rt + e);
          if (16 * rt + m < rows)
            *reinterpret_cast<f32x4*>(Hcat + (row0 + 16 * rt + m) * ((int64_t)C * GHID) + c * GHID + f0) = v;
        },
        [&](const int r, const int q, const f32x4& s) {
          if (r < rows) *reinterpret_cast<f32x4*>(Acat + (row0 + r) * ((int64_t)C * D) + c * D + 4 * q) = s;
        });
    if (owner) gate_accumulate<D, RT>(a_frag, Wih, c, C, wave, m, g, acc);
  }
  // ---- the cell and its backward (ggnn_tile.hpp): the planes, dgi, dghn, and dS_t = dS' z + dgh W_hh so far
  f32x4 ds[1][RT];   // dS_t of this lane's four features
  LNZ_GRU_CELL_BACKWARD(D, RT);
  for (int c = 0; c < C; ++c) {
    if (owner) {   // dA_c = dgi W_ih[:, cD ..]: feature k = row k of WihT[c]
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
      for (int rt = 0; rt < RT; ++rt)
        *reinterpret_cast<f32x4*>(Ab + (16 * rt + m) * SS + f0) = (da[0][rt] + da1[0][rt]) + da2[0][rt];
    }
    __syncthreads();
    // dM_c = Â_c^T dA_c: row j gathers the rows i with an edge (i, j), ascending i, each scaled by row i's weight
    for (int idx = tid; idx < GR * DQ; idx += GNT) {
      const int r = idx / DQ, q = idx - r * DQ;
      unsigned bm = bitsT[c * GR + r];
      const int base = rowbase[r];
      const float* const src = Ab + base * SS + 4 * q;
      const float* const wsrc = inv + c * GR + base;
      f32x4 s = {0.0f, 0.0f, 0.0f, 0.0f};
      while (bm) {
        const int i = __ffs(bm) - 1;
        bm &= bm - 1;
        const float wgt = wsrc[i];
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + i * SS);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] = fmaf(wgt, v[e], s[e]);
      }
      *reinterpret_cast<f32x4*>(Mb + r * SS + 4 * q) = s;
      if (r < rows) *reinterpret_cast<f32x4*>(dM + (row0 + r) * ((int64_t)C * D) + c * D + 4 * q) = s;
    }
    __syncthreads();
    {   // dHpre_c = (dM_c W2_c) [H_c > 0]: hidden column h = row h of W2T[c]
      f32x4 dh[1][RT];
      zero_tiles(dh);
      const float* const wp[1] = {W2T + ((int64_t)c * GHID + 16 * wave + m) * D + 4 * g};
      tile_gemm<1, DB, RT>(m_frag, SS, wp, dh);
      const unsigned hm = (unsigned)(hpos >> (8 * c)) & 0xffu;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (hm >> (4 * rt + e)) & 1u ? dh[0][rt][e] : 0.0f;
        *reinterpret_cast<f32x4*>(Hb + (16 * rt + m) * HS + f0) = v;
        if (16 * rt + m < rows)
          *reinterpret_cast<f32x4*>(dHpre + (row0 + 16 * rt + m) * ((int64_t)C * GHID) + c * GHID + f0) = v;
      }
    }
    __syncthreads();
    if (owner) {   // dS += dHpre_c W1_c: feature k = row k of W1T[c]
      const float* const wp[1] = {W1T + ((int64_t)c * D + 16 * wave + m) * GHID + 4 * g};
      f32x4 part[1][RT];
      zero_tiles(part);
      tile_gemm<1, GHID / 16, RT>(h_frag, HS, wp, part);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) ds[0][rt] += part[0][rt];
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
                int ldo, float* dgi, float* dghn, float* Acat, float* dM, float* Hcat, float* dHpre, int grid,
                hipStream_t s) {
  const size_t lds = sizeof(float) * (size_t)ggnn_bwd_lds_floats(D);
  auto kfn = ggnn_backward_step_kernel<D>;
  LNZ_DYNAMIC_LDS(kfn, lds, "ggnn_grad.hip");
  hipLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(GNT), lds, s, S, lds_, dSn, ldd, L, sb, sr, sc, sch, W1, b1, W2,
                     b2, Wih, bih, Whh, bhh, W1T, W2T, WihT, WhhT, B, N, C, avg, dS, ldo, dgi, dghn, Acat, dM, Hcat,
                     dHpre);
  return lnz::check_launch("lnz_ggnn_backward_step");
}

// ---------------------------------------------------------------------------------------- readout
constexpr int XS = GMAXD + 1;   // row stride of x in LDS

__global__ __launch_bounds__(256) void ggnn_readout_backward_kernel(
    const float* __restrict__ Slast, int ld, const unsigned char* __restrict__ mask, const float* __restrict__ Wo,
    const float* __restrict__ bo, const float* __restrict__ wg, const float* __restrict__ bg,
    const float* __restrict__ dscore, int N, int D, int P, float* __restrict__ ws, float* __restrict__ dSlast,
    int ldg) {
  __shared__ float xs[GMAXN * XS];
  __shared__ float ys[GMAXN * (GMAXP + 1)];
  __shared__ float gs[GMAXN];    // the gate of a masked row, 0 outside the mask
  __shared__ float zs[GMAXN];    // dzg of a masked row, 0 outside the mask
  __shared__ int ins[GMAXN];     // row in the mask
  __shared__ float dys[GMAXP];   // dscore / cnt
  const int64_t b = blockIdx.x;
  const float* Sm = Slast + (b * N) * (int64_t)ld;
  for (int t = threadIdx.x; t < N * D; t += 256) {
    const int i = t / D, d = t - i * D;
    xs[i * XS + d] = Sm[(int64_t)i * ld + d];
  }
  __syncthreads();
  // o and g as the forward computes them
  for (int t = threadIdx.x; t < N * (P + 1); t += 256) {
    const int i = t / (P + 1), p = t - i * (P + 1);
    const float* w = p < P ? Wo + (int64_t)p * D : wg;
    float a = 0.0f;
    for (int d = 0; d < D; ++d) a = fmaf(xs[i * XS + d], w[d], a);
    a += p < P ? bo[p] : bg[0];
    ys[i * (GMAXP + 1) + p] = p < P ? a : sigmoidf_(a);
  }
  if (threadIdx.x < P) {
    float cnt = 0.0f;
    for (int i = 0; i < N; ++i)
      if (mask == nullptr || mask[b * N + i] != 0) cnt += 1.0f;
    dys[threadIdx.x] = dscore[b * P + threadIdx.x] / cnt;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    const int i = threadIdx.x;
    const bool in = mask == nullptr || mask[b * N + i] != 0;
    const float g = ys[i * (GMAXP + 1) + P];
    float s = 0.0f;
    for (int p = 0; p < P; ++p) s = fmaf(dys[p], ys[i * (GMAXP + 1) + p], s);
    ins[i] = in ? 1 : 0;
    gs[i] = in ? g : 0.0f;
    zs[i] = in ? s * (g * (1.0f - g)) : 0.0f;
  }
  __syncthreads();
  // dx = Wo^T do + wg dzg, p ascending; exactly 0 outside the mask
  float* Gm = dSlast + (b * N) * (int64_t)ldg;
  for (int t = threadIdx.x; t < N * D; t += 256) {
    const int i = t / D, d = t - i * D;
    float a = 0.0f;
    if (ins[i]) {
      for (int p = 0; p < P; ++p) a = fmaf(Wo[(int64_t)p * D + d], dys[p] * gs[i], a);
      a = fmaf(wg[d], zs[i], a);
    }
    Gm[(int64_t)i * ldg + d] = a;
  }
  // the molecule's partials [dWo P D | dbo P | dwg D | dbg 1], i ascending (rows outside the mask add 0)
  const int M = P * D + P + D + 1;
  float* part = ws + b * (int64_t)M;
  for (int t = threadIdx.x; t < M; t += 256) {
    float a = 0.0f;
    if (t < P * D) {
      const int p = t / D, d = t - p * D;
      for (int i = 0; i < N; ++i) a = fmaf(dys[p] * gs[i], xs[i * XS + d], a);
    } else if (t < P * D + P) {
      const int p = t - P * D;
      for (int i = 0; i < N; ++i) a += dys[p] * gs[i];
    } else if (t < P * D + P + D) {
      const int d = t - P * D - P;
      for (int i = 0; i < N; ++i) a = fmaf(zs[i], xs[i * XS + d], a);
    } else {
      for (int i = 0; i < N; ++i) a += zs[i];
    }
    part[t] = a;
  }
}

}  // namespace

extern "C" int lnz_ggnn_backward_step(const float* S, int lds, const float* dSnext, int ldd, const float* L,
                                      int64_t stride_b, int64_t stride_r, int64_t stride_c, int64_t stride_ch,
                                      const float* W1, const float* b1, const float* W2, const float* b2,
                                      const float* Wih, const float* bih, const float* Whh, const float* bhh,
                                      const float* W1T, const float* W2T, const float* WihT, const float* WhhT,
                                      int B, int N, int C, int D, int avg, float* dS, int ldo, float* dgi,
                                      float* dghn, float* A, float* dM, float* H, float* dHpre,
                                      lnz_stream_t stream) {
  LNZ_REQUIRE(S && dSnext && L && W1 && b1 && W2 && b2 && Wih && bih && Whh && bhh && W1T && W2T && WihT && WhhT &&
                  dS && dgi && dghn && A && dM && H && dHpre,
              LNZ_EINVAL, "lnz_ggnn_backward_step: null pointer");
  LNZ_REQUIRE(B > 0 && N > 0, LNZ_EINVAL, "lnz_ggnn_backward_step: B = %d, N = %d must be positive", B, N);
  LNZ_REQUIRE(N <= GMAXN && C >= 1 && C <= GMAXC && D >= 32 && D <= GMAXD && D % 32 == 0, LNZ_ENOTSUP,
              "lnz_ggnn_backward_step: N = %d, C = %d, D = %d outside 1 <= N <= 32, 1 <= C <= 8, D a multiple of 32 "
              "and <= 128", N, C, D);
  LNZ_REQUIRE(lds >= D && ldd >= D && ldo >= D, LNZ_EINVAL,
              "lnz_ggnn_backward_step: lds = %d, ldd = %d, ldo = %d below the width %d", lds, ldd, ldo, D);
  LNZ_REQUIRE(stride_b >= 0 && stride_r >= 0 && stride_c >= 0 && stride_ch >= 0, LNZ_EINVAL,
              "lnz_ggnn_backward_step: negative stride of L");
  LNZ_REQUIRE(lds % 4 == 0 && ldd % 4 == 0 && ldo % 4 == 0 && aligned16(S) && aligned16(dSnext) && aligned16(dS) &&
                  aligned16(W1) && aligned16(b1) && aligned16(W2) && aligned16(b2) && aligned16(Wih) &&
                  aligned16(bih) && aligned16(Whh) && aligned16(bhh) && aligned16(W1T) && aligned16(W2T) &&
                  aligned16(WihT) && aligned16(WhhT) && aligned16(dgi) && aligned16(dghn) && aligned16(A) &&
                  aligned16(dM) && aligned16(H) && aligned16(dHpre),
              LNZ_ENOTSUP, "lnz_ggnn_backward_step: the rows of S, dSnext, dS, of the weights and of the row-space "
              "buffers must be 16-byte aligned (lds = %d, ldd = %d, ldo = %d)", lds, ldd, ldo);
  {
    const uint64_t rows = (uint64_t)B * N;
    const void* in[2] = {S, dSnext};
    const uint64_t nin[2] = {span(rows, lds, D), span(rows, ldd, D)};
    const void* out[7] = {dS, dgi, dghn, A, dM, H, dHpre};
    const uint64_t nout[7] = {span(rows, ldo, D),     span(rows, 3 * D, 3 * D),       span(rows, D, D),
                              span(rows, C * D, C * D), span(rows, C * D, C * D),     span(rows, C * GHID, C * GHID),
                              span(rows, C * GHID, C * GHID)};
    for (int o = 0; o < 7; ++o) {
      for (int i = 0; i < 2; ++i)
        LNZ_REQUIRE(!overlap(out[o], nout[o], in[i], nin[i]), LNZ_EINVAL,
                    "lnz_ggnn_backward_step: an output aliases S or dSnext");
      for (int p = 0; p < o; ++p)
        LNZ_REQUIRE(!overlap(out[o], nout[o], out[p], nout[p]), LNZ_EINVAL,
                    "lnz_ggnn_backward_step: two outputs alias each other");
    }
  }
  const int mpt = BGR / N;
  const int64_t grid = ((int64_t)B + mpt - 1) / mpt;
  hipStream_t s = (hipStream_t)stream;
  lnz::note_kernel("ggnn_backward_step_kernel<%d>", D);
#define LNZ_GGNN_STEP(DD)                                                                                      \
  launch_step<DD>(S, lds, dSnext, ldd, L, stride_b, stride_r, stride_c, stride_ch, W1, b1, W2, b2, Wih, bih, Whh, \
                  bhh, W1T, W2T, WihT, WhhT, B, N, C, avg ? 1 : 0, dS, ldo, dgi, dghn, A, dM, H, dHpre, (int)grid, s)
  LNZ_GGNN_WIDTHS(D, LNZ_GGNN_STEP)
#undef LNZ_GGNN_STEP
}

extern "C" int64_t lnz_ggnn_readout_backward_workspace_floats(int B, int D, int P) {
  if (B <= 0 || D <= 0 || P <= 0) return 0;
  return (int64_t)B * ((int64_t)P * D + P + D + 1);
}

extern "C" int lnz_ggnn_readout_backward(const float* Slast, int ld, const uint8_t* mask, const float* Wo,
                                         const float* bo, const float* wg, const float* bg, const float* dscore,
                                         int B, int N, int D, int P, float* workspace, float* dSlast, int ldg,
                                         float* dWo, float* dbo, float* dwg, float* dbg, lnz_stream_t stream) {
  LNZ_REQUIRE(Slast && Wo && bo && wg && bg && dscore && workspace && dSlast && dWo && dbo && dwg && dbg, LNZ_EINVAL,
              "lnz_ggnn_readout_backward: null pointer");
  LNZ_REQUIRE(B > 0 && N > 0, LNZ_EINVAL, "lnz_ggnn_readout_backward: B = %d, N = %d must be positive", B, N);
  LNZ_REQUIRE(N <= GMAXN && D >= 32 && D <= GMAXD && D % 32 == 0 && P >= 1 && P <= GMAXP, LNZ_ENOTSUP,
              "lnz_ggnn_readout_backward: N = %d, D = %d, P = %d outside 1 <= N <= 32, D a multiple of 32 and <= 128, "
              "1 <= P <= 16", N, D, P);
  LNZ_REQUIRE(ld >= D && ldg >= D, LNZ_EINVAL, "lnz_ggnn_readout_backward: ld = %d, ldg = %d below the width %d", ld,
              ldg, D);
  LNZ_REQUIRE(!overlap(dSlast, span((uint64_t)B * N, ldg, D), Slast, span((uint64_t)B * N, ld, D)), LNZ_EINVAL,
              "lnz_ggnn_readout_backward: dSlast must not alias Slast");
  hipLaunchKernelGGL(ggnn_readout_backward_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, Slast, ld,
                     mask, Wo, bo, wg, bg, dscore, N, D, P, workspace, dSlast, ldg);
  const int rc = lnz::check_launch("lnz_ggnn_readout_backward");
  if (rc != LNZ_OK) return rc;
  const int M = P * D + P + D + 1;
  Segments seg = {{dWo, dbo, dwg, dbg, nullptr}, {P * D, P, D, 1, 0}};
  return sum_partials(workspace, B, M, seg, (hipStream_t)stream, "lnz_ggnn_readout_backward (sum of the partials)");
}
