// The backward of the GAT baseline's two kernels (csrc/gat.hip; reference model/gat.py:153-175 and
// :177-196 under loss.backward()).
//
// lnz_gat_attention_backward — per (molecule b, channel c, head h), block k = c H + h of Dh columns, with
// P the attention block recomputed from Wh by the forward's own instructions (column maximum subtracted,
// softmax over the ROW index i per column j, the same summation orders: the same bits):
//     dO[i]    = dOut[i] * (elu ? (out[i] > 0 ? 1 : out[i] + 1) : 1)            elu'(v) = exp(v) = out + 1, v <= 0
//     dP[i][j] = dO[i] . Wh[j]
//     t[j]     = sum_i P[i][j] dP[i][j]
//     dE[i][j] = P[i][j] (dP[i][j] - t[j])
//     dZ[i][j] = dE[i][j] * (s1[i] + s2[j] > 0 ? 1 : 0.2)
//     ds1[i]   = sum_j dZ[i][j] ;  ds2[j] = sum_i dZ[i][j]
//     dWh[j]   = sum_i P[i][j] dO[i] + ds1[j] a1 + ds2[j] a2
//     da1 = sum_i ds1[i] Wh[i], da2 = sum_i ds2[i] Wh[i], db1 = sum_i ds1[i], db2 = sum_i ds2[i], dbias = sum_i dO[i]
// All N padded rows and columns take part, as in the forward; L gets no gradient.
//
// The forward's decomposition: one workgroup of four waves per (molecule, channel), wave w takes the heads
// w, w + 4, ...; the channel's slice of L staged once; per wave a slice for Wh, one for dO, the N x N block
// (P, then dZ in place) and four vectors (s1, s2, ds1, ds2).  LDS: 4,224 B + 4 x (4,608 + 4,608 + 4,224 + 512)
// = 60,032 B, below the 64 KiB that need no grant.  A lane owns a column j and 16 of its rows: dP, t, dE, dZ
// and ds2 stay in registers, the row sums ds1 go through the block in LDS.
//
// The sums over the molecules (da1, db1, da2, db2, dbias) use no atomics and no workgroup waits on another:
// every workgroup writes its row of partials [da1 | da2 | dbias | db1 | db2] to the workspace, and a second
// launch adds the B rows per output in a fixed order (four contiguous quarters of the molecules, each
// ascending, then ((q0 + q1) + q2) + q3).  Every sum inside a block runs in a fixed order too (d, i or j
// ascending; the two 16-row halves of a column low + high): the gradients are a fixed function of the inputs.
//
// lnz_gat_readout_backward — one workgroup per molecule; x, o = Wo x + bo and g = sigmoid(wg x + bg)
// recomputed as the forward computes them; per row i in the mask (cnt of them; all N without a mask):
//     dy = dscore / cnt ; do = dy g ; dzg = (sum_p dy[p] o[p]) g (1 - g) ; dx = Wo^T do + wg dzg
//     dHlast[i, every block] = dx / CH                                            exactly 0 outside the mask
// and the molecule's partials [dWo | dbo | dwg | dbg] for the same fixed-order reduction.
#include "common.hpp"
#include "gat_tile.hpp"
#include "partial_sum.hpp"

namespace {

__global__ __launch_bounds__(64 * GW) void gat_attention_backward_kernel(
    const float* __restrict__ Wh, int ldw, const float* __restrict__ L, int64_t stride_b, int64_t stride_r,
    int64_t stride_c, int64_t stride_ch, const float* __restrict__ a1, const float* __restrict__ b1,
    const float* __restrict__ a2, const float* __restrict__ b2, const float* __restrict__ out, int ldo,
    const float* __restrict__ dOut, int ldd, int N, int C, int H, int Dh, int elu, float* __restrict__ ws,
    float* __restrict__ dWh, int ldg) {
  __shared__ float Ls[GN * LS];
  __shared__ __attribute__((aligned(16))) float Whs[GW][GN * WS];
  __shared__ __attribute__((aligned(16))) float Dos[GW][GN * WS];
  __shared__ float Ps[GW][GN * LS];
  __shared__ float Ss[GW][4 * GN];   // s1, s2, ds1, ds2

  const int c = blockIdx.x % C;
  const int64_t b = blockIdx.x / C;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int dq = Dh >> 2;   // float4 per row of a head block
  const int CH = C * H;
  float* part = ws + b * ((int64_t)CH * (3 * Dh + 2));   // [da1 | da2 | dbias : CH Dh each][db1 | db2 : CH each]

  const float* Lb = L + b * stride_b + c * stride_ch;
  for (int idx = threadIdx.x; idx < N * N; idx += 64 * GW) {
    const int i = idx / N, j = idx - i * N;
    Ls[i * LS + j] = Lb[i * stride_r + j * stride_c];
  }

  float* whs = Whs[wave];
  float* dos = Dos[wave];
  float* ps = Ps[wave];
  float* ss = Ss[wave];
  const int rounds = (H + GW - 1) / GW;   // uniform over the workgroup: every wave meets every barrier
  for (int r = 0; r < rounds; ++r) {
    const int h = r * GW + wave;
    const bool live = h < H;
    const int blk = c * H + h;
    // -- the head's N x Dh blocks of Wh and of dO = dOut * elu'
    if (live) {
      const float* src = Wh + (b * N) * (int64_t)ldw + (int64_t)blk * Dh;
      const float* gsrc = dOut + (b * N) * (int64_t)ldd + (int64_t)blk * Dh;
      for (int t = lane; t < N * dq; t += 64) {
        const int i = t / dq, q = t - i * dq;
        *reinterpret_cast<f32x4*>(whs + i * WS + 4 * q) =
            *reinterpret_cast<const f32x4*>(src + (int64_t)i * ldw + 4 * q);
        f32x4 g = *reinterpret_cast<const f32x4*>(gsrc + (int64_t)i * ldd + 4 * q);
        if (elu) {
          const f32x4 o = *reinterpret_cast<const f32x4*>(out + (b * N + i) * (int64_t)ldo + (int64_t)blk * Dh + 4 * q);
#pragma unroll
          for (int k = 0; k < 4; ++k) g[k] = o[k] > 0.0f ? g[k] : g[k] * (o[k] + 1.0f);
        }
        *reinterpret_cast<f32x4*>(dos + i * WS + 4 * q) = g;
      }
    }
    __syncthreads();   // (also: Ls is complete before its first reader)
    // -- s1 (lanes 0..31) and s2 (lanes 32..63) as the forward: one row per lane, d ascending
    if (live) {
      const int which = lane >> 5, i = lane & 31;
      if (i < N) {
        const float* a = (which ? a2 : a1) + (int64_t)blk * Dh;
        float acc = 0.0f;
        for (int d = 0; d < Dh; ++d) acc = fmaf(whs[i * WS + d], a[d], acc);
        ss[which * GN + i] = acc + (which ? b2 : b1)[blk];
      }
    }
    __syncthreads();
    // -- column j: lane = (half, j), half 0 takes rows 0..15, half 1 rows 16..31.  P as the forward, then dP, t,
    //    dE, dZ and ds2 in registers
    float dz[16];
    {
      const int half = lane >> 5, j = lane & 31;
      const bool col = live && j < N;
      const float s2j = col ? ss[GN + j] : 0.0f;
      float e[16];
      float m = -INFINITY;
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int i = 16 * half + u;
        if (col && i < N) {
          const float z = ss[i] + s2j;
          e[u] = (z > 0.0f ? z : 0.2f * z) + Ls[i * LS + j];
          m = fmaxf(m, e[u]);
        } else {
          e[u] = -INFINITY;
        }
      }
      m = fmaxf(m, __shfl_xor(m, 32));
      float s = 0.0f;
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int i = 16 * half + u;
        if (col && i < N) {
          e[u] = expf(e[u] - m);
          s += e[u];
        }
      }
      const float other = __shfl_xor(s, 32);
      const float tot = half ? other + s : s + other;   // rows 0..15 + rows 16..31 in both halves
      f32x4 wj[GD / 4];
#pragma unroll
      for (int q = 0; q < GD / 4; ++q) {
        if (col && q < dq) wj[q] = *reinterpret_cast<const f32x4*>(whs + j * WS + 4 * q);
        else wj[q] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      }
      float dp[16];
      float tp = 0.0f;
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int i = 16 * half + u;
        dp[u] = 0.0f;
        if (col && i < N) {
          const float p = e[u] / tot;
          ps[i * LS + j] = p;
          e[u] = p;
          float acc = 0.0f;   // dO[i] . Wh[j], d ascending
#pragma unroll
          for (int q = 0; q < GD / 4; ++q) {
            if (q < dq) {
              const f32x4 g = *reinterpret_cast<const f32x4*>(dos + i * WS + 4 * q);
#pragma unroll
              for (int k = 0; k < 4; ++k) acc = fmaf(g[k], wj[q][k], acc);
            }
          }
          dp[u] = acc;
          tp = fmaf(p, acc, tp);
        }
      }
      const float tother = __shfl_xor(tp, 32);
      const float tj = half ? tother + tp : tp + tother;
      float d2 = 0.0f;
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int i = 16 * half + u;
        dz[u] = 0.0f;
        if (col && i < N) {
          const float de = e[u] * (dp[u] - tj);
          dz[u] = ss[i] + s2j > 0.0f ? de : 0.2f * de;
          d2 += dz[u];
        }
      }
      const float dother = __shfl_xor(d2, 32);
      if (col && half == 0) ss[3 * GN + j] = d2 + dother;
    }
    __syncthreads();
    // -- sum_i P[i][j] dO[i]: four columns of one row j of dWh per task, i ascending; kept in registers
    f32x4 acc[(GN * GD / 4) / 64];
#pragma unroll
    for (int it = 0; it < (GN * GD / 4) / 64; ++it) {
      acc[it] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      const int t = lane + 64 * it;
      if (live && t < N * dq) {
        const int j = t / dq, q = t - j * dq;
        for (int i = 0; i < N; ++i) {
          const float p = ps[i * LS + j];
          const f32x4 g = *reinterpret_cast<const f32x4*>(dos + i * WS + 4 * q);
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[it][k] = fmaf(p, g[k], acc[it][k]);
        }
      }
    }
    __syncthreads();   // P has been read: the block takes dZ
    {
      const int half = lane >> 5, j = lane & 31;
      if (live && j < N) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int i = 16 * half + u;
          if (i < N) ps[i * LS + j] = dz[u];
        }
      }
    }
    __syncthreads();
    // -- ds1[i] = sum_j dZ[i][j], j ascending
    if (live && lane < N) {
      float s = 0.0f;
      for (int j = 0; j < N; ++j) s += ps[lane * LS + j];
      ss[2 * GN + lane] = s;
    }
    __syncthreads();
    if (live) {
      // -- dWh[j] = (sum_i P[i][j] dO[i]) + ds1[j] a1 + ds2[j] a2
      float* dst = dWh + (b * N) * (int64_t)ldg + (int64_t)blk * Dh;
#pragma unroll
      for (int it = 0; it < (GN * GD / 4) / 64; ++it) {
        const int t = lane + 64 * it;
        if (t < N * dq) {
          const int j = t / dq, q = t - j * dq;
          const float d1 = ss[2 * GN + j], d2 = ss[3 * GN + j];
          const float* p1 = a1 + (int64_t)blk * Dh + 4 * q;
          const float* p2 = a2 + (int64_t)blk * Dh + 4 * q;
          f32x4 v = acc[it];
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = fmaf(d2, p2[k], fmaf(d1, p1[k], v[k]));
          *reinterpret_cast<f32x4*>(dst + (int64_t)j * ldg + 4 * q) = v;
        }
      }
      // -- the molecule's partials of this block, i ascending: lanes 0..31 da1 and dbias, lanes 32..63 da2;
      //    lane 32 + Dh.. : nothing; db1 / db2 by lanes 0 and 32
      const int which = lane >> 5, d = lane & 31;
      const int64_t CHD = (int64_t)CH * Dh;
      float sd = 0.0f, sw = 0.0f, sb = 0.0f;
      for (int i = 0; i < N; ++i) {
        const float v = ss[(2 + which) * GN + i];
        sd += v;
        if (d < Dh) {
          sw = fmaf(v, whs[i * WS + d], sw);
          sb += dos[i * WS + d];
        }
      }
      if (d < Dh) {
        part[which * CHD + (int64_t)blk * Dh + d] = sw;
        if (which == 0) part[2 * CHD + (int64_t)blk * Dh + d] = sb;
      }
      if (d == 0) part[3 * CHD + which * CH + blk] = sd;
    }
    __syncthreads();   // the wave's LDS slices are free for the next head
  }
}

__global__ __launch_bounds__(256) void gat_readout_backward_kernel(
    const float* __restrict__ Hlast, int ld, const unsigned char* __restrict__ mask,
    const float* __restrict__ Wo, const float* __restrict__ bo, const float* __restrict__ wg,
    const float* __restrict__ bg, const float* __restrict__ dscore, int N, int CH, int Dh, int P,
    float* __restrict__ ws, float* __restrict__ dHlast, int ldg) {
  __shared__ float xs[GN * (GD + 1)];
  __shared__ float ys[GN * (RP + 1)];
  __shared__ float dxs[GN * (GD + 1)];
  __shared__ float gs[GN];    // the gate of a masked row, 0 outside the mask
  __shared__ float zs[GN];    // dzg of a masked row, 0 outside the mask
  __shared__ int ins[GN];     // row in the mask
  __shared__ float dys[RP];   // dscore / cnt
  const int64_t b = blockIdx.x;
  const float* Hb = Hlast + (b * N) * (int64_t)ld;
  // x, o and g as the forward computes them
  for (int t = threadIdx.x; t < N * Dh; t += 256) {
    const int i = t / Dh, d = t - i * Dh;
    const float* p = Hb + (int64_t)i * ld + d;
    float s = 0.0f;
    for (int k = 0; k < CH; ++k) s += p[(int64_t)k * Dh];
    xs[i * (GD + 1) + d] = s / (float)CH;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < N * (P + 1); t += 256) {
    const int i = t / (P + 1), p = t - i * (P + 1);
    const float* w = p < P ? Wo + (int64_t)p * Dh : wg;
    float acc = 0.0f;
    for (int d = 0; d < Dh; ++d) acc = fmaf(xs[i * (GD + 1) + d], w[d], acc);
    acc += p < P ? bo[p] : bg[0];
    ys[i * (RP + 1) + p] = p < P ? acc : 1.0f / (1.0f + expf(-acc));
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
    const float g = ys[i * (RP + 1) + P];
    float s = 0.0f;
    for (int p = 0; p < P; ++p) s = fmaf(dys[p], ys[i * (RP + 1) + p], s);
    ins[i] = in ? 1 : 0;
    gs[i] = in ? g : 0.0f;
    zs[i] = in ? s * (g * (1.0f - g)) : 0.0f;
  }
  __syncthreads();
  // dx = Wo^T do + wg dzg, p ascending; / CH for every block of the row
  for (int t = threadIdx.x; t < N * Dh; t += 256) {
    const int i = t / Dh, d = t - i * Dh;
    float acc = 0.0f;
    if (ins[i]) {
      for (int p = 0; p < P; ++p) acc = fmaf(Wo[(int64_t)p * Dh + d], dys[p] * gs[i], acc);
      acc = fmaf(wg[d], zs[i], acc) / (float)CH;
    }
    dxs[i * (GD + 1) + d] = acc;
  }
  __syncthreads();
  {
    const int width = CH * Dh;
    float* Gb = dHlast + (b * N) * (int64_t)ldg;
    for (int t = threadIdx.x; t < N * width; t += 256) {
      const int i = t / width, col = t - i * width;
      Gb[(int64_t)i * ldg + col] = dxs[i * (GD + 1) + col % Dh];
    }
  }
  // the molecule's partials [dWo P Dh | dbo P | dwg Dh | dbg 1], i ascending (rows outside the mask add 0)
  const int M = P * Dh + P + Dh + 1;
  float* part = ws + b * (int64_t)M;
  for (int t = threadIdx.x; t < M; t += 256) {
    float acc = 0.0f;
    if (t < P * Dh) {
      const int p = t / Dh, d = t - p * Dh;
      for (int i = 0; i < N; ++i) acc = fmaf(dys[p] * gs[i], xs[i * (GD + 1) + d], acc);
    } else if (t < P * Dh + P) {
      const int p = t - P * Dh;
      for (int i = 0; i < N; ++i) acc += dys[p] * gs[i];
    } else if (t < P * Dh + P + Dh) {
      const int d = t - P * Dh - P;
      for (int i = 0; i < N; ++i) acc = fmaf(zs[i], xs[i * (GD + 1) + d], acc);
    } else {
      for (int i = 0; i < N; ++i) acc += zs[i];
    }
    part[t] = acc;
  }
}

}  // namespace

extern "C" int64_t lnz_gat_attention_backward_workspace_floats(int B, int C, int H, int Dh) {
  if (B <= 0 || C <= 0 || H <= 0 || Dh <= 0) return 0;
  return (int64_t)B * C * H * (3 * (int64_t)Dh + 2);
}

extern "C" int lnz_gat_attention_backward(const float* Wh, int ldw, const float* L, int64_t stride_b,
                                          int64_t stride_r, int64_t stride_c, int64_t stride_ch, const float* a1,
                                          const float* b1, const float* a2, const float* b2, const float* out,
                                          int ldo, const float* dOut, int ldd, int B, int N, int C, int H, int Dh,
                                          int elu, float* workspace, float* dWh, int ldg, float* da1, float* db1,
                                          float* da2, float* db2, float* dbias, lnz_stream_t stream) {
  LNZ_REQUIRE(Wh && L && a1 && b1 && a2 && b2 && dOut && workspace && dWh && da1 && db1 && da2 && db2 && dbias,
              LNZ_EINVAL, "lnz_gat_attention_backward: null pointer");
  LNZ_REQUIRE(out || !elu, LNZ_EINVAL, "lnz_gat_attention_backward: elu = 1 needs the layer's output");
  LNZ_REQUIRE(B > 0 && N > 0 && C > 0 && H > 0 && Dh > 0, LNZ_EINVAL,
              "lnz_gat_attention_backward: B = %d, N = %d, C = %d, H = %d, Dh = %d must be positive", B, N, C, H,
              Dh);
  LNZ_REQUIRE(N <= GN && C <= 8 && H <= 16 && Dh <= GD && Dh % 4 == 0, LNZ_ENOTSUP,
              "lnz_gat_attention_backward: N = %d, C = %d, H = %d, Dh = %d outside N <= 32, C <= 8, H <= 16, "
              "Dh a multiple of 4 and <= 32", N, C, H, Dh);
  if (!elu) ldo = ldw;   // not read
  LNZ_REQUIRE(ldw % 4 == 0 && ldo % 4 == 0 && ldd % 4 == 0 && ldg % 4 == 0, LNZ_ENOTSUP,
              "lnz_gat_attention_backward: ldw = %d, ldo = %d, ldd = %d, ldg = %d must be multiples of 4", ldw,
              ldo, ldd, ldg);
  const int width = C * H * Dh;
  LNZ_REQUIRE(ldw >= width && ldo >= width && ldd >= width && ldg >= width, LNZ_EINVAL,
              "lnz_gat_attention_backward: ldw = %d, ldo = %d, ldd = %d, ldg = %d below the width %d", ldw, ldo,
              ldd, ldg, width);
  LNZ_REQUIRE(stride_b >= 0 && stride_r >= 0 && stride_c >= 0 && stride_ch >= 0, LNZ_EINVAL,
              "lnz_gat_attention_backward: negative stride of L");
  LNZ_REQUIRE(aligned16(Wh) && aligned16(dOut) && aligned16(dWh) && (!elu || aligned16(out)), LNZ_EINVAL,
              "lnz_gat_attention_backward: Wh, out, dOut and dWh must be 16-byte aligned");
  LNZ_REQUIRE((int64_t)B * C <= 0x7fffffffLL, LNZ_ENOTSUP, "lnz_gat_attention_backward: B * C = %lld workgroups",
              (long long)B * C);
  {
    const uint64_t rows = (uint64_t)B * N;
    LNZ_REQUIRE(!overlap(dWh, Wh, rows, ldg, ldw, width) && !overlap(dWh, dOut, rows, ldg, ldd, width) &&
                    (!elu || !overlap(dWh, out, rows, ldg, ldo, width)),
                LNZ_EINVAL, "lnz_gat_attention_backward: dWh must not alias Wh, out or dOut");
  }
  hipLaunchKernelGGL(gat_attention_backward_kernel, dim3((unsigned)(B * C)), dim3(64 * GW), 0, (hipStream_t)stream,
                     Wh, ldw, L, stride_b, stride_r, stride_c, stride_ch, a1, b1, a2, b2, elu ? out : nullptr, ldo,
                     dOut, ldd, N, C, H, Dh, elu, workspace, dWh, ldg);
  const int rc = lnz::check_launch("lnz_gat_attention_backward");
  if (rc != LNZ_OK) return rc;
  const int CH = C * H;
  const int64_t M = (int64_t)CH * (3 * Dh + 2);
  Segments seg = {{da1, da2, dbias, db1, db2}, {CH * Dh, CH * Dh, CH * Dh, CH, CH}};
  return sum_partials(workspace, B, M, seg, (hipStream_t)stream, "lnz_gat_attention_backward (sum of the partials)");
}

extern "C" int64_t lnz_gat_readout_backward_workspace_floats(int B, int Dh, int P) {
  if (B <= 0 || Dh <= 0 || P <= 0) return 0;
  return (int64_t)B * ((int64_t)P * Dh + P + Dh + 1);
}

extern "C" int lnz_gat_readout_backward(const float* Hlast, int ld, const uint8_t* mask, const float* Wo,
                                        const float* bo, const float* wg, const float* bg, const float* dscore,
                                        int B, int N, int CH, int Dh, int P, float* workspace, float* dHlast,
                                        int ldg, float* dWo, float* dbo, float* dwg, float* dbg,
                                        lnz_stream_t stream) {
  LNZ_REQUIRE(Hlast && Wo && bo && wg && bg && dscore && workspace && dHlast && dWo && dbo && dwg && dbg,
              LNZ_EINVAL, "lnz_gat_readout_backward: null pointer");
  LNZ_REQUIRE(B > 0 && N > 0 && CH > 0 && Dh > 0 && P > 0, LNZ_EINVAL,
              "lnz_gat_readout_backward: B = %d, N = %d, CH = %d, Dh = %d, P = %d must be positive", B, N, CH, Dh,
              P);
  LNZ_REQUIRE(N <= GN && Dh <= GD && P <= RP, LNZ_ENOTSUP,
              "lnz_gat_readout_backward: N = %d, Dh = %d, P = %d outside N <= 32, Dh <= 32, P <= 16", N, Dh, P);
  LNZ_REQUIRE((int64_t)ld >= (int64_t)CH * Dh && (int64_t)ldg >= (int64_t)CH * Dh, LNZ_EINVAL,
              "lnz_gat_readout_backward: ld = %d, ldg = %d below CH * Dh = %lld", ld, ldg, (long long)CH * Dh);
  LNZ_REQUIRE((int64_t)CH * Dh * N <= 0x7fffffffLL, LNZ_ENOTSUP, "lnz_gat_readout_backward: CH = %d blocks", CH);
  LNZ_REQUIRE(!overlap(dHlast, Hlast, (uint64_t)B * N, ldg, ld, CH * Dh), LNZ_EINVAL,
              "lnz_gat_readout_backward: dHlast must not alias Hlast");
  hipLaunchKernelGGL(gat_readout_backward_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, Hlast, ld, mask, Wo,
                     bo, wg, bg, dscore, N, CH, Dh, P, workspace, dHlast, ldg);
  const int rc = lnz::check_launch("lnz_gat_readout_backward");
  if (rc != LNZ_OK) return rc;
  const int M = P * Dh + P + Dh + 1;
  Segments seg = {{dWo, dbo, dwg, dbg, nullptr}, {P * Dh, P, Dh, 1, 0}};
  return sum_partials(workspace, B, M, seg, (hipStream_t)stream, "lnz_gat_readout_backward (sum of the partials)");
}
