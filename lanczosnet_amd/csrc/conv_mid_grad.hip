// Training for graphs of 33..128 nodes (config/graph_lanczos_net.yaml under runner/graph_runner.py:
// loss.backward() through model/lanczos_net_general.py:157-194, model/lanczos_net.py:157-194): the
// backward of csrc/conv_mid.hip, exact fp32 on v_mfma_f32_16x16x4_f32, three launches.
//
// The forward leaves every layer's output state X_{l+1} = relu(out_l) in its exchange buffer
// (Xwork [num_layer, B, NR, 128]); these are the stored activations.  With dOut_l = dX_{l+1} masked
// by [X_{l+1} > 0]:
//   dX_l  = sum_s V diag(g_s) V^T dOut_l W_s + sum_c L_c^T dOut_l W_c
//   dW_s  = sum_b (V^T dOut_l)^T diag(g_s) (V^T X_l),  dW_c = sum_b dOut_l^T (L_c X_l),  db_l = column sums
//   dG[l][b][k][s] = sum_o (V^T dOut_l)[k][o] ((V^T X_l) W_s^T)[k][o]
//
//   1. midgraph_head_grad_kernel   one workgroup per graph: the readout head's backward on the stored
//      last state -> dOut of the last layer, per-graph partials of the head's parameter gradients.
//   2. midgraph_input_grad_kernel  dOut of EVERY layer in one launch.  It is the forward kernel run on
//      the gradient: the same four workgroups per graph by output columns, the same exchange (placement
//      read from HW_REG_XCC_ID, write-through stores + sc1 loads on one L2, agent-scope release /
//      acquire otherwise, bounded spins, launches sized to the resident workgroups in whole groups
//      of eight graphs — see conv_mid.hip), with the weight blocks transposed ([128 in][S + C][128
//      out], the layer-0 block zero-padded to 128 rows), the Laplacian fragments transposed (the
//      operators are NOT assumed symmetric), the gains unchanged and "mask by the stored state"
//      as the epilogue.  The dOut buffer is the exchange buffer.
//   3. midgraph_project_kernel     one workgroup per (graph, layer): A = V^T dOut_l and Y = V^T X_l,
//      the operands of the weight-gradient GEMMs — Q = [g_s . Y]_s over the B K eigen rows for the long
//      scales (5x fewer rows than the node rows at the reference's sizes), M_c = L_c X_l over the node
//      rows for the edge types —, the gain gradients dG from A and Y, and the per-graph column sums
//      of dOut_l.  dW_l is then one library GEMM per operand (the caller's).
// Every sum runs in a fixed order; there are no float atomics.  Rows at or beyond a graph's node count
// come out of launch 2 exactly zero without being masked: the rows of L^T and V there are zero.
#include "common.hpp"
#include "conv_tiles.hpp"
#include "conv_mid.hpp"

namespace {

// ------------------------------------------------------------------------------------------ 1. head
struct HeadGradArgs {
  const float* Xlast;   // [B, NR, 128] the stored last state (slot num_layer - 1 of Xwork)
  const uint8_t* mask;  // [B, N]
  const float* gscore;  // [B, P]
  const float* Whead;   // [P + 1, 128]: head rows, then the gate row
  const float* bhead;   // [P + 1]
  float* dOut;          // [B, NR, 128]
  float* dWpart;        // [B, P + 1, 128]
  float* dbpart;        // [B, P + 1]
  int N, NR, P;
};

constexpr int ZP = 33;  // row pitch of the head's [N][P + 1] block
constexpr int head_lds_floats(int NR) { return NR * XP + 32 * 128 + 128 * ZP; }

__global__ __launch_bounds__(256) void midgraph_head_grad_kernel(HeadGradArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int N = a.N, NR = a.NR, P = a.P, no = P + 1;
  float* Xs = lds;              // [NR][XP]
  float* Wh = Xs + NR * XP;     // [no][128]
  float* Z = Wh + 32 * 128;     // [N][ZP]: y / gate pre-activations, then their gradients
  const float* X = a.Xlast + (int64_t)b * NR * 128;
  for (int idx = tid; idx < NR * 32; idx += 256) {
    const int row = idx >> 5, c4 = idx & 31;
    *reinterpret_cast<f32x4*>(&Xs[row * XP + 4 * c4]) = *reinterpret_cast<const f32x4*>(X + row * 128 + 4 * c4);
  }
  for (int idx = tid; idx < no * 32; idx += 256)
    *reinterpret_cast<f32x4*>(&Wh[4 * idx]) = *reinterpret_cast<const f32x4*>(a.Whead + 4 * idx);
  const int live = tid < N && a.mask[(int64_t)b * N + tid] ? 1 : 0;
  const float den = (float)__syncthreads_count(live);   // (also: Xs and Wh are complete)
  // z = W_h x + b_h, the same dot products as the forward's head
  for (int idx = tid; idx < N * no; idx += 256) {
    const int row = idx / no, o = idx - row * no;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll 8
    for (int k = 0; k < 128; k += 4) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(&Xs[row * XP + k]);
      const f32x4 ww = *reinterpret_cast<const f32x4*>(&Wh[o * 128 + k]);
      s0 = fmaf(x[0], ww[0], s0), s1 = fmaf(x[1], ww[1], s1);
      s2 = fmaf(x[2], ww[2], s2), s3 = fmaf(x[3], ww[3], s3);
    }
    Z[row * ZP + o] = (s0 + s1) + (s2 + s3) + a.bhead[o];
  }
  __syncthreads();
  // score_o = sum_rows y_o sigmoid(z_gate) / den over the masked rows
  if (tid < N) {
    float* z = Z + tid * ZP;
    if (live) {
      const float sg = 1.0f / (1.0f + expf(-z[P]));
      float acc = 0.0f;
      for (int o = 0; o < P; ++o) {
        const float dy = a.gscore[(int64_t)b * P + o] / den;
        acc = fmaf(dy, z[o], acc);
        z[o] = dy * sg;
      }
      z[P] = acc * sg * (1.0f - sg);
    } else {
      for (int o = 0; o < no; ++o) z[o] = 0.0f;
    }
  }
  __syncthreads();
  // dOut = (dZ W_h) masked by the stored state; rows at or beyond N (zero in the stored state) are zero
  {
    const int col = tid & 127;
    float* out = a.dOut + (int64_t)b * NR * 128;
    for (int row = tid >> 7; row < NR; row += 2) {
      float acc = 0.0f;
      if (row < N)
        for (int o = 0; o < no; ++o) acc = fmaf(Z[row * ZP + o], Wh[o * 128 + col], acc);
      out[row * 128 + col] = (row < N && Xs[row * XP + col] > 0.0f) ? acc : 0.0f;
    }
  }
  // per-graph partials of dW_h = dZ^T X and db_h = column sums of dZ, rows in order
  for (int idx = tid; idx < no * 128; idx += 256) {
    const int o = idx >> 7, col = idx & 127;
    float acc = 0.0f;
    for (int row = 0; row < N; ++row) acc = fmaf(Z[row * ZP + o], Xs[row * XP + col], acc);
    a.dWpart[((int64_t)b * no + o) * 128 + col] = acc;
  }
  if (tid < no) {
    float acc = 0.0f;
    for (int row = 0; row < N; ++row) acc += Z[row * ZP + tid];
    a.dbpart[(int64_t)b * no + tid] = acc;
  }
}

// ------------------------------------------------------------------------------------ 2. input grad
struct MidGradArgs {
  float* D;             // [num_layer, B, NR, 128]: slot num_layer - 1 holds the last layer's dOut on entry;
                        // the launch writes the others (the exchange buffer)
  const float* Xwork;   // [num_layer, B, NR, 128] the forward's stored states
  const float* L;       // [B, N, N, C] by element strides
  int64_t sb, sr, sc, sch;
  const float* V;       // [B, N, K]
  const float* G;       // [num_layer, B, S, K]
  const float* Wt;      // per layer [128 in][S + C][128 out]
  int32_t* sync;        // [B * (num_layer + 1)] zero-initialised, this launch's own
  float* dX0;           // [B, NR, din0] or NULL
  int32_t* folded;      // [B] or NULL: 1 where the graph's operator channels are equal
  int B, N, K, C, S, num_layer, din0, R;
  int b0, b1;
  int force_fenced;
};

constexpr int mid_grad_lds_floats(int R) {
  return 16 * R * XP + 32 * TP + 32 * XP + 2 * 32 * TP + 32 * AP + 16 * 32;
}

// Layer l's transposed weights and gains into registers, as the forward's fetch_layer (every layer
// is 128 wide here)
template <int C>
__device__ __forceinline__ void fetch_grad_layer(const MidGradArgs& a, const int l, const int b, const int q,
                                                 const int tid, const int wave, const int j, const int kq,
                                                 f32x4 (&bw)[2][8], f32x4 (&we)[C][2], float& gnext) {
  const int S = a.S, K = a.K, nch = a.S + C;
  const float* Wp = a.Wt + (int64_t)l * 128 * nch * 128;
  gnext = 0.0f;
  if (tid < S * 32) {
    const int sidx = tid >> 5, k = tid & 31;
    gnext = k < K ? a.G[(((int64_t)l * a.B + b) * S + sidx) * K + k] : 0.0f;
  }
  const int s0 = wave < S ? wave : 0;
  const float* w0 = Wp + ((int64_t)(32 * q + j) * nch + s0) * 128 + 4 * kq;
  const float* w1 = w0 + (int64_t)16 * nch * 128;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    bw[0][t] = *reinterpret_cast<const f32x4*>(w0 + 16 * t);
    bw[1][t] = *reinterpret_cast<const f32x4*>(w1 + 16 * t);
  }
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int idx = tid + 512 * h, n = idx >> 5, k4 = idx & 31;
      we[c][h] = *reinterpret_cast<const f32x4*>(Wp + ((int64_t)(32 * q + n) * nch + S + c) * 128 + 4 * k4);
    }
}

template <int C>
__global__ __launch_bounds__(512) void midgraph_input_grad_kernel(MidGradArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, kq = lane >> 4;
  // block numbering as the forward: the four column quarters of a graph are 8 blocks apart
  const int idx32 = blockIdx.x & 31;
  const int b = a.b0 + 8 * (blockIdx.x >> 5) + (idx32 & 7), q = idx32 >> 3;
  if (b >= a.b1) return;
  __shared__ int one_l2;
  const int Lnum = a.num_layer;
  int32_t* place = a.sync + (int64_t)a.B * Lnum + b;
  if (tid == 0) {
    const int xcc = (int)__builtin_amdgcn_s_getreg((4 - 1) << 11 | 0 << 6 | 20) & 15;   // HW_REG_XCC_ID
    __hip_atomic_fetch_add(place, 1 | ((xcc + 1) << (8 + 4 * q)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  const int N = a.N, K = a.K, S = a.S, R = a.R, NR = 16 * R, B = a.B;
  float* Xs = lds;                    // [NR][XP]       dOut of the current layer
  float* Vt = Xs + NR * XP;           // [32 slots][TP]
  float* Ys = Vt + 32 * TP;           // [32 slots][XP]
  float* Tt = Ys + 32 * XP;           // [32 columns][TP]
  float* Ws = Tt + 32 * TP;           // [32 columns][TP]
  float* Ps = Tt;                     // [8 waves][32 slots][PP] (Tt + Ws)
  float* Pacc = Ws + 32 * TP;         // [32 slots][AP]
  float* gs = Pacc + 32 * AP;         // [S <= 16][32]

  for (int idx = tid; idx < 32 * NR; idx += 512) {
    const int k = idx / NR, node = idx - k * NR;
    Vt[k * TP + node] = (k < K && node < N) ? finite_or_zero(a.V[((int64_t)b * N + node) * K + k]) : 0.0f;
  }
  float vf[2][4];     // V[16 wave + j][16 t + 4 kq + u]
  float Lf[C][8][4];  // L_c^T[16 wave + j][16 t + 4 kq + u] = L_c[16 t + 4 kq + u][16 wave + j]
  {
    const int node = 16 * wave + j;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = 16 * t + 4 * kq + u;
        vf[t][u] = (wave < R && node < N && k < K) ? finite_or_zero(a.V[((int64_t)b * N + node) * K + k]) : 0.0f;
      }
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int col = 16 * t + 4 * kq + u;
          Lf[c][t][u] = (wave < R && node < N && col < N)
                            ? a.L[(int64_t)b * a.sb + (int64_t)col * a.sr + (int64_t)node * a.sc + (int64_t)c * a.sch]
                            : 0.0f;
        }
  }
  // equal operator channels: one edge pass with the summed weight blocks, as the forward
  bool fold = false;
  if (C > 1) {
    int same = 1;
#pragma unroll
    for (int c = 1; c < C; ++c)
#pragma unroll
      for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) same &= Lf[c][t][u] == Lf[0][t][u] ? 1 : 0;
    fold = __syncthreads_and(same) != 0;
  }
  if (a.folded && q == 0 && tid == 0) a.folded[b] = fold ? 1 : 0;
  // the last layer's dOut (the head's launch wrote it)
  {
    const float* d = a.D + ((int64_t)(Lnum - 1) * B + b) * NR * 128;
    for (int idx = tid; idx < NR * 32; idx += 512) {
      const int row = idx >> 5, c4 = idx & 31;
      *reinterpret_cast<f32x4*>(&Xs[row * XP + 4 * c4]) = *reinterpret_cast<const f32x4*>(d + row * 128 + 4 * c4);
    }
  }
  const int nch = S + C;
  f32x4 bw[2][8];
  f32x4 we[C][2];
  float gnext;
  fetch_grad_layer<C>(a, Lnum - 1, b, q, tid, wave, j, kq, bw, we, gnext);
  for (int l = Lnum - 1; l >= 0; --l) {
    const float* Wl = a.Wt + (int64_t)l * 128 * nch * 128;
    if (tid < S * 32) gs[tid] = gnext;
    __syncthreads();
    // ---- 1. Y = V^T dOut
    {
      f32x4 y0 = zero4(), y1 = zero4();
      for (int t = 0; t < R; ++t) {
        float xa[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) xa[u] = Xs[(16 * t + 4 * kq + u) * XP + 16 * wave + j];
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(&Vt[j * TP + 16 * t + 4 * kq]);
        const f32x4 b1 = *reinterpret_cast<const f32x4*>(&Vt[(16 + j) * TP + 16 * t + 4 * kq]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          y0 = mfma16(xa[u], b0[u], y0);
          y1 = mfma16(xa[u], b1[u], y1);
        }
      }
      *reinterpret_cast<f32x4*>(&Ys[j * XP + 16 * wave + 4 * kq]) = y0;
      *reinterpret_cast<f32x4*>(&Ys[(16 + j) * XP + 16 * wave + 4 * kq]) = y1;
    }
    __syncthreads();
    // ---- 2. long scales: P = sum_s (g_s . Y) W_s, wave w = scales w, w + 8
    {
      f32x4 p[2][2] = {{zero4(), zero4()}, {zero4(), zero4()}};
      for (int s = wave; s < S; s += 8) {
        const float g0 = gs[s * 32 + j], g1 = gs[s * 32 + 16 + j];
        if (s >= 8) {
          const float* w0 = Wl + ((int64_t)(32 * q + j) * nch + s) * 128 + 4 * kq;
          const float* w1 = w0 + (int64_t)16 * nch * 128;
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            bw[0][t] = *reinterpret_cast<const f32x4*>(w0 + 16 * t);
            bw[1][t] = *reinterpret_cast<const f32x4*>(w1 + 16 * t);
          }
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          f32x4 a0 = *reinterpret_cast<const f32x4*>(&Ys[j * XP + 16 * t + 4 * kq]);
          f32x4 a1 = *reinterpret_cast<const f32x4*>(&Ys[(16 + j) * XP + 16 * t + 4 * kq]);
          const f32x4 b0 = bw[0][t], b1 = bw[1][t];
          a0 *= g0;
          a1 *= g1;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            p[0][0] = mfma16(a0[u], b0[u], p[0][0]);
            p[0][1] = mfma16(a0[u], b1[u], p[0][1]);
            p[1][0] = mfma16(a1[u], b0[u], p[1][0]);
            p[1][1] = mfma16(a1[u], b1[u], p[1][1]);
          }
        }
      }
      float* pw = Ps + wave * 32 * PP;
#pragma unroll
      for (int st = 0; st < 2; ++st)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) pw[(16 * st + 4 * kq + r) * PP + 16 * ct + j] = p[st][ct][r];
    }
    __syncthreads();
    for (int idx = tid; idx < 1024; idx += 512) {
      const int k = idx >> 5, col = idx & 31;
      float acc = 0.0f;
#pragma unroll
      for (int w = 0; w < 8; ++w) acc += Ps[(w * 32 + k) * PP + col];
      Pacc[k * AP + col] = acc;
    }
    __syncthreads();
    // ---- 3. edge types: T = dOut W_c, out += L_c^T T
    f32x4 o0 = zero4(), o1 = zero4();
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (fold && c > 0) continue;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int idx = tid + 512 * h, n = idx >> 5, k4 = idx & 31;
        f32x4 v = we[c][h];
        if (fold) {
#pragma unroll
          for (int c2 = 1; c2 < C; ++c2) v += we[c2][h];
        }
        *reinterpret_cast<f32x4*>(&Ws[n * TP + 4 * k4]) = v;
      }
      __syncthreads();
      if (wave < R) {
        f32x4 t0 = zero4(), t1 = zero4();
#pragma unroll 1
        for (int t = 0; t < 8; ++t) {
          const f32x4 xa = *reinterpret_cast<const f32x4*>(&Xs[(16 * wave + j) * XP + 16 * t + 4 * kq]);
          const f32x4 b0 = *reinterpret_cast<const f32x4*>(&Ws[j * TP + 16 * t + 4 * kq]);
          const f32x4 b1 = *reinterpret_cast<const f32x4*>(&Ws[(16 + j) * TP + 16 * t + 4 * kq]);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            t0 = mfma16(xa[u], b0[u], t0);
            t1 = mfma16(xa[u], b1[u], t1);
          }
        }
        *reinterpret_cast<f32x4*>(&Tt[j * TP + 16 * wave + 4 * kq]) = t0;
        *reinterpret_cast<f32x4*>(&Tt[(16 + j) * TP + 16 * wave + 4 * kq]) = t1;
      }
      __syncthreads();
      if (wave < R) {
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          if (t < R) {
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(&Tt[j * TP + 16 * t + 4 * kq]);
            const f32x4 b1 = *reinterpret_cast<const f32x4*>(&Tt[(16 + j) * TP + 16 * t + 4 * kq]);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              o0 = mfma16(Lf[c][t][u], b0[u], o0);
              o1 = mfma16(Lf[c][t][u], b1[u], o1);
            }
          }
        }
      }
    }
    // the ReLU mask of this layer's result: the stored state X_l, this wave's rows and the
    // workgroup's columns (issued here, behind the
    // last use of the staged weight registers; used in the epilogue)
    float m0[4] = {0.f, 0.f, 0.f, 0.f}, m1[4] = {0.f, 0.f, 0.f, 0.f};
    if (l > 0 && wave < R) {
      const float* xm = a.Xwork + ((int64_t)(l - 1) * B + b) * NR * 128 + 32 * q;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * wave + 4 * kq + r;
        m0[r] = xm[row * 128 + j];
        m1[r] = xm[row * 128 + 16 + j];
      }
    }
    // ---- 4. lift out += V P
    if (wave < R) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float b0[4], b1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          b0[u] = Pacc[(16 * t + 4 * kq + u) * AP + j];
          b1[u] = Pacc[(16 * t + 4 * kq + u) * AP + 16 + j];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          o0 = mfma16(vf[t][u], b0[u], o0);
          o1 = mfma16(vf[t][u], b1[u], o1);
        }
      }
    }
    if (l == 0) {
      // dX_0 (the embedding model's): this workgroup's columns below the input width.  Nothing waits
      // for it: no exchange.
      if (a.dX0 && wave < R) {
        float* dx = a.dX0 + (int64_t)b * NR * a.din0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * wave + 4 * kq + r;
          if (32 * q + j < a.din0) dx[row * a.din0 + 32 * q + j] = o0[r];
          if (32 * q + 16 + j < a.din0) dx[row * a.din0 + 32 * q + 16 + j] = o1[r];
        }
      }
      return;
    }
    __syncthreads();  // every wave is through with Tt
    // ---- 5. dOut_{l-1} = dX_l where the stored X_l is positive, staged as the [NR, 32] column slice.
    //      No row mask: the rows of L^T and V at or beyond the node count are zero, and so is o.
    float* Os = Tt;   // [NR][AP]
    if (wave < R) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * wave + 4 * kq + r;
        Os[row * AP + j] = m0[r] > 0.0f ? o0[r] : 0.0f;
        Os[row * AP + 16 + j] = m1[r] > 0.0f ? o1[r] : 0.0f;
      }
    }
    __syncthreads();
    // ---- 6. exchange, exactly as the forward's (conv_mid.hip): write-through stores, counter, sc1 loads
    {
      float* xo = a.D + ((int64_t)(l - 1) * B + b) * NR * 128 + 32 * q;
      for (int idx = tid; idx < NR * 16; idx += 512) {
        const int row = idx >> 4, w2 = idx & 15;
        const unsigned long long v = *reinterpret_cast<const unsigned long long*>(&Os[row * AP + 2 * w2]);
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(xo + row * 128 + 2 * w2), v, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (l == Lnum - 1 && tid == 0) {
      const int pw = spin_until_four(place);
      const int mine = (pw >> (8 + 4 * q)) & 15;
      one_l2 = ((pw >> 8) & 15) == mine && ((pw >> 12) & 15) == mine && ((pw >> 16) & 15) == mine &&
               ((pw >> 20) & 15) == mine && !a.force_fenced;
    }
    __syncthreads();
    fetch_grad_layer<C>(a, l - 1, b, q, tid, wave, j, kq, bw, we, gnext);
    const bool fenced = !one_l2;   // (workgroup-uniform)
    if (tid == 0) {
      if (fenced) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      __hip_atomic_fetch_add(&a.sync[b * Lnum + l], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      (void)spin_until_four(&a.sync[b * Lnum + l]);
    }
    __syncthreads();
    if (fenced) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    {
      const float* xi = a.D + ((int64_t)(l - 1) * B + b) * NR * 128;
      for (int idx = tid; idx < NR * 48; idx += 512) {
        const int row = idx / 48, w3 = idx - row * 48;
        const int qq = w3 >> 4, qsrc = qq + (qq >= q ? 1 : 0), w2 = 16 * qsrc + (w3 & 15);
        const unsigned long long v = __hip_atomic_load(
            reinterpret_cast<const unsigned long long*>(xi + row * 128 + 2 * w2), __ATOMIC_RELAXED,
            __HIP_MEMORY_SCOPE_AGENT);
        *reinterpret_cast<unsigned long long*>(&Xs[row * XP + 2 * w2]) = v;
      }
      for (int idx = tid; idx < NR * 16; idx += 512) {
        const int row = idx >> 4, w2 = idx & 15;
        *reinterpret_cast<unsigned long long*>(&Xs[row * XP + 32 * q + 2 * w2]) =
            *reinterpret_cast<const unsigned long long*>(&Os[row * AP + 2 * w2]);
      }
    }
  }
}

// --------------------------------------------------------------------------------------- 3. project
struct ProjectArgs {
  const float* D;       // [num_layer, B, NR, 128] dOut
  const float* Xwork;   // [num_layer, B, NR, 128]
  const float* X0;      // [B, N, din0]
  const float* L;
  int64_t sb, sr, sc, sch;
  const float* V;       // [B, N, K]
  const float* G;       // [num_layer, B, S, K]
  const float* W;       // the forward's weights: per layer [128][S + C][din_l]
  float* A;             // [num_layer, B, K, 128]      V^T dOut_l
  float* Q;             // [num_layer, B, K, S, 128]   g_s . (V^T X_l)
  float* M;             // [num_layer, B, NR, C, 128]  L_c X_l
  float* dG;            // [num_layer, B, K, S] or NULL
  float* dbpart;        // [num_layer, B, 128]         column sums of dOut_l
  int B, N, K, C, S, num_layer, din0, R;
};

constexpr int project_lds_floats(int R) { return 32 * TP + 16 * R * XP + 2 * 32 * XP + 16 * 32; }

// Zs^T-free product V^T Z for all 128 columns: wave w = columns [16 w, 16 w + 16), both slot tiles
__device__ __forceinline__ void project_onto_v(const float* Zs, const float* Vt, float* out, const int R,
                                               const int wave, const int j, const int kq) {
  f32x4 y0 = zero4(), y1 = zero4();
  for (int t = 0; t < R; ++t) {
    float xa[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) xa[u] = Zs[(16 * t + 4 * kq + u) * XP + 16 * wave + j];
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(&Vt[j * TP + 16 * t + 4 * kq]);
    const f32x4 b1 = *reinterpret_cast<const f32x4*>(&Vt[(16 + j) * TP + 16 * t + 4 * kq]);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      y0 = mfma16(xa[u], b0[u], y0);
      y1 = mfma16(xa[u], b1[u], y1);
    }
  }
  *reinterpret_cast<f32x4*>(&out[j * XP + 16 * wave + 4 * kq]) = y0;
  *reinterpret_cast<f32x4*>(&out[(16 + j) * XP + 16 * wave + 4 * kq]) = y1;
}

__global__ __launch_bounds__(512) void midgraph_project_kernel(ProjectArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, kq = lane >> 4;
  const int b = blockIdx.x, l = blockIdx.y;
  const int N = a.N, K = a.K, S = a.S, C = a.C, R = a.R, NR = 16 * R, B = a.B, nch = S + C;
  const int din = l ? 128 : a.din0, nk = din >> 4;
  float* Vt = lds;                 // [32 slots][TP]
  float* Zs = Vt + 32 * TP;        // [NR][XP]: dOut_l, then X_l
  float* As = Zs + NR * XP;        // [32 slots][XP]
  float* Ys = As + 32 * XP;        // [32 slots][XP]
  float* gs = Ys + 32 * XP;        // [S <= 16][32]
  const int64_t lb = (int64_t)l * B + b;
  for (int idx = tid; idx < 32 * NR; idx += 512) {
    const int k = idx / NR, node = idx - k * NR;
    Vt[k * TP + node] = (k < K && node < N) ? finite_or_zero(a.V[((int64_t)b * N + node) * K + k]) : 0.0f;
  }
  if (tid < S * 32) {
    const int sidx = tid >> 5, k = tid & 31;
    gs[tid] = k < K ? a.G[(lb * S + sidx) * K + k] : 0.0f;
  }
  {
    const float* d = a.D + lb * NR * 128;
    for (int idx = tid; idx < NR * 32; idx += 512) {
      const int row = idx >> 5, c4 = idx & 31;
      *reinterpret_cast<f32x4*>(&Zs[row * XP + 4 * c4]) = *reinterpret_cast<const f32x4*>(d + row * 128 + 4 * c4);
    }
  }
  __syncthreads();
  // ---- A = V^T dOut_l; db partial = column sums of dOut_l, rows in order
  project_onto_v(Zs, Vt, As, R, wave, j, kq);
  if (tid < 128) {
    float acc = 0.0f;
    for (int row = 0; row < N; ++row) acc += Zs[row * XP + tid];
    a.dbpart[lb * 128 + tid] = acc;
  }
  __syncthreads();
  if (S > 0)
    for (int idx = tid; idx < K * 32; idx += 512) {
      const int k = idx >> 5, c4 = idx & 31;
      *reinterpret_cast<f32x4*>(a.A + (lb * K + k) * 128 + 4 * c4) = *reinterpret_cast<const f32x4*>(&As[k * XP + 4 * c4]);
    }
  // ---- X_l (the input state for layer 0, else the stored state of layer l - 1), zero beyond its width
  if (l == 0) {
    const int d4 = din >> 2;
    for (int idx = tid; idx < NR * 32; idx += 512) {
      const int row = idx >> 5, c4 = idx & 31;
      f32x4 v = zero4();
      if (row < N && c4 < d4) v = *reinterpret_cast<const f32x4*>(a.X0 + ((int64_t)b * N + row) * din + 4 * c4);
      *reinterpret_cast<f32x4*>(&Zs[row * XP + 4 * c4]) = v;
    }
  } else {
    const float* x = a.Xwork + ((int64_t)(l - 1) * B + b) * NR * 128;
    for (int idx = tid; idx < NR * 32; idx += 512) {
      const int row = idx >> 5, c4 = idx & 31;
      *reinterpret_cast<f32x4*>(&Zs[row * XP + 4 * c4]) = *reinterpret_cast<const f32x4*>(x + row * 128 + 4 * c4);
    }
  }
  __syncthreads();
  // ---- Y = V^T X_l
  project_onto_v(Zs, Vt, Ys, R, wave, j, kq);
  // ---- M_c = L_c X_l over the node rows: wave w = rows [16 w, 16 w + 16), all 128 columns
  if (wave < R) {
    const int node = 16 * wave + j;
    for (int c = 0; c < C; ++c) {
      f32x4 acc[8];
#pragma unroll
      for (int ct = 0; ct < 8; ++ct) acc[ct] = zero4();
      for (int t = 0; t < R; ++t) {
        float lf[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int col = 16 * t + 4 * kq + u;
          lf[u] = (node < N && col < N)
                      ? a.L[(int64_t)b * a.sb + (int64_t)node * a.sr + (int64_t)col * a.sc + (int64_t)c * a.sch]
                      : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float* xr = &Zs[(16 * t + 4 * kq + u) * XP + j];
#pragma unroll
          for (int ct = 0; ct < 8; ++ct) acc[ct] = mfma16(lf[u], xr[16 * ct], acc[ct]);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float* m = a.M + ((lb * NR + 16 * wave + 4 * kq + r) * C + c) * 128 + j;
#pragma unroll
        for (int ct = 0; ct < 8; ++ct) m[16 * ct] = acc[ct][r];
      }
    }
  }
  __syncthreads();
  if (S == 0) return;
  // ---- Q[k][s][:] = g_s[k] Y[k][:]
  for (int idx = tid; idx < K * S * 32; idx += 512) {
    const int c4 = idx & 31, ks = idx >> 5, k = ks / S, s = ks - k * S;
    f32x4 v = *reinterpret_cast<const f32x4*>(&Ys[k * XP + 4 * c4]);
    v *= gs[s * 32 + k];
    *reinterpret_cast<f32x4*>(a.Q + ((lb * K + k) * S + s) * 128 + 4 * c4) = v;
  }
  if (!a.dG) return;
  // ---- dG[k][s] = sum_o A[k][o] (Y W_s^T)[k][o]: wave w = scales w, w + 8; the W_s fragments
  //      straight from global memory
  const float* Wl = a.W + (l ? (int64_t)128 * nch * a.din0 + (int64_t)(l - 1) * 128 * nch * 128 : 0);
  for (int s = wave; s < S; s += 8) {
    f32x4 acc[2][8];
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int ct = 0; ct < 8; ++ct) acc[st][ct] = zero4();
    for (int t = 0; t < nk; ++t) {
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(&Ys[j * XP + 16 * t + 4 * kq]);
      const f32x4 a1 = *reinterpret_cast<const f32x4*>(&Ys[(16 + j) * XP + 16 * t + 4 * kq]);
#pragma unroll
      for (int ct = 0; ct < 8; ++ct) {
        const f32x4 bf = *reinterpret_cast<const f32x4*>(Wl + ((int64_t)(16 * ct + j) * nch + s) * din + 16 * t + 4 * kq);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          acc[0][ct] = mfma16(a0[u], bf[u], acc[0][ct]);
          acc[1][ct] = mfma16(a1[u], bf[u], acc[1][ct]);
        }
      }
    }
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int slot = 16 * st + 4 * kq + r;
        float v = 0.0f;
#pragma unroll
        for (int ct = 0; ct < 8; ++ct) v = fmaf(acc[st][ct][r], As[slot * XP + 16 * ct + j], v);
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if (j == 0 && slot < K) a.dG[(lb * K + slot) * S + s] = v;
      }
  }
}

}  // namespace

extern "C" int64_t lnz_midgraph_head_grad_workspace_floats(int B, int dout) {
  if (B <= 0 || dout < 1) return 0;
  return (int64_t)B * (dout + 1) * 129;
}

extern "C" int lnz_midgraph_head_grad(const float* X_last, const uint8_t* mask, const float* grad_score,
                                      const float* Whead, const float* bhead, int B, int N, int dout,
                                      float* dOut_last, float* workspace, lnz_stream_t stream) {
  LNZ_REQUIRE(X_last && mask && grad_score && Whead && bhead && dOut_last && workspace && B > 0, LNZ_EINVAL,
              "lnz_midgraph_head_grad: null pointer or B=%d", B);
  LNZ_REQUIRE(N > 0 && N <= 128 && dout >= 1 && dout <= 31, LNZ_ENOTSUP,
              "lnz_midgraph_head_grad: built for N <= 128, head width <= 31 (N=%d dout=%d)", N, dout);
  HeadGradArgs a;
  a.Xlast = X_last, a.mask = mask, a.gscore = grad_score, a.Whead = Whead, a.bhead = bhead;
  a.dOut = dOut_last, a.dWpart = workspace, a.dbpart = workspace + (int64_t)B * (dout + 1) * 128;
  a.N = N, a.NR = 16 * ((N + 15) / 16), a.P = dout;
  const size_t bytes = (size_t)head_lds_floats(a.NR) * sizeof(float);
  LNZ_DYNAMIC_LDS(midgraph_head_grad_kernel, bytes, "lnz_midgraph_head_grad");
  midgraph_head_grad_kernel<<<dim3(B), dim3(256), bytes, (hipStream_t)stream>>>(a);
  return lnz::check_launch("lnz_midgraph_head_grad");
}

extern "C" int lnz_midgraph_input_grad(float* dOut, const float* Xwork, const float* L, int64_t stride_b,
                                       int64_t stride_r, int64_t stride_c, int64_t stride_ch, const float* V,
                                       const float* G, const float* Wt, int B, int N, int K, int C, int S,
                                       int num_layer, int din0, int32_t* sync, float* dX0, int32_t* folded,
                                       lnz_stream_t stream) {
  LNZ_REQUIRE(dOut && Xwork && L && V && Wt && sync && B > 0, LNZ_EINVAL,
              "lnz_midgraph_input_grad: null pointer or B=%d", B);
  LNZ_REQUIRE(N > 0 && N <= 128 && K > 0 && K <= 32 && S >= 0 && S <= 16 && (S == 0 || G) && num_layer > 0,
              LNZ_ENOTSUP, "lnz_midgraph_input_grad: built for N <= 128, K <= 32, <= 16 long scales "
              "(N=%d K=%d S=%d)", N, K, S);
  LNZ_REQUIRE(C >= 1 && C <= 2, LNZ_ENOTSUP, "lnz_midgraph_input_grad: built for 1..2 operator channels (C=%d)", C);
  LNZ_REQUIRE(din0 > 0 && din0 % 16 == 0 && din0 <= 128, LNZ_ENOTSUP,
              "lnz_midgraph_input_grad: input width %d must be a multiple of 16, <= 128 (zero-pad)", din0);
  MidGradArgs a;
  a.D = dOut, a.Xwork = Xwork, a.L = L, a.sb = stride_b, a.sr = stride_r, a.sc = stride_c, a.sch = stride_ch;
  a.V = V, a.G = G, a.Wt = Wt, a.sync = sync, a.dX0 = dX0, a.folded = folded;
  a.B = B, a.N = N, a.K = K, a.C = C, a.S = S, a.num_layer = num_layer, a.din0 = din0;
  a.R = (N + 15) / 16;
  const size_t bytes = (size_t)mid_grad_lds_floats(a.R) * sizeof(float);
  const void* fn = C == 1 ? (const void*)midgraph_input_grad_kernel<1> : (const void*)midgraph_input_grad_kernel<2>;
  LNZ_DYNAMIC_LDS(fn, bytes, "lnz_midgraph_input_grad");
  // the four workgroups of a graph wait for each other: launches of what the device holds at once,
  // whole groups of 32 blocks = 8 graphs, as lnz_midgraph_forward
  int dev = 0, n_cu = 0, per_cu = 0;
  LNZ_REQUIRE(hipGetDevice(&dev) == hipSuccess &&
                  hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
                  hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 512, bytes) == hipSuccess,
              LNZ_ELAUNCH, "lnz_midgraph_input_grad: occupancy query failed");
  const int groups = (int)(((int64_t)n_cu * per_cu) / 32);
  LNZ_REQUIRE(groups >= 1, LNZ_ENOTSUP,
              "lnz_midgraph_input_grad: the device holds %d x %d workgroups at once, 32 (eight graphs) are needed",
              n_cu, per_cu);
  const char* ff = getenv("LNZ_MID_FENCED");
  a.force_fenced = ff && ff[0] == '1';
  lnz::note_kernel("midgraph_input_grad_kernel<%d>", C);
  for (int b0 = 0; b0 < B; b0 += 8 * groups) {
    a.b0 = b0;
    a.b1 = b0 + 8 * groups < B ? b0 + 8 * groups : B;
    const int grid = ((a.b1 - a.b0 + 7) / 8) * 32;
    void* params[] = {&a};
    (void)hipLaunchKernel(fn, dim3(grid), dim3(512), params, bytes, (hipStream_t)stream);
    const int rc = lnz::check_launch("lnz_midgraph_input_grad");
    if (rc != LNZ_OK) return rc;
  }
  return LNZ_OK;
}

extern "C" int64_t lnz_midgraph_project_workspace_floats(int B, int N, int K, int C, int S, int num_layer) {
  if (B <= 0 || N <= 0 || K <= 0 || C <= 0 || S < 0 || num_layer <= 0) return 0;
  const int64_t NR = 16 * ((N + 15) / 16);
  // A | Q | M | dG | db partials
  return (int64_t)num_layer * B * ((int64_t)K * 128 + (int64_t)K * S * 128 + NR * C * 128 + (int64_t)K * S + 128);
}

extern "C" int lnz_midgraph_project(const float* dOut, const float* Xwork, const float* X0, const float* L,
                                    int64_t stride_b, int64_t stride_r, int64_t stride_c, int64_t stride_ch,
                                    const float* V, const float* G, const float* W, int B, int N, int K, int C,
                                    int S, int num_layer, int din0, int want_dgains, float* workspace,
                                    lnz_stream_t stream) {
  LNZ_REQUIRE(dOut && Xwork && X0 && L && V && W && workspace && B > 0, LNZ_EINVAL,
              "lnz_midgraph_project: null pointer or B=%d", B);
  LNZ_REQUIRE(N > 0 && N <= 128 && K > 0 && K <= 32 && S >= 0 && S <= 16 && (S == 0 || G) && num_layer > 0 &&
                  num_layer <= 65535 && C >= 1 && C <= 2,
              LNZ_ENOTSUP, "lnz_midgraph_project: built for N <= 128, K <= 32, <= 16 long scales, 1..2 operator "
              "channels (N=%d K=%d S=%d C=%d)", N, K, S, C);
  LNZ_REQUIRE(din0 > 0 && din0 % 16 == 0 && din0 <= 128, LNZ_ENOTSUP,
              "lnz_midgraph_project: input width %d must be a multiple of 16, <= 128 (zero-pad)", din0);
  ProjectArgs a;
  a.D = dOut, a.Xwork = Xwork, a.X0 = X0, a.L = L, a.sb = stride_b, a.sr = stride_r, a.sc = stride_c;
  a.sch = stride_ch, a.V = V, a.G = G, a.W = W;
  a.B = B, a.N = N, a.K = K, a.C = C, a.S = S, a.num_layer = num_layer, a.din0 = din0, a.R = (N + 15) / 16;
  const int64_t LB = (int64_t)num_layer * B, NR = 16 * a.R;
  a.A = workspace;
  a.Q = a.A + LB * K * 128;
  a.M = a.Q + LB * K * S * 128;
  float* dG = a.M + LB * NR * C * 128;
  a.dG = want_dgains && S > 0 ? dG : nullptr;
  a.dbpart = dG + LB * K * S;
  const size_t bytes = (size_t)project_lds_floats(a.R) * sizeof(float);
  LNZ_DYNAMIC_LDS(midgraph_project_kernel, bytes, "lnz_midgraph_project");
  midgraph_project_kernel<<<dim3(B, num_layer), dim3(512), bytes, (hipStream_t)stream>>>(a);
  return lnz::check_launch("lnz_midgraph_project");
}
