// The full symmetric eigendecomposition of get_graph_laplacian_eigs(..., use_eigen_decomp=True)
// (utils/data_helper.py:197-223: `np.linalg.eigh` of the n_b x n_b block, then the top-K |lambda|
// cut) for ragged batches of graphs of up to 2048 nodes.  All arithmetic is fp64, outputs fp32.
//
// Stages (one stream, ordered by launch boundaries; no grid-wide barriers, no atomics):
//   1. load        the lower triangle of A (UPLO='L', as numpy) -> fp64 workspace;  rows/columns
//                  >= n_b and the strict upper triangle are never read.
//   2. tridiag     dsytrd 'L' with a latrd-style panel of NB columns.  Per column: a one-workgroup
//                  launch per graph corrects the column by the panel's earlier reflectors, forms the
//                  Householder reflector and the panel dots; the symmetric matrix-vector product over
//                  the trailing lower triangle is split into 64 x 64 tiles, one workgroup each, which
//                  write partial row sums (a fixed slot per tile pair); the next column's launch
//                  sums them in a fixed order.  After the panel a rank-2 NB update of the trailing
//                  lower triangle (fp64 FMA, tiles of 64 x 64).
//   3. tridiagonal eigenpairs: split at negligible off-diagonals, Sturm-count bisection for the K
//                  smallest and K largest eigenvalues, the stable descending-|lambda| cut (one
//                  workgroup per graph); inverse iteration with partial-pivoting LU (dgttrf / dgttrs)
//                  and re-orthogonalisation (CGS2) inside clusters (dstein's 1e-3 ||T|| cluster gap),
//                  clusters spread over the workgroups of a graph.
//   4. back-transformation: Q Z with the panels' compact WY form I - Y T Y^T (T from the dots kept
//                  in stage 2, dlarft forward / columnwise), last panel first.
//   5. epilogue    sign rule (first largest-magnitude entry positive), fp32, zero padding.
// Every sum runs in a fixed order that depends on n_b only: results are bitwise repeatable and
// independent of the other graphs of the batch.
#include "common.hpp"
#include "tridiag_eig.hpp"

#include <float.h>

#include <algorithm>

namespace {

constexpr int NB = 32;          // panel width (reflectors per panel)
constexpr int TS = 64;          // tile edge of the trailing-matrix product and update
constexpr int COL_T = 512;      // threads of the per-column launch
constexpr int KC = 16;          // eigenvector columns per back-transformation workgroup
constexpr int MAX_N = 2048;
constexpr int MAX_K = 256;
constexpr int MAX_B = 65535;    // graphs per call: the batch is the launches' grid y

struct Layout {
  int64_t A, P, Vp, Wp, X, TD, d, e, tau, Z, lam, bad, sel, per_graph;
};

inline int64_t al256(int64_t x) { return (x + 255) / 256 * 256; }

Layout layout(int N, int K) {
  Layout L;
  const int nT = (N + TS - 1) / TS;
  int64_t at = 0;
  L.A = at;   at += al256((int64_t)N * N * 8);
  L.P = at;   at += al256((int64_t)nT * nT * TS * 8);
  L.Vp = at;  at += al256((int64_t)NB * N * 8);
  L.Wp = at;  at += al256((int64_t)NB * N * 8);
  L.X = at;   at += al256(2 * NB * 8);
  L.TD = at;  at += al256((int64_t)N * NB * 8);
  L.d = at;   at += al256((int64_t)N * 8);
  L.e = at;   at += al256((int64_t)N * 8);
  L.tau = at; at += al256((int64_t)N * 8);
  L.Z = at;   at += al256((int64_t)K * N * 8);
  L.lam = at; at += al256((int64_t)K * 8);
  L.bad = at; at += al256((int64_t)(N + 1) * 4);   // [N] non-finite rows, [N] = 1: input not finite
  L.sel = at; at += al256((int64_t)(K + 2) * 8 + (int64_t)(3 * K + 2) * 4);   // struct Sel
  L.per_graph = at;
  return L;
}

struct Ws {
  char* base;
  Layout L;
  int N;
  __device__ char* g(int b) const { return base + (int64_t)b * L.per_graph; }
  __device__ double* A(int b) const { return (double*)(g(b) + L.A); }
  __device__ double* P(int b) const { return (double*)(g(b) + L.P); }
  __device__ double* Vp(int b) const { return (double*)(g(b) + L.Vp); }
  __device__ double* Wp(int b) const { return (double*)(g(b) + L.Wp); }
  __device__ double* X(int b) const { return (double*)(g(b) + L.X); }
  __device__ double* TD(int b) const { return (double*)(g(b) + L.TD); }
  __device__ double* d(int b) const { return (double*)(g(b) + L.d); }
  __device__ double* e(int b) const { return (double*)(g(b) + L.e); }
  __device__ double* tau(int b) const { return (double*)(g(b) + L.tau); }
  __device__ double* Z(int b) const { return (double*)(g(b) + L.Z); }
  __device__ double* lam(int b) const { return (double*)(g(b) + L.lam); }
  __device__ int32_t* bad(int b) const { return (int32_t*)(g(b) + L.bad); }
  __device__ char* sel(int b) const { return g(b) + L.sel; }
};

__device__ inline int graph_n(const int32_t* n_nodes, int b, int N) {
  if (!n_nodes) return N;
  const int n = n_nodes[b];
  return n < 0 ? 0 : (n > N ? N : n);
}

using lnz_tri::block_max;
using lnz_tri::block_sum;
using lnz_tri::wave_sum_butterfly;

// ------------------------------------------------------------------------------------ 1. load
__global__ __launch_bounds__(256) void eigh_load_kernel(const float* __restrict__ A, int64_t sb,
                                                        int64_t sr, int64_t sc,
                                                        const int32_t* __restrict__ n_nodes, int N,
                                                        Ws ws) {
  __shared__ int bad_s;
  const int r = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const int n = graph_n(n_nodes, b, N);
  if (t == 0) bad_s = 0;
  __syncthreads();
  if (r < n) {
    const float* src = A + (int64_t)b * sb + (int64_t)r * sr;
    double* dst = ws.A(b) + (int64_t)r * N;
    int bad = 0;
    for (int c = t; c <= r; c += 256) {
      const float v = src[(int64_t)c * sc];
      bad |= !isfinite(v);
      dst[c] = (double)v;
    }
    if (bad) bad_s = 1;   // benign race: every writer stores 1
  }
  __syncthreads();
  if (t == 0) {
    ws.bad(b)[r] = (r < n) ? bad_s : 0;
    if (r == 0) ws.bad(b)[N] = 0;
  }
}

// -------------------------------------------------------------------- 2a. one column of the panel
// finish (column fj, panel slot fi): w = tau (A22 v - V (W^T v) - W (V^T v)), w += -tau/2 (w.v) v
// prep   (column pj, panel slot pi): correct column pj by the panel so far, form its reflector,
//        the dots V^T v, W^T v (kept for finish and, V^T v, for the block reflector's T).
__global__ __launch_bounds__(COL_T) void eigh_column_kernel(const int32_t* __restrict__ n_nodes, int N,
                                                            Ws ws, int fj, int fi, int pj, int pi) {
  __shared__ double col[MAX_N];
  __shared__ double red[COL_T];
  __shared__ double xs[2 * NB];
  const int b = blockIdx.x, t = threadIdx.x;
  const int n = graph_n(n_nodes, b, N);
  double* Aw = ws.A(b);
  double* Vp = ws.Vp(b);
  double* Wp = ws.Wp(b);
  double* X = ws.X(b);
  if (fj >= 0 && fj < n - 1) {
    const int j = fj, i = fi;
    const double tau = ws.tau(b)[j];
    if (t < 2 * NB) xs[t] = (t % NB) < i ? X[t] : 0.0;
    __syncthreads();
    const double* P = ws.P(b);
    const int nT = (N + TS - 1) / TS;
    const int t0 = (j + 1) / TS, nTb = (n + TS - 1) / TS;
    double part = 0.0;
    for (int r = j + 1 + t; r < n; r += COL_T) {
      const double* pr = P + ((int64_t)(r / TS) * nT) * TS + (r % TS);
      double y = 0.0;
      for (int ct = t0; ct < nTb; ++ct) y += pr[(int64_t)ct * TS];
      double corr = 0.0;
      for (int a = 0; a < i; ++a)
        corr += Vp[(int64_t)a * N + r] * xs[NB + a] + Wp[(int64_t)a * N + r] * xs[a];
      const double p = tau * (y - corr);
      col[r] = p;
      part += p * Vp[(int64_t)i * N + r];
    }
    const double dot = block_sum<COL_T>(part, red);
    const double alpha = -0.5 * tau * dot;
    for (int r = j + 1 + t; r < n; r += COL_T)
      Wp[(int64_t)i * N + r] = col[r] + alpha * Vp[(int64_t)i * N + r];
    __syncthreads();
  }
  if (pj < 0 || pj >= n) return;
  const int j = pj, i = pi;
  for (int r = j + t; r < n; r += COL_T) {
    double v = Aw[(int64_t)r * N + j];
    for (int a = 0; a < i; ++a)
      v -= Vp[(int64_t)a * N + r] * Wp[(int64_t)a * N + j] + Wp[(int64_t)a * N + r] * Vp[(int64_t)a * N + j];
    col[r] = v;
  }
  __syncthreads();
  if (j == n - 1) {
    if (t == 0) {
      ws.d(b)[j] = col[j];
      ws.tau(b)[j] = 0.0;
    }
    return;
  }
  double ss = 0.0;
  for (int r = j + 2 + t; r < n; r += COL_T) ss += col[r] * col[r];
  const double xnorm2 = block_sum<COL_T>(ss, red);
  const double alpha = col[j + 1];
  double tau = 0.0, beta = alpha, scal = 0.0;
  if (xnorm2 > 0.0) {
    beta = -copysign(sqrt(alpha * alpha + xnorm2), alpha);
    tau = (beta - alpha) / beta;
    scal = 1.0 / (alpha - beta);
  }
  if (t == 0) {
    ws.d(b)[j] = col[j];
    ws.e(b)[j] = beta;
    ws.tau(b)[j] = tau;
  }
  __syncthreads();   // col[j + 1] read by every thread above
  for (int r = j + 1 + t; r < n; r += COL_T) {
    const double v = r == j + 1 ? 1.0 : col[r] * scal;
    col[r] = v;
    Vp[(int64_t)i * N + r] = v;
    if (r >= j + 2) Aw[(int64_t)r * N + j] = v;   // the reflector, kept for the back-transformation
  }
  __syncthreads();
  // the 2 i dots, one wave each in turn
  const int wave = t >> 6, lane = t & 63;
  for (int q = wave; q < 2 * i; q += COL_T / 64) {
    const double* src = (q < i ? Vp : Wp) + (int64_t)(q % i) * N;
    double s = 0.0;
    for (int r = j + 1 + lane; r < n; r += 64) s += src[r] * col[r];
    s = wave_sum_butterfly(s);
    if (lane == 0) {
      X[(q < i ? 0 : NB) + q % i] = s;
      if (q < i) ws.TD(b)[(int64_t)j * NB + q] = s;
    }
  }
}

// tile index -> (row tile, column tile), row >= column, both >= t0
__device__ inline void tile_pair(int idx, int t0, int& rt, int& ct) {
  int r = (int)((sqrt(8.0 * idx + 1.0) - 1.0) * 0.5);
  while ((r + 1) * (r + 2) / 2 <= idx) ++r;
  while (r * (r + 1) / 2 > idx) --r;
  rt = t0 + r;
  ct = t0 + idx - r * (r + 1) / 2;
}

// ------------------------------------------------------- 2b. trailing product y = A22 v, by tiles
// Tile (rt, ct) of the trailing lower triangle (rows and columns in [j + 1, n)): P[rt][ct] = A_tile v_c
// and, off the diagonal, P[ct][rt] = A_tile^T v_r.  Every slot is written by exactly one tile.
__global__ __launch_bounds__(256) void eigh_symv_kernel(const int32_t* __restrict__ n_nodes, int N,
                                                        Ws ws, int j, int i) {
  __shared__ double S[TS][TS + 1];
  __shared__ double vr[TS], vc[TS];
  __shared__ double red[4][TS];
  const int b = blockIdx.y, t = threadIdx.x;
  const int n = graph_n(n_nodes, b, N);
  if (j >= n - 1) return;
  const int o = j + 1;
  int rt, ct;
  tile_pair(blockIdx.x, o / TS, rt, ct);
  if (rt * TS >= n) return;
  const double* Aw = ws.A(b);
  const double* v = ws.Vp(b) + (int64_t)i * N;
  const int r0 = rt * TS, c0 = ct * TS;
  const bool diag = rt == ct;
  for (int q = t; q < TS * TS; q += 256) {
    const int rr = q / TS, cc = q % TS;
    const int r = r0 + rr, c = c0 + cc;
    double a = 0.0;
    if (r >= o && r < n && c >= o && c < n && (!diag || c <= r)) a = Aw[(int64_t)r * N + c];
    S[rr][cc] = a;
  }
  if (t < TS) {
    const int r = r0 + t, c = c0 + t;
    vr[t] = (r >= o && r < n) ? v[r] : 0.0;
    vc[t] = (c >= o && c < n) ? v[c] : 0.0;
  }
  __syncthreads();
  if (diag) {
    for (int q = t; q < TS * TS; q += 256) {
      const int rr = q / TS, cc = q % TS;
      if (cc > rr) S[rr][cc] = S[cc][rr];
    }
    __syncthreads();
  }
  const int nT = (N + TS - 1) / TS;
  double* P = ws.P(b);
  {
    const int rr = t >> 2, qq = t & 3;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += S[rr][qq * 16 + k] * vc[qq * 16 + k];
    red[qq][rr] = s;
  }
  __syncthreads();
  if (t < TS)
    P[((int64_t)rt * nT + ct) * TS + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
  if (diag) return;
  __syncthreads();
  {
    const int cc = t >> 2, qq = t & 3;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += S[qq * 16 + k][cc] * vr[qq * 16 + k];
    red[qq][cc] = s;
  }
  __syncthreads();
  if (t < TS)
    P[((int64_t)ct * nT + rt) * TS + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

// ------------------------------------------- 2c. rank-2 jb update of the trailing lower triangle
// A[r][c] -= sum_a V[a][r] W[a][c] + W[a][r] V[a][c] for c <= r, r and c in [s, n), s = j0 + jb.
__global__ __launch_bounds__(256) void eigh_update_kernel(const int32_t* __restrict__ n_nodes, int N,
                                                          Ws ws, int s, int jb) {
  __shared__ double Vr[NB][TS], Wr[NB][TS];
  const int b = blockIdx.y, t = threadIdx.x;
  const int n = graph_n(n_nodes, b, N);
  if (s >= n) return;
  int rt, ct;
  tile_pair(blockIdx.x, s / TS, rt, ct);
  if (rt * TS >= n) return;
  const double* Vp = ws.Vp(b);
  const double* Wp = ws.Wp(b);
  const int r0 = rt * TS, c0 = ct * TS;
  for (int q = t; q < jb * TS; q += 256) {
    const int a = q / TS, rr = q % TS, r = r0 + rr;
    const bool in = r >= s && r < n;
    Vr[a][rr] = in ? Vp[(int64_t)a * N + r] : 0.0;
    Wr[a][rr] = in ? Wp[(int64_t)a * N + r] : 0.0;
  }
  __syncthreads();
  const int cc = t & 63, rg = t >> 6, c = c0 + cc;
  if (c < s || c >= n) return;
  double acc[16];
#pragma unroll
  for (int m = 0; m < 16; ++m) acc[m] = 0.0;
  for (int a = 0; a < jb; ++a) {
    const double vc = Vp[(int64_t)a * N + c], wc = Wp[(int64_t)a * N + c];
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const int rr = rg + 4 * m;
      acc[m] = fma(Vr[a][rr], wc, acc[m]);
      acc[m] = fma(Wr[a][rr], vc, acc[m]);
    }
  }
  double* Aw = ws.A(b);
#pragma unroll
  for (int m = 0; m < 16; ++m) {
    const int r = r0 + rg + 4 * m;
    if (r >= s && r < n && c <= r) Aw[(int64_t)r * N + c] -= acc[m];
  }
}

// ---------------------------------------------------------- 3. eigenpairs of the tridiagonal T
// (the arithmetic is csrc/tridiag_eig.hpp, shared with the wide K-step Lanczos path)
using lnz_tri::EIG_T;
using lnz_tri::MAX_CAND;
using lnz_tri::Sel;

__device__ inline Sel sel_of(const Ws& ws, int b, int K) { return lnz_tri::sel_at(ws.sel(b), K); }

// 3a. one workgroup per graph; dynamic LDS: d, e, e2 [N] doubles.  Splits T (the zeroed
// off-diagonals go back to the workspace), bisection for the K smallest and K largest eigenvalues,
// the stable descending-|lambda| cut, and the clusters of consecutive selected eigenvalues.
__global__ __launch_bounds__(EIG_T) void eigh_bisect_kernel(const int32_t* __restrict__ n_nodes, int N,
                                                             int K, Ws ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ double red[EIG_T];
  __shared__ double lamc[MAX_CAND];
  __shared__ int rankc[MAX_CAND];
  __shared__ int bad_s;
  double* d = (double*)smem;
  double* e = d + N;
  double* e2 = e + N;
  const int b = blockIdx.x, t = threadIdx.x;
  const int n = graph_n(n_nodes, b, N);
  int32_t* badw = ws.bad(b);
  const Sel sl = sel_of(ws, b, K);
  if (t == 0) bad_s = 0;
  __syncthreads();
  for (int r = t; r < n; r += EIG_T)
    if (badw[r]) bad_s = 1;
  __syncthreads();
  if (bad_s || n == 0) {
    if (t == 0) {
      badw[N] = bad_s;
      sl.ncl[0] = 0;
    }
    return;
  }
  lnz_tri::bisect_body(n, K, ws.d(b), ws.e(b), ws.lam(b), sl, d, e, e2, red, lamc, rankc);
  if (t == 0) badw[N] = 0;
}

// 3b. inverse iteration; workgroup x of graph b takes clusters x, x + gridDim.x, ... (the host
// spreads a small batch's clusters over the chip and keeps one workgroup per graph for a large
// one: the results do not depend on the split); dynamic LDS: d, e, dd, du, du2, dl,
// x [N] doubles, piv [N] bytes.  Inside a cluster the vectors are computed in ascending order, each
// re-orthogonalised (CGS2) against the cluster's earlier ones; clusters are independent.
__global__ __launch_bounds__(EIG_T) void eigh_invit_kernel(const int32_t* __restrict__ n_nodes, int N, int K,
                                                            Ws ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ double red[EIG_T];
  __shared__ int clus[MAX_K];
  __shared__ double hq[MAX_K];
  double* d = (double*)smem;
  double* e = d + N;
  double* dd = e + N;
  double* du = dd + N;
  double* du2 = du + N;
  double* dl = du2 + N;
  double* x = dl + N;
  unsigned char* piv = (unsigned char*)(x + N);
  const int b = blockIdx.y;
  const int n = graph_n(n_nodes, b, N);
  if (n == 0 || ws.bad(b)[N] == 1) return;
  lnz_tri::invit_body(n, N, ws.d(b), ws.e(b), sel_of(ws, b, K), ws.Z(b), (int)blockIdx.x, (int)gridDim.x, d, e,
                      dd, du, du2, dl, x, piv, red, clus, hq);
}

// --------------------------------------------------------------------- 4. back-transformation
// Z[:, k0:k0+KC] <- Q Z, Q = H_0 ... H_{n-2}; per panel (last first) Z -= Y (T (Y^T Z)).
__device__ inline double refl(const double* Aw, int N, int r, int j) {
  return r <= j ? 0.0 : (r == j + 1 ? 1.0 : Aw[(int64_t)r * N + j]);
}

__global__ __launch_bounds__(256) void eigh_backtransform_kernel(const int32_t* __restrict__ n_nodes,
                                                                 int N, int K, Ws ws) {
  __shared__ double Tm[NB][NB + 1];
  __shared__ double Wm[NB][KC];
  __shared__ double W2[NB][KC];
  __shared__ double part[8][NB][KC];
  const int b = blockIdx.y, t = threadIdx.x, k0 = blockIdx.x * KC;
  const int n = graph_n(n_nodes, b, N);
  const int kk = n < K ? n : K;
  if (k0 >= kk || n < 2 || ws.bad(b)[N] == 1) return;
  const int kc = kk - k0 < KC ? kk - k0 : KC;
  const double* Aw = ws.A(b);
  const double* tau = ws.tau(b);
  const double* TD = ws.TD(b);
  double* Z = ws.Z(b) + (int64_t)k0 * N;
  const int npan = (n - 2) / NB + 1;   // panels holding reflectors 0 .. n-2
  for (int p = npan - 1; p >= 0; --p) {
    const int j0 = p * NB;
    const int jb = (n - 1 - j0) < NB ? (n - 1 - j0) : NB;
    // T (upper triangular): T[a][a] = tau_a, T[0:a, a] = -tau_a T[0:a, 0:a] (Y^T y_a)
    for (int q = t; q < NB * NB; q += 256) Tm[q / NB][q % NB] = 0.0;
    __syncthreads();
    for (int a = 0; a < jb; ++a) {
      const double ta = tau[j0 + a];
      if (t < a) {
        double s = 0.0;
        for (int a2 = t; a2 < a; ++a2) s += Tm[t][a2] * TD[(int64_t)(j0 + a) * NB + a2];
        Tm[t][a] = -ta * s;
      }
      if (t == 0) Tm[a][a] = ta;
      __syncthreads();
    }
    // W = Y^T Z (rows j0+1 .. n-1), 8 row slices, reduced in order
    {
      const int a = t & 31, sl = t >> 5;
      double acc[KC];
#pragma unroll
      for (int c = 0; c < KC; ++c) acc[c] = 0.0;
      if (a < jb) {
        for (int r = j0 + 1 + sl; r < n; r += 8) {
          const double y = refl(Aw, N, r, j0 + a);
#pragma unroll
          for (int c = 0; c < KC; ++c)
            if (c < kc) acc[c] += y * Z[(int64_t)c * N + r];
        }
      }
#pragma unroll
      for (int c = 0; c < KC; ++c) part[sl][a][c] = acc[c];
    }
    __syncthreads();
    for (int q = t; q < NB * KC; q += 256) {
      const int a = q / KC, c = q % KC;
      double s = 0.0;
      for (int sl = 0; sl < 8; ++sl) s += part[sl][a][c];
      Wm[a][c] = s;
    }
    __syncthreads();
    for (int q = t; q < NB * KC; q += 256) {
      const int a = q / KC, c = q % KC;
      double s = 0.0;
      for (int a2 = a; a2 < jb; ++a2) s += Tm[a][a2] * Wm[a2][c];
      W2[a][c] = a < jb ? s : 0.0;
    }
    __syncthreads();
    for (int r = j0 + 1 + t; r < n; r += 256) {
      double acc[KC];
#pragma unroll
      for (int c = 0; c < KC; ++c) acc[c] = 0.0;
      for (int a = 0; a < jb; ++a) {
        const double y = refl(Aw, N, r, j0 + a);
#pragma unroll
        for (int c = 0; c < KC; ++c) acc[c] += y * W2[a][c];
      }
#pragma unroll
      for (int c = 0; c < KC; ++c)
        if (c < kc) Z[(int64_t)c * N + r] -= acc[c];
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------- 5. epilogue
__global__ __launch_bounds__(256) void eigh_epilogue_kernel(const int32_t* __restrict__ n_nodes, int N,
                                                            int K, Ws ws, float* __restrict__ D,
                                                            float* __restrict__ V, int32_t* __restrict__ info) {
  __shared__ double rv[256];
  __shared__ int ri[256];
  const int k = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const int n = graph_n(n_nodes, b, N);
  const int kk = n < K ? n : K;
  if (k == 0 && t == 0 && info) {
    // 1: the input block was not finite; 2: an inverse iteration did not converge
    int st = ws.bad(b)[N] == 1 ? 1 : 0;
    if (!st) {
      const Sel sl = sel_of(ws, b, K);
      for (int q = 0; q < sl.ncl[0]; ++q)
        if (sl.fail[q]) st = 2;
    }
    info[b] = st;
  }
  float* Vb = V + (int64_t)b * N * K + k;
  const bool ok = k < kk && ws.bad(b)[N] != 1;
  if (!ok) {
    for (int r = t; r < N; r += 256) Vb[(int64_t)r * K] = 0.0f;
    if (t == 0) D[(int64_t)b * K + k] = 0.0f;
    return;
  }
  const double* z = ws.Z(b) + (int64_t)k * N;
  double best = -1.0;
  int bi = 0x7fffffff;
  for (int r = t; r < n; r += 256) {
    const double a = fabs(z[r]);
    if (a > best) {
      best = a;
      bi = r;
    }
  }
  rv[t] = best;
  ri[t] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      const double o = rv[t + s];
      const int oi = ri[t + s];
      if (o > rv[t] || (o == rv[t] && oi < ri[t])) {
        rv[t] = o;
        ri[t] = oi;
      }
    }
    __syncthreads();
  }
  const double sg = (ri[0] < n && z[ri[0]] < 0.0) ? -1.0 : 1.0;
  for (int r = t; r < N; r += 256) Vb[(int64_t)r * K] = r < n ? (float)(sg * z[r]) : 0.0f;
  if (t == 0) D[(int64_t)b * K + k] = (float)ws.lam(b)[k];
}

inline int check(const char* who) { return lnz::check_launch(who); }

}  // namespace

extern "C" int64_t lnz_sym_eigh_topk_workspace_bytes(int B, int N, int K) {
  if (B <= 0 || N <= 0 || K <= 0 || N > MAX_N || K > MAX_K) return 0;
  return (int64_t)B * layout(N, K).per_graph;
}

extern "C" int lnz_sym_eigh_topk(const float* A, int64_t stride_b, int64_t stride_r, int64_t stride_c,
                                 const int32_t* n_nodes, int B, int N, int K, void* workspace,
                                 int64_t workspace_bytes, float* D, float* V, int32_t* info,
                                 lnz_stream_t stream) {
  const char* who = "lnz_sym_eigh_topk";
  LNZ_REQUIRE(N <= MAX_N, LNZ_ENOTSUP, "%s: N=%d: graphs of up to N <= %d nodes are served", who, N, MAX_N);
  LNZ_REQUIRE(K <= MAX_K, LNZ_ENOTSUP, "%s: K=%d: up to K <= %d eigenpairs are served", who, K, MAX_K);
  LNZ_REQUIRE(A && D && V && workspace && B > 0 && N > 0 && K > 0, LNZ_EINVAL,
              "%s: bad arguments (A, D, V, workspace non-null; B=%d, N=%d, K=%d >= 1)", who, B, N, K);
  LNZ_REQUIRE(stride_r > 0 && stride_c > 0 && stride_b >= 0, LNZ_EINVAL, "%s: bad strides", who);
  LNZ_REQUIRE(B <= MAX_B, LNZ_EINVAL, "%s: B=%d: at most %d graphs per call (the caller chunks)", who, B, MAX_B);
  const Layout L = layout(N, K);
  LNZ_REQUIRE(workspace_bytes >= (int64_t)B * L.per_graph, LNZ_EINVAL, "%s: workspace of %lld bytes, %lld needed",
              who, (long long)workspace_bytes, (long long)((int64_t)B * L.per_graph));
  LNZ_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, LNZ_EINVAL, "%s: workspace alignment (256 B)",
              who);
  const size_t bis_lds = (size_t)N * 8 * 3;
  const size_t inv_lds = (size_t)N * 8 * 7 + (size_t)N;
  LNZ_DYNAMIC_LDS(eigh_bisect_kernel, bis_lds, who);
  LNZ_DYNAMIC_LDS(eigh_invit_kernel, inv_lds, who);
  hipStream_t st = (hipStream_t)stream;
  const Ws ws{(char*)workspace, L, N};
  hipLaunchKernelGGL(eigh_load_kernel, dim3(N, B), dim3(256), 0, st, A, stride_b, stride_r, stride_c, n_nodes, N,
                     ws);
  int rc = check(who);
  if (rc != LNZ_OK) return rc;
  const int nT = (N + TS - 1) / TS;
  auto tiles = [&](int first) {
    const int m = nT - first / TS;
    return m * (m + 1) / 2;
  };
  for (int j0 = 0; j0 < N; j0 += NB) {
    const int jb = N - j0 < NB ? N - j0 : NB;
    hipLaunchKernelGGL(eigh_column_kernel, dim3(B), dim3(COL_T), 0, st, n_nodes, N, ws, -1, 0, j0, 0);
    for (int i = 0; i < jb; ++i) {
      const int j = j0 + i;
      if (j + 1 < N)
        hipLaunchKernelGGL(eigh_symv_kernel, dim3(tiles(j + 1), B), dim3(256), 0, st, n_nodes, N, ws, j, i);
      const bool more = i + 1 < jb;
      hipLaunchKernelGGL(eigh_column_kernel, dim3(B), dim3(COL_T), 0, st, n_nodes, N, ws, j, i,
                         more ? j + 1 : -1, more ? i + 1 : 0);
    }
    if (j0 + jb < N)
      hipLaunchKernelGGL(eigh_update_kernel, dim3(tiles(j0 + jb), B), dim3(256), 0, st, n_nodes, N, ws,
                         j0 + jb, jb);
    rc = check(who);
    if (rc != LNZ_OK) return rc;
  }
  hipLaunchKernelGGL(eigh_bisect_kernel, dim3(B), dim3(EIG_T), bis_lds, st, n_nodes, N, K, ws);
  rc = check(who);
  if (rc != LNZ_OK) return rc;
  // about 256 workgroups in all: a workgroup's LDS (7 N doubles) leaves room for one per CU, and a
  // grid of one workgroup per cluster measured slower at B = 256
  const int inv_x = std::max(1, std::min(K, (256 + B - 1) / B));
  hipLaunchKernelGGL(eigh_invit_kernel, dim3(inv_x, B), dim3(EIG_T), inv_lds, st, n_nodes, N, K, ws);
  rc = check(who);
  if (rc != LNZ_OK) return rc;
  hipLaunchKernelGGL(eigh_backtransform_kernel, dim3((K + KC - 1) / KC, B), dim3(256), 0, st, n_nodes, N, K, ws);
  rc = check(who);
  if (rc != LNZ_OK) return rc;
  hipLaunchKernelGGL(eigh_epilogue_kernel, dim3(K, B), dim3(256), 0, st, n_nodes, N, K, ws, D, V, info);
  return check(who);
}
