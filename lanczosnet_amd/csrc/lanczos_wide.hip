// The K-step Lanczos Ritz pairs (csrc/lanczos_large.hip: the reference's `eigsh` branch,
// utils/data_helper.py:205-208) for what one workgroup cannot hold: graphs of up to 16384 nodes and
// up to 256 Lanczos steps.  Same function as lnz_lanczos_ritz_kstep — same start vector, classical
// Gram-Schmidt against every previous vector with a second pass under the lnz::CgsBound rule, early
// stop on an invariant subspace (relative to the matrix' scale), top-K |theta| Ritz pairs — on
// another schedule: a graph is spread over many workgroups, and the stages are ordered by launch
// boundaries only (no grid-wide barrier, no spinning; the only atomics are the slab widths of the
// shared compaction pass, a max).  All
// arithmetic fp64, fp32 in and out.
//
// Per call:  compaction (csrc/ell_image.hpp: A read from HBM once into a sliced-ELL image) ->
// start vector -> M x { SpMV, dots, update, dots (pass 2), update (pass 2) } -> bisection and
// inverse iteration on the M x M tridiagonal (csrc/tridiag_eig.hpp, shared with the full
// decomposition) -> V = Q^T S.  5 M + 8 launches.
//
// What depends on the data — "this graph has stopped", "the second pass runs" — is decided on the
// device by every workgroup for itself from the same words in the workspace: the per-slab / per-chunk
// partial sums of |w|^2 that the previous launches left in fixed slots, alive[b][j] (step j of
// graph b was taken), again[b][j] and bound[b][j] (the second pass of step j runs; the bound on the
// loss of orthogonality of the vector it made: written by chunk 0's workgroup of the first update
// launch of step j) and tol[b] (the stop, from max |a_ij| as step 0's product met it).  A launch
// only reads words that an EARLIER launch wrote (the slots it writes itself belong to the current
// step: the SpMV's partials alternate between two sets by the parity of j).  The host never looks.
// Every sum has a fixed order that depends on N and the graph only:
// results are bitwise repeatable and independent of the rest of the batch.
//
// Bytes per graph and step j: the image (6 B per stored entry, slab padding included) + the gather
// of q from L2 (8 B per entry; q is 128 KiB at N = 16384), and the basis, (j + 1) N 8 B, twice per
// Gram-Schmidt pass (dots, update).
#include "common.hpp"
#include "edge_image.hpp"
#include "ell_image.hpp"
#include "tridiag_eig.hpp"
#include "wave.hpp"

#include <algorithm>

namespace {

constexpr int WT = 256;          // threads of every workgroup here
constexpr int CH = 512;          // rows per Gram-Schmidt chunk (one workgroup)
constexpr int MAX_N = 16384;
constexpr int MAX_M = 256;       // Lanczos steps (= lnz_tri::MAX_K: the tridiagonal stage's limit)
constexpr int DOT_U = 4;         // basis vectors a wave has in flight in the dots kernel
// early stop: |w| <= kTol lnz::matrix_scale_pow2(max |a_ij|); second Gram-Schmidt pass beyond kCgsFrac
// of |w|^2 or by the carried bound (lnz::CgsBound) — the rules of lanczos_large.hip, DESIGN.md 4.5h
constexpr double kTol = 1e-8;
constexpr double kCgsFrac = 1.0 - 1e-6;

using lnz_tri::block_max;
using lnz_tri::block_sum;
using lnz_tri::wave_sum_butterfly;

inline int64_t al256(int64_t x) { return (x + 255) / 256 * 256; }

struct Layout {
  int64_t Q, w, d, e, p0, p1, p2, cpart, Z, lam, sel, alive, steps, over, widths, vals, cols, rowcnt, total;
  int64_t again, bound, amax, tol;
  int64_t sel_stride;
  int nslab, nchunk;
};

Layout layout(int B, int N, int M, int row_cap) {
  Layout L;
  L.nslab = (N + 63) / 64;
  L.nchunk = (N + CH - 1) / CH;
  L.sel_stride = al256(lnz_tri::sel_bytes(M));
  int64_t at = 0;
  auto take = [&](int64_t bytes) {
    const int64_t here = at;
    at += al256(bytes);
    return here;
  };
  L.Q = take((int64_t)B * M * N * 8);
  L.w = take((int64_t)2 * B * N * 8);
  L.d = take((int64_t)B * M * 8);
  L.e = take((int64_t)B * M * 8);
  L.p0 = take((int64_t)2 * B * L.nslab * 8);
  L.p1 = take((int64_t)B * L.nchunk * 8);
  L.p2 = take((int64_t)B * L.nchunk * 8);
  L.cpart = take((int64_t)B * L.nchunk * M * 8);
  L.Z = take((int64_t)B * M * M * 8);
  L.lam = take((int64_t)B * M * 8);
  L.sel = take((int64_t)B * L.sel_stride);
  L.alive = take((int64_t)B * M * 4);
  L.steps = take((int64_t)B * 4);
  L.over = take((int64_t)B * 4);
  L.widths = take((int64_t)B * L.nslab * 4);
  L.vals = take((int64_t)B * L.nslab * row_cap * 64 * 4);
  L.cols = take((int64_t)B * L.nslab * row_cap * 64 * 2);
  L.rowcnt = take((int64_t)B * N * 4);
  L.again = take((int64_t)B * M * 4);
  L.bound = take((int64_t)B * M * 4);
  L.amax = take((int64_t)B * L.nslab * 4);
  L.tol = take((int64_t)B * 8);
  L.total = at;
  return L;
}

struct Wide {
  double* Q;       // [B][M][N] the Krylov basis
  double* w;       // [2][B][N] the vector of the recurrence: step j reads set j & 1, writes the other
  double* d;       // [B][M] alpha
  double* e;       // [B][M] beta
  double* p0;      // [2][B][nslab]  |A q|^2 by slab (set j & 1)
  double* p1;      // [B][nchunk]    |w|^2 by chunk after the first pass (the start vector's before step 0)
  double* p2;      // [B][nchunk]    ... after the second
  double* cpart;   // [B][nchunk][M] <q_i, w> by chunk
  double* Z;       // [B][M][M] eigenvectors of T, row = output slot
  double* lam;     // [B][M]
  char* sel;
  int64_t sel_stride;
  int32_t* alive;  // [B][M]
  int32_t* steps;  // [B]
  int32_t* again;  // [B][M] the second Gram-Schmidt pass of step j runs
  float* bound;    // [B][M] lnz::CgsBound's e^2 of the vector step j made
  float* amax;     // [B][nslab] max |a_ij| by slab (step 0)
  double* tol;     // [B] the stop: kTol times the matrix' scale
  const int32_t* over;   // [B] the image could not hold a row of this graph
  const float* vals;
  const uint16_t* cols;
  const int32_t* widths;
  const int32_t* n_nodes;
  int cap, B, N, M, K, nslab, nchunk;
  int skip_over;   // A's rows are not contiguous: a graph beyond the image is left to the caller
};

__device__ inline int graph_n(const Wide& p, int b) {
  if (!p.n_nodes) return p.N;
  const int n = p.n_nodes[b];
  return n < 0 ? 0 : (n > p.N ? p.N : n);
}

__device__ inline bool skipped(const Wide& p, int b) { return p.skip_over && p.over[b] != 0; }

// sum of up to WT slots in a fixed tree (every thread gets it)
__device__ inline double sum_slots(const double* s, int cnt, double* red) {
  const int t = threadIdx.x;
  return block_sum<WT>(t < cnt ? s[t] : 0.0, red);
}

// ---- start vector (same hash as every Ritz kernel of the project) ---------------------------------
__global__ __launch_bounds__(WT) void wide_init_kernel(Wide p) {
  __shared__ double red[WT];
  const int ch = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const int n_b = graph_n(p, b);
  double part = 0.0;
#pragma unroll
  for (int u = 0; u < CH / WT; ++u) {
    const int r = ch * CH + t + WT * u;
    if (r < p.N) {
      double w = 0.0;
      if (r < n_b) w = lnz::lanczos_start_entry(r);
      p.w[(int64_t)b * p.N + r] = w;
      part = fma(w, w, part);
    }
  }
  const double s = block_sum<WT>(part, red);
  if (t == 0) {
    p.p1[(int64_t)b * p.nchunk + ch] = s;
    if (ch == 0) p.steps[b] = 0;
  }
}

// ---- step j: beta_{j-1}, q_j = w / beta, w <- A q_j -------------------------------------------------
// Workgroup x of graph b: rows [256 x, 256 x + 256), one wave per 64-row slab.  On the image lane i
// forms row 64 g + i (entries in the order the compaction met them, two accumulators, as the
// one-workgroup kernel); for a graph beyond the image's row capacity the wave walks its 64 rows of
// the dense A one by one (contiguous rows, one float4 per lane and trip).
__global__ __launch_bounds__(WT) void wide_spmv_kernel(Wide p, const float* __restrict__ A, int64_t sb, int64_t sr,
                                                        int j) {
  __shared__ double red[WT];
  const int b = blockIdx.y, t = threadIdx.x;
  if (skipped(p, b)) return;
  const bool first = blockIdx.x == 0 && t == 0;
  int32_t* alive = p.alive + (int64_t)b * p.M;
  if (j > 0 && alive[j - 1] == 0) {
    if (first) alive[j] = 0;
    return;
  }
  const int n_b = graph_n(p, b);
  // |w|^2 as the last Gram-Schmidt pass that ran left it (the start vector's before step 0)
  const bool ran2 = j > 0 && p.again[(int64_t)b * p.M + j - 1] != 0;
  const double nrm2 = sum_slots((ran2 ? p.p2 : p.p1) + (int64_t)b * p.nchunk, p.nchunk, red);
  const double nrm = sqrt(nrm2);
  const double tol = j > 0 ? p.tol[b] : 0.0;
  // invariant subspace reached: stop (slots stay zero); an empty graph takes no step at all
  if ((j > 0 || n_b == 0) && nrm <= tol) {
    if (first) alive[j] = 0;
    return;
  }
  if (first) {
    alive[j] = 1;
    p.steps[b] = j + 1;
    if (j > 0) p.e[(int64_t)b * p.M + j - 1] = nrm;
  }
  const double ninv = 1.0 / nrm;
  const double* win = p.w + ((int64_t)(j & 1) * p.B + b) * p.N;
  double* wout = p.w + ((int64_t)((j + 1) & 1) * p.B + b) * p.N;
  {
    const int r = blockIdx.x * WT + t;
    if (r < p.N) p.Q[((int64_t)b * p.M + j) * p.N + r] = win[r] * ninv;
  }
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int g = blockIdx.x * (WT / 64) + wave;
  if (g >= p.nslab) return;
  double acc;
  float amax = 0.0f;
  if (p.over[b] == 0) {
    const int wdt = __builtin_amdgcn_readfirstlane(p.widths[(int64_t)b * p.nslab + g]);
    const int64_t base = (((int64_t)b * p.nslab + g) * p.cap) * 64 + lane;
    const float* vp = p.vals + base;
    const uint16_t* cp = p.cols + base;
    double acc0 = 0.0, acc1 = 0.0;
    for (int k0 = 0; k0 < wdt; k0 += ELL_UNROLL) {
      float vb[ELL_UNROLL];
      double qb[ELL_UNROLL];
#pragma unroll
      for (int i = 0; i < ELL_UNROLL; ++i) {
        vb[i] = vp[(int64_t)(k0 + i) * 64];
        qb[i] = win[cp[(int64_t)(k0 + i) * 64]];
        amax = fmaxf(amax, fabsf(vb[i]));   // (kept at j == 0 only: cheaper than a branch here)
      }
#pragma unroll
      for (int i = 0; i < ELL_UNROLL; i += 2) {
        acc0 = fma((double)vb[i], qb[i] * ninv, acc0);
        acc1 = fma((double)vb[i + 1], qb[i + 1] * ninv, acc1);
      }
    }
    acc = acc0 + acc1;
  } else {
    acc = 0.0;
    const int nq = p.N >> 2;
    for (int i = 0; i < 64; ++i) {
      const int row = 64 * g + i;
      if (row >= p.N) break;
      const float4* src = reinterpret_cast<const float4*>(A + (int64_t)b * sb + (int64_t)row * sr);
      double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
      for (int q = lane; q < nq; q += 64) {
        const float4 a = src[q];
        amax = fmaxf(fmaxf(amax, fmaxf(fabsf(a.x), fabsf(a.y))), fmaxf(fabsf(a.z), fabsf(a.w)));
        const double2* wp = reinterpret_cast<const double2*>(win + 4 * q);
        const double2 x = wp[0], y = wp[1];
        s0 = fma((double)a.x, x.x * ninv, s0);
        s1 = fma((double)a.y, x.y * ninv, s1);
        s2 = fma((double)a.z, y.x * ninv, s2);
        s3 = fma((double)a.w, y.y * ninv, s3);
      }
      const double tot = wave_sum_butterfly((s0 + s1) + (s2 + s3));
      if (lane == i) acc = tot;
    }
  }
  const int row = 64 * g + lane;
  if (row < p.N) wout[row] = acc;   // (rows in [N, 64 nslab) have no entries: acc = 0)
  const double s = wave_sum_butterfly(acc * acc);
  if (lane == 0) p.p0[((int64_t)(j & 1) * p.B + b) * p.nslab + g] = s;
  if (j == 0) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    if (lane == 0) p.amax[(int64_t)b * p.nslab + g] = amax;
  }
}

// ---- Gram-Schmidt, first half: the chunk's share of c_i = <q_i, w>, i <= j ---------------------------
// One wave per basis vector, DOT_U vectors in flight; lane l holds rows l, l + 64, ... of the chunk.
__global__ __launch_bounds__(WT) void wide_dots_kernel(Wide p, int j, int pass) {
  __shared__ double red[WT];
  const int ch = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  if (skipped(p, b) || p.alive[(int64_t)b * p.M + j] == 0) return;
  if (pass == 1 && p.again[(int64_t)b * p.M + j] == 0) return;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const double* w = p.w + ((int64_t)((j + 1) & 1) * p.B + b) * p.N;
  const double* Qb = p.Q + (int64_t)b * p.M * p.N;
  constexpr int RU = CH / 64;
  double wreg[RU];
  bool in[RU];
#pragma unroll
  for (int u = 0; u < RU; ++u) {
    const int r = ch * CH + lane + 64 * u;
    in[u] = r < p.N;
    wreg[u] = in[u] ? w[r] : 0.0;
  }
  double* cp = p.cpart + ((int64_t)b * p.nchunk + ch) * p.M;
  for (int i0 = wave; i0 <= j; i0 += (WT / 64) * DOT_U) {
    double qv[DOT_U][RU];
#pragma unroll
    for (int v = 0; v < DOT_U; ++v) {
      const int i = min(i0 + (WT / 64) * v, j);   // (past j: a repeat, not stored)
      const double* qi = Qb + (int64_t)i * p.N + ch * CH + lane;
#pragma unroll
      for (int u = 0; u < RU; ++u) qv[v][u] = in[u] ? qi[64 * u] : 0.0;
    }
#pragma unroll
    for (int v = 0; v < DOT_U; ++v) {
      double s0 = 0.0, s1 = 0.0;
#pragma unroll
      for (int u = 0; u < RU; u += 2) {
        s0 = fma(qv[v][u], wreg[u], s0);
        s1 = fma(qv[v][u + 1], wreg[u + 1], s1);
      }
      const double c = wave_sum_butterfly(s0 + s1);
      const int i = i0 + (WT / 64) * v;
      if (lane == 0 && i <= j) cp[i] = c;
    }
  }
}

// ---- Gram-Schmidt, second half: w -= sum_i c_i q_i on the chunk, |w|^2 of the chunk, alpha -------------
__global__ __launch_bounds__(WT) void wide_update_kernel(Wide p, int j, int pass) {
  __shared__ double red[WT];
  __shared__ double cs[MAX_M];
  const int ch = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  if (skipped(p, b) || p.alive[(int64_t)b * p.M + j] == 0) return;
  if (pass == 1 && p.again[(int64_t)b * p.M + j] == 0) return;
  if (t <= j) {
    const double* cp = p.cpart + (int64_t)b * p.nchunk * p.M + t;
    double c = 0.0;
    for (int k = 0; k < p.nchunk; ++k) c += cp[(int64_t)k * p.M];
    cs[t] = c;
  }
  __syncthreads();
  if (pass == 0 && ch == 0) {
    // Does the second pass run (lnz::CgsBound, wave.hpp)?  One workgroup decides for the graph, from
    // |A q|^2 and the squared coefficients, and leaves the word for the launches behind it.
    const double xx = sum_slots(p.p0 + ((int64_t)(j & 1) * p.B + b) * p.nslab, p.nslab, red);
    const double cc2 = block_sum<WT>(t <= j ? cs[t] * cs[t] : 0.0, red);
    lnz::CgsBound ob;
    ob.cur = j > 0 ? p.bound[(int64_t)b * p.M + j - 1] : 0.0f;
    ob.prev = j > 1 ? p.bound[(int64_t)b * p.M + j - 2] : 0.0f;
    const bool again = ob.second_pass(xx, cc2, ob.threshold(kCgsFrac, false), false);
    double am = 0.0;
    if (j == 0) am = block_max<WT>(t < p.nslab ? (double)p.amax[(int64_t)b * p.nslab + t] : 0.0, red);
    if (t == 0) {
      p.again[(int64_t)b * p.M + j] = again ? 1 : 0;
      p.bound[(int64_t)b * p.M + j] = ob.cand;
      if (j == 0) p.tol[b] = kTol * lnz::matrix_scale_pow2(am);
    }
  }
  double* w = p.w + ((int64_t)((j + 1) & 1) * p.B + b) * p.N;
  const double* Qb = p.Q + (int64_t)b * p.M * p.N;
  double part = 0.0;
#pragma unroll
  for (int u = 0; u < CH / WT; ++u) {
    const int r = ch * CH + t + WT * u;
    if (r < p.N) {
      const double* q = Qb + r;
      double acc0 = 0.0, acc1 = 0.0;
      int i = 0;
#pragma unroll 4
      for (; i + 1 <= j; i += 2) {
        acc0 = fma(cs[i], q[(int64_t)i * p.N], acc0);
        acc1 = fma(cs[i + 1], q[(int64_t)(i + 1) * p.N], acc1);
      }
      if (i <= j) acc0 = fma(cs[i], q[(int64_t)i * p.N], acc0);
      const double x = w[r] - (acc0 + acc1);
      w[r] = x;
      part = fma(x, x, part);
    }
  }
  const double s = block_sum<WT>(part, red);
  if (t == 0) {
    (pass ? p.p2 : p.p1)[(int64_t)b * p.nchunk + ch] = s;
    if (ch == 0) {
      double* dj = p.d + (int64_t)b * p.M + j;
      *dj = pass ? *dj + cs[j] : cs[j];
    }
  }
}

// ---- the steps x steps tridiagonal (csrc/tridiag_eig.hpp) ---------------------------------------------
__global__ __launch_bounds__(lnz_tri::EIG_T) void wide_bisect_kernel(Wide p) {
  __shared__ double d[MAX_M], e[MAX_M], e2[MAX_M];
  __shared__ double red[lnz_tri::EIG_T];
  __shared__ double lamc[lnz_tri::MAX_CAND];
  __shared__ int rankc[lnz_tri::MAX_CAND];
  const int b = blockIdx.x;
  if (skipped(p, b)) return;
  const lnz_tri::Sel sl = lnz_tri::sel_at(p.sel + (int64_t)b * p.sel_stride, p.K);
  const int n = p.steps[b];
  if (n == 0) {
    if (threadIdx.x == 0) sl.ncl[0] = 0;
    return;
  }
  lnz_tri::bisect_body(n, p.K, p.d + (int64_t)b * p.M, p.e + (int64_t)b * p.M, p.lam + (int64_t)b * p.M, sl, d, e,
                       e2, red, lamc, rankc);
}

__global__ __launch_bounds__(lnz_tri::EIG_T) void wide_invit_kernel(Wide p) {
  __shared__ double d[MAX_M], e[MAX_M], dd[MAX_M], du[MAX_M], du2[MAX_M], dl[MAX_M], x[MAX_M];
  __shared__ unsigned char piv[MAX_M];
  __shared__ double red[lnz_tri::EIG_T];
  __shared__ int clus[lnz_tri::MAX_K];
  __shared__ double hq[lnz_tri::MAX_K];
  const int b = blockIdx.y;
  if (skipped(p, b)) return;
  const int n = p.steps[b];
  if (n == 0) return;
  lnz_tri::invit_body(n, p.M, p.d + (int64_t)b * p.M, p.e + (int64_t)b * p.M,
                      lnz_tri::sel_at(p.sel + (int64_t)b * p.sel_stride, p.K), p.Z + (int64_t)b * p.M * p.M,
                      (int)blockIdx.x, (int)gridDim.x, d, e, dd, du, du2, dl, x, piv, red, clus, hq);
}

// ---- D [K], V [N, K] = Q^T S (plain fp64 FMA), fp32 out, zero padding -----------------------------------
// Workgroup (x, y) of graph b: rows [64 x, 64 x + 64) x Ritz vectors [64 y, 64 y + 64); lane = row,
// wave = 16 vectors.  The signed coefficients (largest-magnitude coefficient of a Ritz vector in the
// Krylov basis positive, as the one-workgroup kernel) pass through LDS 32 basis vectors at a time and
// are read as broadcasts; the sum over the basis runs in index order.
constexpr int VI = 32;
__global__ __launch_bounds__(WT) void wide_vectors_kernel(Wide p, float* __restrict__ D, float* __restrict__ V,
                                                           int32_t* __restrict__ info) {
  __shared__ double St[VI][64];
  __shared__ double sgn[64];
  const int b = blockIdx.z, t = threadIdx.x, k0 = 64 * blockIdx.y;
  if (skipped(p, b)) return;
  const int n = p.steps[b], n_b = graph_n(p, b);
  const int kk = p.K < n ? p.K : n;
  const double* Zb = p.Z + (int64_t)b * p.M * p.M;
  if (t < 64) {
    double sg = 1.0;
    if (k0 + t < kk) {
      const double* s = Zb + (int64_t)(k0 + t) * p.M;
      double best = 0.0;
      for (int x = 0; x < n; ++x) {
        const double av = fabs(s[x]);
        if (av > best) {
          best = av;
          sg = s[x] < 0 ? -1.0 : 1.0;
        }
      }
    }
    sgn[t] = sg;
    if (blockIdx.x == 0 && k0 + t < p.K)
      D[(int64_t)b * p.K + k0 + t] = k0 + t < kk ? (float)p.lam[(int64_t)b * p.M + k0 + t] : 0.0f;
  }
  if (info && blockIdx.x == 0 && blockIdx.y == 0 && t == 0) info[b] = n;
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int row = 64 * blockIdx.x + lane;
  const double* Qb = p.Q + (int64_t)b * p.M * p.N;
  double acc[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) acc[c] = 0.0;
  for (int i0 = 0; i0 < n; i0 += VI) {
    for (int idx = t; idx < VI * 64; idx += WT) {
      const int ii = idx & (VI - 1), kc = idx / VI;
      const int i = i0 + ii, k = k0 + kc;
      St[ii][kc] = (k < kk && i < n) ? sgn[kc] * Zb[(int64_t)k * p.M + i] : 0.0;
    }
    __syncthreads();
    const int ni = min(VI, n - i0);
    for (int ii = 0; ii < ni; ++ii) {
      const double q = row < p.N ? Qb[(int64_t)(i0 + ii) * p.N + row] : 0.0;
      const double* sp = &St[ii][16 * wave];
#pragma unroll
      for (int c = 0; c < 16; ++c) acc[c] = fma(q, sp[c], acc[c]);
    }
    __syncthreads();
  }
  if (row < p.N) {
    float* vr = V + ((int64_t)b * p.N + row) * p.K;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const int k = k0 + 16 * wave + c;
      if (k < p.K) vr[k] = (row < n_b && k < kk) ? (float)acc[c] : 0.0f;
    }
  }
}

}  // namespace

static int wide_steps(const char* who, const Layout& L, char* ws, const int32_t* over, const float* A, int64_t stride_b,
                      int64_t stride_r, bool skip_over, const int32_t* n_nodes, int B, int N, int M, int K, int row_cap,
                      float* D, float* V, int32_t* info, hipStream_t st);

extern "C" int64_t lnz_lanczos_ritz_kstep_wide_workspace_bytes(int B, int N, int M, int row_cap) {
  if (B <= 0 || N <= 0 || M <= 0 || row_cap <= 0) return 0;
  return layout(B, N, M, row_cap).total;
}

extern "C" int lnz_lanczos_ritz_kstep_wide(const float* A, int64_t stride_b, int64_t stride_r, int64_t stride_c,
                                           const int32_t* n_nodes, int B, int N, int M, int K, int row_cap,
                                           void* workspace, int64_t workspace_bytes, float* D, float* V,
                                           int32_t* info, int32_t* dense_fallback, lnz_stream_t stream) {
  const char* who = "lnz_lanczos_ritz_kstep_wide";
  LNZ_REQUIRE(stride_c == 1 || (stride_c == 2 && dense_fallback), LNZ_ENOTSUP,
              "%s: stride_c=%lld: columns are contiguous, or (with dense_fallback) A is channel 0 of a "
              "channels-last [N][N][2] block", who, (long long)stride_c);
  LNZ_REQUIRE(A && workspace && D && V && B > 0 && N > 0 && M > 0 && K > 0, LNZ_EINVAL,
              "%s: bad arguments (A, workspace, D, V non-null; B=%d N=%d M=%d K=%d >= 1)", who, B, N, M, K);
  LNZ_REQUIRE(N <= MAX_N && M <= MAX_M && K <= M, LNZ_ENOTSUP, "%s: N=%d <= %d, K=%d <= M=%d <= %d required", who,
              N, MAX_N, K, M, MAX_M);
  LNZ_REQUIRE(N % 4 == 0 && stride_r % 4 == 0 && stride_b % 4 == 0 && (reinterpret_cast<uintptr_t>(A) & 15) == 0,
              LNZ_ENOTSUP, "%s: rows must be 16-byte aligned, N %% 4 == 0", who);
  LNZ_REQUIRE(stride_r > 0 && stride_b >= 0 && ((int64_t)(N - 1) * stride_r + (int64_t)N * stride_c) * 4 < (int64_t)0xffffffff,
              LNZ_ENOTSUP, "%s: one graph must span less than 4 GiB (row stride %lld)", who, (long long)stride_r);
  LNZ_REQUIRE(M <= N, LNZ_EINVAL, "%s: M=%d > N=%d", who, M, N);
  LNZ_REQUIRE(B <= 65535, LNZ_EINVAL, "%s: B=%d: at most 65535 graphs per call (the caller chunks)", who, B);
  LNZ_REQUIRE(row_cap >= ELL_UNROLL && row_cap % ELL_UNROLL == 0 && row_cap <= 1024, LNZ_EINVAL,
              "%s: row_cap=%d must be a multiple of %d in [%d, 1024]", who, row_cap, ELL_UNROLL, ELL_UNROLL);
  const Layout L = layout(B, N, M, row_cap);
  LNZ_REQUIRE(workspace_bytes >= L.total, LNZ_EINVAL, "%s: workspace of %lld bytes, %lld needed", who,
              (long long)workspace_bytes, (long long)L.total);
  LNZ_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, LNZ_EINVAL, "%s: workspace alignment (256 B)", who);
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int32_t* over = dense_fallback ? dense_fallback : (int32_t*)(ws + L.over);
  int32_t* widths = (int32_t*)(ws + L.widths);
  float* vals = (float*)(ws + L.vals);
  uint16_t* cols = (uint16_t*)(ws + L.cols);
  int32_t* rowcnt = (int32_t*)(ws + L.rowcnt);
  if (hipMemsetAsync(over, 0, (size_t)B * 4, st) != hipSuccess ||
      hipMemsetAsync(widths, 0, (size_t)B * L.nslab * 4, st) != hipSuccess) {
    lnz::set_error("%s: hipMemsetAsync failed", who);
    return LNZ_ELAUNCH;
  }
  // ---- the image: the compaction pass of the one-workgroup path, unchanged (generic in N: u16 columns)
  const int64_t rows = (int64_t)B * N;
  const ConvImageOut nocv{nullptr, nullptr, nullptr, nullptr, 0};
  if (stride_c == 2)
    hipLaunchKernelGGL(ell_compact_rows_kernel<true>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, A, stride_b,
                       stride_r, B, N, row_cap, vals, cols, widths, rowcnt, over, nocv);
  else
    hipLaunchKernelGGL(ell_compact_rows_kernel<false>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, A, stride_b,
                       stride_r, B, N, row_cap, vals, cols, widths, rowcnt, over, nocv);
  int rc = lnz::check_launch(who);
  if (rc != LNZ_OK) return rc;
  hipLaunchKernelGGL(ell_pad_kernel, dim3((unsigned)(((int64_t)B * L.nslab + 3) / 4)), dim3(256), 0, st, B, N, row_cap,
                     vals, cols, widths, rowcnt);
  rc = lnz::check_launch(who);
  if (rc != LNZ_OK) return rc;
  return wide_steps(who, L, ws, over, A, stride_b, stride_r, stride_c != 1, n_nodes, B, N, M, K, row_cap, D, V, info, st);
}

// ---- the recurrence on the image in the workspace (`over`: the graphs it could not hold) --------------
static int wide_steps(const char* who, const Layout& L, char* ws, const int32_t* over, const float* A, int64_t stride_b,
                      int64_t stride_r, bool skip_over, const int32_t* n_nodes, int B, int N, int M, int K, int row_cap,
                      float* D, float* V, int32_t* info, hipStream_t st) {
  int rc;
  Wide p;
  p.Q = (double*)(ws + L.Q);
  p.w = (double*)(ws + L.w);
  p.d = (double*)(ws + L.d);
  p.e = (double*)(ws + L.e);
  p.p0 = (double*)(ws + L.p0);
  p.p1 = (double*)(ws + L.p1);
  p.p2 = (double*)(ws + L.p2);
  p.cpart = (double*)(ws + L.cpart);
  p.Z = (double*)(ws + L.Z);
  p.lam = (double*)(ws + L.lam);
  p.sel = ws + L.sel;
  p.sel_stride = L.sel_stride;
  p.alive = (int32_t*)(ws + L.alive);
  p.steps = (int32_t*)(ws + L.steps);
  p.again = (int32_t*)(ws + L.again);
  p.bound = (float*)(ws + L.bound);
  p.amax = (float*)(ws + L.amax);
  p.tol = (double*)(ws + L.tol);
  p.over = over;
  p.vals = (const float*)(ws + L.vals);
  p.cols = (const uint16_t*)(ws + L.cols);
  p.widths = (const int32_t*)(ws + L.widths);
  p.n_nodes = n_nodes;
  p.cap = row_cap;
  p.B = B;
  p.N = N;
  p.M = M;
  p.K = K;
  p.nslab = L.nslab;
  p.nchunk = L.nchunk;
  p.skip_over = skip_over ? 1 : 0;
  const dim3 gs((unsigned)((L.nslab + WT / 64 - 1) / (WT / 64)), (unsigned)B), gc((unsigned)L.nchunk, (unsigned)B);
  hipLaunchKernelGGL(wide_init_kernel, gc, dim3(WT), 0, st, p);
  for (int j = 0; j < M; ++j) {
    hipLaunchKernelGGL(wide_spmv_kernel, gs, dim3(WT), 0, st, p, A, stride_b, stride_r, j);
    for (int pass = 0; pass < 2; ++pass) {
      hipLaunchKernelGGL(wide_dots_kernel, gc, dim3(WT), 0, st, p, j, pass);
      hipLaunchKernelGGL(wide_update_kernel, gc, dim3(WT), 0, st, p, j, pass);
    }
    rc = lnz::check_launch(who);
    if (rc != LNZ_OK) return rc;
  }
  hipLaunchKernelGGL(wide_bisect_kernel, dim3(B), dim3(lnz_tri::EIG_T), 0, st, p);
  const int inv_x = std::max(1, std::min(K, (256 + B - 1) / B));
  hipLaunchKernelGGL(wide_invit_kernel, dim3(inv_x, B), dim3(lnz_tri::EIG_T), 0, st, p);
  hipLaunchKernelGGL(wide_vectors_kernel, dim3((unsigned)L.nslab, (unsigned)((K + 63) / 64), (unsigned)B), dim3(WT), 0,
                     st, p, D, V, info);
  lnz::note_kernel("lanczos_wide: wide_spmv_kernel, wide_dots_kernel, wide_update_kernel");
  return lnz::check_launch(who);
}

// ---- the same launches on an image built from edge lists (csrc/edge_image.hip): no dense A ------------
// workspace: the layout above, then the gate words and the builder's scratch
extern "C" int64_t lnz_lanczos_ritz_kstep_wide_edges_workspace_bytes(int B, int N, int M, int row_cap,
                                                                     int conv_row_cap) {
  if (B <= 0 || N <= 0 || M <= 0 || row_cap <= 0 || conv_row_cap < 0) return 0;
  return layout(B, N, M, row_cap).total + al256((int64_t)B * 4) +
         lnz::edge_scratch_bytes(B, N, lnz::edge_stage_cap(row_cap, conv_row_cap));
}

extern "C" int lnz_lanczos_ritz_kstep_wide_edges(const int32_t* edges, int64_t n_edges, const int64_t* edge_off,
                                                 const int32_t* n_nodes, int B, int N, int M, int K, int row_cap,
                                                 int row_order, void* workspace, int64_t workspace_bytes, float* D,
                                                 float* V, int32_t* info, int32_t* fallback, uint32_t* conv_entries,
                                                 float* conv_values, int32_t* conv_counts, int conv_row_cap,
                                                 int conv_order, int32_t* conv_flags, int32_t* status,
                                                 lnz_stream_t stream) {
  const char* who = "lnz_lanczos_ritz_kstep_wide_edges";
  LNZ_REQUIRE(workspace && D && V && B > 0 && N > 0 && M > 0 && K > 0, LNZ_EINVAL,
              "%s: bad arguments (workspace, D, V non-null; B=%d N=%d M=%d K=%d >= 1)", who, B, N, M, K);
  LNZ_REQUIRE(N <= MAX_N && M <= MAX_M && K <= M, LNZ_ENOTSUP, "%s: N=%d <= %d, K=%d <= M=%d <= %d required", who, N,
              MAX_N, K, M, MAX_M);
  LNZ_REQUIRE(N % 4 == 0, LNZ_ENOTSUP, "%s: N %% 4 == 0 required (pad the batch)", who);
  LNZ_REQUIRE(M <= N, LNZ_EINVAL, "%s: M=%d > N=%d", who, M, N);
  LNZ_REQUIRE(B <= 65535, LNZ_EINVAL, "%s: B=%d: at most 65535 graphs per call (the caller chunks)", who, B);
  LNZ_REQUIRE(row_cap > 0, LNZ_EINVAL, "%s: row_cap=%d", who, row_cap);
  const int ccap = conv_entries ? conv_row_cap : 0;
  const int64_t need = lnz_lanczos_ritz_kstep_wide_edges_workspace_bytes(B, N, M, row_cap, ccap);
  LNZ_REQUIRE(workspace_bytes >= need, LNZ_EINVAL, "%s: workspace of %lld bytes, %lld needed", who,
              (long long)workspace_bytes, (long long)need);
  LNZ_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, LNZ_EINVAL, "%s: workspace alignment (256 B)", who);
  const Layout L = layout(B, N, M, row_cap);
  char* ws = (char*)workspace;
  const int64_t scratch_at = L.total + al256((int64_t)B * 4);
  int32_t* over = fallback ? fallback : (int32_t*)(ws + L.over);
  int32_t* gate = (int32_t*)(ws + L.total);
  const lnz::EdgeBatch g{edges, n_edges, edge_off, n_nodes, B, N};
  const lnz::EdgeEll ell{(float*)(ws + L.vals), (uint16_t*)(ws + L.cols), (int32_t*)(ws + L.widths),
                         (int32_t*)(ws + L.rowcnt), over, row_cap, row_order};
  const lnz::EdgeConv cv{conv_entries, conv_values, conv_counts, conv_flags, ccap, conv_order};
  const lnz::EdgeRitz rz{D, V, info, K, gate};
  const int rc = lnz::edge_image_build(who, g, ell, cv, rz, ws + scratch_at, workspace_bytes - scratch_at, status,
                                       (hipStream_t)stream);
  if (rc != LNZ_OK) return rc;
  // a graph beyond row_cap or with a status is skipped by every launch (its D, V, info are zero already)
  return wide_steps(who, L, ws, gate, nullptr, 0, N, true, n_nodes, B, N, M, K, row_cap, D, V, info,
                    (hipStream_t)stream);
}
