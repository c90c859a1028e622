// The top-K |lambda| eigenpairs of a symmetric tridiagonal T (n <= 2048 rows, K <= 256), shared by
// the full decomposition (csrc/sym_eigh.hip, stage 3) and the wide K-step Lanczos path
// (csrc/lanczos_wide.hip, the M x M matrix of the recurrence): split at negligible off-diagonals,
// Sturm-count bisection for the K smallest and K largest eigenvalues, the stable descending-|lambda|
// cut, inverse iteration with partial-pivoting LU (dgttrf / dgttrs) and re-orthogonalisation (CGS2)
// inside clusters (dstein's 1e-3 ||T|| cluster gap).  The callers own the kernels (where T lives,
// how n is found, LDS); the bodies below are the one implementation of the arithmetic.  Every sum
// runs in a fixed order that depends on n only.
#pragma once
#include "common.hpp"

#include <float.h>

namespace lnz_tri {

constexpr int EIG_T = 256;       // threads of a workgroup that runs one of the bodies
constexpr int MAX_K = 256;
constexpr int MAX_CAND = 2 * MAX_K;

// Deterministic block sum: every thread's value into red[], then a fixed halving tree.
template <int T>
__device__ double block_sum(double v, double* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
#pragma unroll
  for (int s = T / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

template <int T>
__device__ double block_max(double v, double* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
#pragma unroll
  for (int s = T / 2; s > 0; s >>= 1) {
    if (t < s) red[t] = fmax(red[t], red[t + s]);
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// Wave sum in a fixed butterfly order (every lane gets the total): NOT the tree of lnz::wave_sum
// (wave.hpp) — another summation order, other bits.
__device__ inline double wave_sum_butterfly(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ inline int sturm_count(const double* d, const double* e2, int n, double x, double pivmin) {
  double q = d[0] - x;
  if (fabs(q) <= pivmin) q = -pivmin;
  int cnt = q <= 0.0;
  for (int k = 1; k < n; ++k) {
    q = (d[k] - x) - e2[k - 1] / q;
    if (fabs(q) <= pivmin) q = -pivmin;
    cnt += q <= 0.0;
  }
  return cnt;
}

__device__ inline double start_entry(int r, int slot) {
  uint32_t h = (uint32_t)r * 2654435761u ^ ((uint32_t)slot * 40503u + 0x9E3779B9u);
  h ^= h >> 16;
  h *= 0x7feb352du;
  h ^= h >> 15;
  h *= 0x846ca68bu;
  h ^= h >> 16;
  return (double)h * (2.0 / 4294967296.0) - 1.0;
}

// The selected pairs in ascending order and their clusters, written by bisect_body for invit_body
// and the callers' epilogues (a [K + 2] double and a [3 K + 2] int block per graph).
struct Sel {
  double* lam;     // [K] selected eigenvalues, ascending
  double* nrm;     // [2]: ||T||, pivmin
  int32_t* slot;   // [K] output slot of each (its descending-|lambda| rank)
  int32_t* cstart; // [K + 1] first ascending position of each cluster, then kk
  int32_t* fail;   // [K] per cluster: an inverse iteration did not converge
  int32_t* ncl;    // [1] number of clusters
};

__host__ __device__ inline int64_t sel_bytes(int K) { return (int64_t)(K + 2) * 8 + (int64_t)(3 * K + 2) * 4; }

__device__ inline Sel sel_at(char* base, int K) {
  Sel s;
  s.lam = (double*)base;
  s.nrm = s.lam + K;
  s.slot = (int32_t*)(s.nrm + 2);
  s.cstart = s.slot + K;
  s.fail = s.cstart + K + 1;
  s.ncl = s.fail + K;
  return s;
}

// One workgroup of EIG_T threads, n >= 1.  dg / eg: the diagonal [n] and off-diagonal [n - 1] of T
// in global memory (eg [n] receives the split off-diagonals: negligible ones as zeros).  d, e, e2:
// LDS, n doubles each; red [EIG_T], lamc / rankc [MAX_CAND]: LDS scratch.  Writes lam_out[rank] for
// the min(n, K) selected eigenvalues and the block `sl`.
__device__ inline void bisect_body(const int n, const int K, const double* dg, double* eg, double* lam_out,
                                   const Sel sl, double* d, double* e, double* e2, double* red, double* lamc,
                                   int* rankc) {
  const int t = threadIdx.x;
  const int kk = n < K ? n : K;
  for (int r = t; r < n; r += EIG_T) {
    d[r] = dg[r];
    e[r] = r < n - 1 ? eg[r] : 0.0;
  }
  __syncthreads();
  double lmax = 0.0;
  for (int r = t; r < n; r += EIG_T)
    lmax = fmax(lmax, fabs(d[r]) + fabs(e[r]) + (r > 0 ? fabs(e[r - 1]) : 0.0));
  const double tnorm = block_max<EIG_T>(lmax, red);
  const double eps = DBL_EPSILON;
  // split: an off-diagonal entry below n eps ||T|| is set to zero (T decouples there)
  const double thr = (double)n * eps * tnorm;
  double e2max = 0.0;
  for (int r = t; r < n; r += EIG_T) {
    if (fabs(e[r]) <= thr) e[r] = 0.0;
    e2[r] = e[r] * e[r];
    e2max = fmax(e2max, e2[r]);
    eg[r] = e[r];
  }
  const double pivmin = DBL_MIN * fmax(1.0, block_max<EIG_T>(e2max, red));
  double glo = INFINITY, ghi = -INFINITY;
  for (int r = t; r < n; r += EIG_T) {
    const double rad = fabs(e[r]) + (r > 0 ? fabs(e[r - 1]) : 0.0);
    glo = fmin(glo, d[r] - rad);
    ghi = fmax(ghi, d[r] + rad);
  }
  glo = -block_max<EIG_T>(-glo, red);
  ghi = block_max<EIG_T>(ghi, red);
  const double pad = 2.0 * eps * tnorm * n + 2.0 * pivmin;
  glo -= pad;
  ghi += pad;
  // candidates: the K smallest and the K largest (all of them when they overlap), ascending
  const int nc = 2 * kk >= n ? n : 2 * kk;
  const double atol = 2.0 * eps * tnorm + pivmin;
  for (int c = t; c < nc; c += EIG_T) {
    const int idx = (nc == n || c < kk) ? c : n - 2 * kk + c;
    double lo = glo, hi = ghi;
    for (int it = 0; it < 256; ++it) {
      if (!(hi - lo > fmax(atol, 2.0 * eps * fmax(fabs(lo), fabs(hi))))) break;
      const double mid = 0.5 * (lo + hi);
      if (mid <= lo || mid >= hi) break;
      if (sturm_count(d, e2, n, mid, pivmin) <= idx) lo = mid;
      else hi = mid;
    }
    lamc[c] = 0.5 * (lo + hi);
  }
  __syncthreads();
  // stable descending-|lambda| rank over ascending lambda (np.argsort(-|w|, kind='mergesort'))
  for (int c = t; c < nc; c += EIG_T) {
    const double a = fabs(lamc[c]);
    int rk = 0;
    for (int q = 0; q < nc; ++q) {
      const double aq = fabs(lamc[q]);
      rk += (aq > a) || (aq == a && q < c);
    }
    rankc[c] = rk;
    if (rk < kk) lam_out[rk] = lamc[c];
  }
  __syncthreads();
  // the selected ones in ascending order; a cluster starts where the gap exceeds dstein's 1e-3 ||T||
  if (t == 0) {
    const double ortol = 1e-3 * tnorm;
    int p = 0, q = 0;
    double prev = 0.0;
    for (int c = 0; c < nc; ++c) {
      if (rankc[c] >= kk) continue;
      const double lam = lamc[c];
      if (p == 0 || lam - prev > ortol) {
        sl.cstart[q] = p;
        sl.fail[q] = 0;
        ++q;
      }
      prev = lam;
      sl.lam[p] = lam;
      sl.slot[p] = rankc[c];
      ++p;
    }
    sl.cstart[q] = p;
    sl.ncl[0] = q;
    sl.nrm[0] = tnorm;
    sl.nrm[1] = pivmin;
  }
}

// One workgroup of EIG_T threads takes clusters cq0, cq0 + cqstep, ... of the block `sl` (the
// results do not depend on the split).  dg / eg as bisect_body left them; Z [K][ldz] receives the
// unit eigenvector of output slot s in row s.  LDS: d, e, dd, du, du2, dl, x [n] doubles,
// piv [n] bytes, red [EIG_T], clus / hq [MAX_K].  Inside a cluster the vectors are computed in
// ascending order, each re-orthogonalised (CGS2) against the cluster's earlier ones.
__device__ inline void invit_body(const int n, const int ldz, const double* dg, const double* eg, const Sel sl,
                                  double* Z, const int cq0, const int cqstep, double* d, double* e, double* dd,
                                  double* du, double* du2, double* dl, double* x, unsigned char* piv,
                                  double* red, int* clus, double* hq) {
  const int t = threadIdx.x;
  const int N = ldz;
  const int ncl_all = sl.ncl[0];
  if (cq0 >= ncl_all) return;
  for (int r = t; r < n; r += EIG_T) {
    d[r] = dg[r];
    e[r] = r < n - 1 ? eg[r] : 0.0;
  }
  __syncthreads();
  const double tnorm = sl.nrm[0], pivmin = sl.nrm[1];
  const double eps = DBL_EPSILON;
  const double pert = eps * tnorm > pivmin ? eps * tnorm : pivmin;
  const int wave = t >> 6, lane = t & 63;
  for (int cq = cq0; cq < ncl_all; cq += cqstep) {
  const int p0 = sl.cstart[cq], p1 = sl.cstart[cq + 1];
  int fail = 0;
  for (int p = p0; p < p1; ++p) {
    const int ncl = p - p0;
    const int slot = sl.slot[p];
    const double lam = sl.lam[p];
    // LU of T - lam I with partial pivoting (dgttrf), tiny pivots perturbed
    if (t == 0) {
      for (int r = 0; r < n; ++r) {
        dd[r] = d[r] - lam;
        du[r] = e[r];
        dl[r] = e[r];
        du2[r] = 0.0;
        piv[r] = 0;
      }
      for (int r = 0; r < n - 1; ++r) {
        if (fabs(dd[r]) >= fabs(dl[r])) {
          if (dd[r] != 0.0) {
            const double f = dl[r] / dd[r];
            dl[r] = f;
            dd[r + 1] -= f * du[r];
          }
        } else {
          const double f = dd[r] / dl[r];
          dd[r] = dl[r];
          dl[r] = f;
          const double tmp = du[r];
          du[r] = dd[r + 1];
          dd[r + 1] = tmp - f * dd[r + 1];
          if (r < n - 2) {
            du2[r] = du[r + 1];
            du[r + 1] = -f * du[r + 1];
          }
          piv[r] = 1;
        }
      }
      for (int r = 0; r < n; ++r)
        if (fabs(dd[r]) < pert) dd[r] = dd[r] < 0.0 ? -pert : pert;
    }
    for (int r = t; r < n; r += EIG_T) x[r] = start_entry(r, slot);
    __syncthreads();
    for (int it = 0; it < 3; ++it) {
      if (t == 0) {
        for (int r = 0; r < n - 1; ++r) {
          if (!piv[r]) {
            x[r + 1] -= dl[r] * x[r];
          } else {
            const double tmp = x[r];
            x[r] = x[r + 1];
            x[r + 1] = tmp - dl[r] * x[r];
          }
        }
        x[n - 1] /= dd[n - 1];
        if (n > 1) x[n - 2] = (x[n - 2] - du[n - 2] * x[n - 1]) / dd[n - 2];
        for (int r = n - 3; r >= 0; --r) x[r] = (x[r] - du[r] * x[r + 1] - du2[r] * x[r + 2]) / dd[r];
      }
      __syncthreads();
      double mx = 0.0;
      for (int r = t; r < n; r += EIG_T) mx = fmax(mx, fabs(x[r]));
      mx = block_max<EIG_T>(mx, red);
      const double inv = mx > 0.0 ? 1.0 / mx : 1.0;
      for (int r = t; r < n; r += EIG_T) x[r] *= inv;
      __syncthreads();
      for (int pass = 0; pass < 2 && ncl > 0; ++pass) {
        for (int q = wave; q < ncl; q += EIG_T / 64) {
          const double* zq = Z + (int64_t)clus[q] * N;
          double s = 0.0;
          for (int r = lane; r < n; r += 64) s += zq[r] * x[r];
          s = wave_sum_butterfly(s);
          if (lane == 0) hq[q] = s;
        }
        __syncthreads();
        for (int r = t; r < n; r += EIG_T) {
          double v = x[r];
          for (int q = 0; q < ncl; ++q) v -= hq[q] * Z[(int64_t)clus[q] * N + r];
          x[r] = v;
        }
        __syncthreads();
      }
      double ss = 0.0;
      for (int r = t; r < n; r += EIG_T) ss += x[r] * x[r];
      const double nrm = sqrt(block_sum<EIG_T>(ss, red));
      const double sc = nrm > 0.0 ? 1.0 / nrm : 0.0;
      for (int r = t; r < n; r += EIG_T) x[r] *= sc;
      __syncthreads();
    }
    // residual of the pair on T
    double res = 0.0;
    for (int r = t; r < n; r += EIG_T) {
      double y = (d[r] - lam) * x[r];
      if (r > 0) y += e[r - 1] * x[r - 1];
      if (r < n - 1) y += e[r] * x[r + 1];
      res = fmax(res, fabs(y));
      Z[(int64_t)slot * N + r] = x[r];
    }
    res = block_max<EIG_T>(res, red);
    // relative to ||T||, and never below what bisection resolves: it places an eigenvalue of the
    // zero matrix within its pad of 2 pivmin (at -1.5 pivmin), a residual of that size on T = 0
    if (!(res <= fmax(1e-9 * tnorm, 4.0 * pivmin))) fail = 1;
    if (t == 0) clus[ncl] = slot;
    __syncthreads();
  }
  if (t == 0) sl.fail[cq] = fail;
  }
}

}  // namespace lnz_tri
