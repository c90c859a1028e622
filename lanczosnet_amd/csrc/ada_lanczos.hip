// AdaLanczosNet stages:
//   lnz_ada_graph_laplacian   model/ada_lanczos_net.py:101-137  Gaussian-kernel learned Laplacian
//   lnz_ada_lanczos_layer     model/ada_lanczos_net.py:139-247  in-model Lanczos layer, the
//                             reference's algorithm step for step ("ada_ref"): sequential
//                             Gram-Schmidt twice, the 1e-4 breakdown mask and the three quirks of
//                             SURVEY.md F6 / §A.3.  fp32 in / fp32 out, fp64 inside: an fp32
//                             Lanczos recurrence drifts from exact arithmetic by 1e-6 (median) to
//                             2e-4 (worst of 512 QM8-sized molecules, the reference's own torch
//                             CPU run measured against an fp64 restatement), in a way that depends
//                             on the summation order of every dot product — no second fp32
//                             implementation can reproduce that noise.  Computing the recurrence in
//                             fp64 puts this kernel at the exact-arithmetic result, so its distance
//                             to the reference IS the reference's own rounding noise
//                             (tests/test_gpu_ada.py asserts exactly that, per molecule).
//   lnz_ada_t_powers          model/ada_lanczos_net.py:262-270  T^p by sequential TT = TT T (fp64
//                             products, rounded to fp32 on output)
//   lnz_ada_symmetrize_filters :276-278 (DD + DD^T)/2, relaid out [B,K,K,S] -> [B,S,K,K]
#include "common.hpp"
#include "wave.hpp"

namespace {

using lnz::wave_sum;

constexpr float kEpsF = 1.1920928955078125e-07f;  // np.finfo(np.float32).eps (ada_lanczos_net.py:8)

// ---------------------------------------------------------------------------------------------
// R4: learned graph Laplacian.  One workgroup per molecule.
//   dist2[i][j] = |x_j - x_i|^2 ; sigma2 = mean over ALL N^2 pairs (padded nodes included, as
//   the reference) ; A = exp(-dist2 / sigma2) * adj ; D = (rowsum + [rowsum == 0])^-1/2 ; L = D A D
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ada_graph_laplacian_kernel(
    const int64_t* __restrict__ node_feat, const float* __restrict__ embedding, int num_atom,
    const float* __restrict__ Xf, int Dm, const float* __restrict__ L0, int64_t sb, int64_t sr,
    int64_t sc, int N, float* __restrict__ Le) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* X = smem;                  // [N][Dm]
  float* d2 = X + N * Dm;           // [N][N]  -> later A
  float* red = d2 + N * N;          // [256] partial sums / row scale
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int idx = tid; idx < N * Dm; idx += 256) {
    int i = idx / Dm, f = idx - i * Dm;
    float v;
    if (node_feat) {
      int64_t id = node_feat[(int64_t)b * N + i];
      id = id < 0 ? 0 : (id >= num_atom ? num_atom - 1 : id);
      v = embedding[id * Dm + f];
    } else {
      v = Xf[((int64_t)b * N + i) * Dm + f];
    }
    X[idx] = v;
  }
  __syncthreads();
  double part = 0.0;
  for (int p = tid; p < N * N; p += 256) {
    int i = p / N, jn = p - i * N;
    float s = 0.0f;
    for (int f = 0; f < Dm; ++f) {
      float df = X[jn * Dm + f] - X[i * Dm + f];
      s = fmaf(df, df, s);
    }
    d2[p] = s;
    part += (double)s;
  }
  // block reduction of the mean (fp64 accumulate, rounded once)
  __shared__ double dred[256];
  dred[tid] = part;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) dred[tid] += dred[tid + st];
    __syncthreads();
  }
  const float sigma2 = (float)(dred[0] / (double)(N * N));
  const float* Lb = L0 + (int64_t)b * sb;
  for (int p = tid; p < N * N; p += 256) {
    int i = p / N, jn = p - i * N;
    float adj = Lb[i * sr + jn * sc] != 0.0f ? 1.0f : 0.0f;  // :310-311
    d2[p] = expf(-d2[p] / sigma2) * adj;
  }
  __syncthreads();
  for (int i = tid; i < N; i += 256) {
    double rs = 0.0;
    for (int jn = 0; jn < N; ++jn) rs += (double)d2[i * N + jn];
    float rowsum = (float)rs;
    float pad = rowsum == 0.0f ? 1.0f : 0.0f;
    red[i] = 1.0f / sqrtf(rowsum + pad);  // 1 / (row_sum + pad).pow(0.5)
  }
  __syncthreads();
  float* out = Le + (int64_t)b * N * N;
  for (int p = tid; p < N * N; p += 256) {
    int i = p / N, jn = p - i * N;
    out[p] = (red[i] * d2[p]) * red[jn];
  }
}

// ---------------------------------------------------------------------------------------------
// R5: the reference's Lanczos layer.  One wavefront per molecule, lane = node row (N <= 64).
// A tile (fp32, as given) and the basis (fp64) live in LDS; alpha / beta / Gram-Schmidt
// coefficients are fp64 wave reductions (DPP tree, identical in every lane).
// ---------------------------------------------------------------------------------------------
template <int NMAX, int KMAX>
__global__ __launch_bounds__(64) void ada_lanczos_layer_kernel(
    const float* __restrict__ A, const uint8_t* __restrict__ mask, const float* __restrict__ q1,
    int N, int K, float* __restrict__ T, float* __restrict__ Q) {
  __shared__ float As[NMAX * (NMAX + 1)];
  __shared__ double Qs[(KMAX + 2) * NMAX];  // Q[0] = 0, Q[1..Tit+1]
  __shared__ double zb[NMAX];
  __shared__ double alpha_s[KMAX + 1], beta_s[KMAX + 1], qq_s[KMAX + 2];
  __shared__ float valid_s[KMAX + 1];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int Tit = N < K ? N : K;
  const double eps = (double)kEpsF;
  const float* Ab = A + (int64_t)b * N * N;
  for (int idx = lane; idx < N * N; idx += 64) {
    int r = idx / N, c = idx - r * N;
    As[r * (NMAX + 1) + c] = Ab[idx];
  }
  const bool row = lane < N;
  const float mk = (row && (mask == nullptr || mask[(int64_t)b * N + lane] != 0)) ? 1.0f : 0.0f;
  double q = row ? (double)(q1[(int64_t)b * N + lane] * mk) : 0.0;  // :161-165
  {
    double nrm = sqrt(wave_sum(q * q));
    q = q / nrm;  // :167 (no EPS: an all-masked molecule is NaN in the reference too)
  }
  if (lane < NMAX) {
    Qs[0 * NMAX + lane] = 0.0;
    Qs[1 * NMAX + lane] = q;
  }
  double q_prev = 0.0, beta_prev = 0.0;
  float valid_prev = 1.0f;
  const float nmask = wave_sum(mk);
  __syncthreads();
  for (int ii = 1; ii <= Tit; ++ii) {
    if (lane < NMAX) zb[lane] = q;
    __syncthreads();
    double z = 0.0;
    if (row) {
      const float* ar = &As[lane * (NMAX + 1)];
      for (int c = 0; c < N; ++c) z = fma((double)ar[c], zb[c], z);  // :173
    }
    const double alpha = wave_sum(q * z);              // :174
    z = z - alpha * q - beta_prev * q_prev;            // :175
    if (ii > 1) {                                      // :177-189, use_reorthogonalization (F7)
      for (int pass = 0; pass < 2; ++pass) {
        for (int jj = 1; jj < ii; ++jj) {
          const double qj = lane < NMAX ? Qs[jj * NMAX + lane] : 0.0;
          const double num = wave_sum(z * qj);
          z = z - num / (qq_s[jj] + eps) * qj;
        }
      }
    }
    const double beta = sqrt(wave_sum(z * z));         // :191
    const float ok = beta >= (double)1.0e-4f ? 1.0f : 0.0f;  // :195 (the fp32 constant lb)
    const float valid = (ii == 1) ? ok : valid_prev * ok;  // :196-199
    const double qn = (z * (double)valid) / (beta + eps);  // :202
    if (lane == 0) {
      alpha_s[ii] = alpha;
      beta_s[ii] = beta;
      valid_s[ii] = valid;
    }
    const double qq_cur = wave_sum(q * q);             // <Q[ii], Q[ii]> for later projections
    if (lane == 0) qq_s[ii] = qq_cur;
    if (lane < NMAX) Qs[(ii + 1) * NMAX + lane] = qn;
    q_prev = q;
    q = qn;
    beta_prev = beta;
    valid_prev = valid;
    __syncthreads();
  }
  // idx_mask = min(sum(valid), sum(mask))  (:209-211); valid[idx_mask:] = 0 (:213-215)
  float vsum = 0.0f;
  for (int ii = 1; ii <= Tit; ++ii) vsum += valid_s[ii];
  int idx_mask = (int)vsum;
  if (mask != nullptr) {
    int nm = (int)nmask;
    idx_mask = idx_mask < nm ? idx_mask : nm;
  }
  // T [K,K] (zero padded) = diag(alpha*valid) + offdiag(beta*valid[:-1])   (:218-226, quirk 1)
  float* Tb = T + (int64_t)b * K * K;
  for (int idx = lane; idx < K * K; idx += 64) {
    int i = idx / K, jn = idx - i * K;
    float v = 0.0f;
    if (i < Tit && jn < Tit) {
      auto vm = [&](int t0) { return (t0 < idx_mask) ? valid_s[t0 + 1] : 0.0f; };  // 0-based step
      if (i == jn) v = (float)alpha_s[i + 1] * vm(i);
      else if (jn == i + 1 && i < Tit - 1) v = (float)beta_s[i + 1] * vm(i);
      else if (i == jn + 1 && jn < Tit - 1) v = (float)beta_s[jn + 1] * vm(jn);
    }
    Tb[idx] = v;
  }
  // Q [N,K] = [q_1..q_Tit] * valid (per column, quirk 2); rows >= idx_mask zeroed (quirk 3)
  float* Qb = Q + (int64_t)b * N * K;
  for (int idx = lane; idx < N * K; idx += 64) {
    int r = idx / K, k = idx - r * K;
    float v = 0.0f;
    if (k < Tit) {
      float vmk = (k < idx_mask) ? valid_s[k + 1] : 0.0f;
      float rowkeep = (idx_mask < N && r >= idx_mask) ? 0.0f : 1.0f;
      v = (float)Qs[(k + 1) * NMAX + r] * (vmk * rowkeep);  // Q * Q_mask (:237)
    }
    Qb[idx] = v;
  }
}

// ---------------------------------------------------------------------------------------------
// R8 glue: T^p (sequential TT = TT T, fp32) -> Tcat [B, K, S*K] as torch.cat(T_list, dim=2)
// ---------------------------------------------------------------------------------------------
struct PowArr {
  int32_t v[16];
};

__global__ __launch_bounds__(256) void ada_t_powers_kernel(const float* __restrict__ T, int K,
                                                            PowArr dist, int S, int pmax,
                                                            float* __restrict__ Tcat) {
  extern __shared__ __attribute__((aligned(16))) double dsmem[];
  double* Ts = dsmem;           // [K][K]
  double* TT = Ts + K * K;      // current power
  double* TN = TT + K * K;      // next
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < K * K; i += 256) {
    double v = (double)T[(int64_t)b * K * K + i];
    Ts[i] = v;
    TT[i] = v;
  }
  __syncthreads();
  float* out = Tcat + (int64_t)b * K * S * K;
  for (int ii = 1; ii <= pmax; ++ii) {
    for (int s = 0; s < S; ++s) {
      if (dist.v[s] == ii) {
        for (int i = tid; i < K * K; i += 256) {
          int r = i / K, c = i - r * K;
          out[(int64_t)r * S * K + s * K + c] = (float)TT[i];
        }
      }
    }
    if (ii == pmax) break;
    for (int i = tid; i < K * K; i += 256) {
      int r = i / K, c = i - r * K;
      double acc = 0.0;
      for (int k = 0; k < K; ++k) acc = fma(TT[r * K + k], Ts[k * K + c], acc);
      TN[i] = acc;
    }
    __syncthreads();
    double* t = TT;
    TT = TN;
    TN = t;
  }
}

// DDp[b][s][k1][k2] = 0.5 * (DD[b][k1][k2][s] + DD[b][k2][k1][s])
__global__ void ada_symmetrize_kernel(const float* __restrict__ DD, int64_t total, int K, int S,
                                      float* __restrict__ DDp) {
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int k2 = (int)(idx % K);
  int k1 = (int)((idx / K) % K);
  int s = (int)((idx / ((int64_t)K * K)) % S);
  int64_t b = idx / ((int64_t)K * K * S);
  const float* base = DD + b * K * K * S;
  float x = base[((int64_t)k1 * K + k2) * S + s];
  float y = base[((int64_t)k2 * K + k1) * S + s];
  DDp[idx] = (x + y) * 0.5f;
}


// ---- split-precision operand of the filter MLP's library GEMMs (opt-in, R8) ---------------------
// v = [relu](alpha * X[m][k] + bias[k])  ->  out[m] = [ hi | hi | lo ] (3 Kp halfs),
// hi = fp16(v), lo = fp16(v - hi): against weights stored as [ w_hi | w_lo | w_hi ] one fp16 GEMM
// of depth 3 Kp accumulates  hi w_hi + hi w_lo + lo w_hi  in fp32 — v w to ~2^-22 relative.
__global__ void split_f16x3_kernel(const float* __restrict__ X, int M, int K, int ldx,
                                   const float* __restrict__ bias, float alpha, int relu, int Kp,
                                   _Float16* __restrict__ out) {
  typedef _Float16 h4 __attribute__((ext_vector_type(4)));
  const int c4 = blockIdx.x * blockDim.x + threadIdx.x;  // group of 4 columns
  const int m = blockIdx.y;
  if (4 * c4 >= Kp) return;
  float v[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int k = 4 * c4 + u;
    float x = 0.0f;
    if (k < K) {
      x = X[(int64_t)m * ldx + k] * alpha + (bias ? bias[k] : 0.0f);
      if (relu) x = fmaxf(x, 0.0f);
    }
    v[u] = x;
  }
  h4 hi, lo;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    hi[u] = (_Float16)v[u];
    lo[u] = (_Float16)(v[u] - (float)hi[u]);
  }
  _Float16* o = out + (int64_t)m * 3 * Kp + 4 * c4;
  *reinterpret_cast<h4*>(o) = hi;
  *reinterpret_cast<h4*>(o + Kp) = hi;
  *reinterpret_cast<h4*>(o + 2 * Kp) = lo;
}

}  // namespace

extern "C" int lnz_ada_graph_laplacian(const int64_t* node_feat, const float* embedding,
                                       int num_atom, const float* node_feat_f, int D,
                                       const float* L0, int64_t stride_b, int64_t stride_r,
                                       int64_t stride_c, int B, int N, float* Le,
                                       lnz_stream_t stream) {
  LNZ_REQUIRE(((node_feat && embedding && num_atom > 0) || node_feat_f) && L0 && Le && B > 0 &&
                  N > 0 && D > 0,
              LNZ_EINVAL, "lnz_ada_graph_laplacian: bad arguments (B=%d N=%d D=%d)", B, N, D);
  size_t lds = ((size_t)N * D + (size_t)N * N + 256) * sizeof(float);
  LNZ_REQUIRE(lds <= 60 * 1024, LNZ_ENOTSUP, "lnz_ada_graph_laplacian: N*D + N*N too large");
  hipLaunchKernelGGL(ada_graph_laplacian_kernel, dim3(B), dim3(256), lds, (hipStream_t)stream,
                     node_feat, embedding, num_atom, node_feat_f, D, L0, stride_b, stride_r,
                     stride_c, N, Le);
  return lnz::check_launch("lnz_ada_graph_laplacian");
}

extern "C" int lnz_ada_lanczos_layer(const float* A, const uint8_t* mask, const float* q1, int B,
                                     int N, int K, float* T, float* Q, lnz_stream_t stream) {
  LNZ_REQUIRE(A && q1 && T && Q && B > 0 && N > 0 && K > 0, LNZ_EINVAL,
              "lnz_ada_lanczos_layer: bad arguments (B=%d N=%d K=%d)", B, N, K);
  LNZ_REQUIRE(N <= 64 && K <= 64, LNZ_ENOTSUP, "lnz_ada_lanczos_layer: N=%d, K=%d exceed 64", N, K);
  hipStream_t s = (hipStream_t)stream;
  if (N <= 32 && K <= 32) {
    hipLaunchKernelGGL((ada_lanczos_layer_kernel<32, 32>), dim3(B), dim3(64), 0, s, A, mask, q1, N,
                       K, T, Q);
  } else {
    hipLaunchKernelGGL((ada_lanczos_layer_kernel<64, 64>), dim3(B), dim3(64), 0, s, A, mask, q1, N,
                       K, T, Q);
  }
  return lnz::check_launch("lnz_ada_lanczos_layer");
}

extern "C" int lnz_ada_t_powers(const float* T, int B, int K, const int32_t* dist_host, int S,
                                float* Tcat, lnz_stream_t stream) {
  LNZ_REQUIRE(T && dist_host && Tcat && B > 0 && K > 0 && S > 0, LNZ_EINVAL,
              "lnz_ada_t_powers: bad arguments");
  LNZ_REQUIRE(S <= 16 && K <= 64, LNZ_ENOTSUP, "lnz_ada_t_powers: S=%d K=%d out of range", S, K);
  PowArr d;
  int pmax = 0;
  for (int i = 0; i < 16; ++i) {
    d.v[i] = i < S ? dist_host[i] : -1;
    if (i < S && dist_host[i] > pmax) pmax = dist_host[i];
    // every exponent, not only the largest: a slot whose exponent the loop never reaches stays unwritten
    LNZ_REQUIRE(i >= S || (dist_host[i] >= 1 && dist_host[i] <= 4096), LNZ_EINVAL,
                "lnz_ada_t_powers: bad exponents (dist[%d]=%d, 1 .. 4096)", i, i < S ? dist_host[i] : 0);
  }
  size_t lds = (size_t)3 * K * K * sizeof(double);   // 96 KiB at K = 64: beyond 64 KiB from K = 53
  LNZ_DYNAMIC_LDS(ada_t_powers_kernel, lds, "ada_lanczos.hip");
  hipLaunchKernelGGL(ada_t_powers_kernel, dim3(B), dim3(256), lds, (hipStream_t)stream, T, K, d, S,
                     pmax, Tcat);
  return lnz::check_launch("lnz_ada_t_powers");
}

extern "C" int lnz_ada_symmetrize_filters(const float* DD, int B, int K, int S, float* DDp,
                                          lnz_stream_t stream) {
  LNZ_REQUIRE(DD && DDp && B > 0 && K > 0 && S > 0, LNZ_EINVAL,
              "lnz_ada_symmetrize_filters: bad arguments");
  int64_t total = (int64_t)B * S * K * K;
  hipLaunchKernelGGL(ada_symmetrize_kernel, dim3((int)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, DD, total, K, S, DDp);
  return lnz::check_launch("lnz_ada_symmetrize_filters");
}

extern "C" int lnz_split_f16x3(const float* X, int M, int K, int ldx, const float* bias, float alpha,
                               int relu, int Kp, void* out, lnz_stream_t stream) {
  LNZ_REQUIRE(X && out && M > 0 && K > 0 && ldx >= K && Kp >= K && Kp % 4 == 0, LNZ_EINVAL,
              "lnz_split_f16x3: bad arguments (M=%d K=%d ldx=%d Kp=%d)", M, K, ldx, Kp);
  LNZ_REQUIRE(M <= 65535, LNZ_ENOTSUP, "lnz_split_f16x3: M=%d > 65535", M);
  dim3 grid((Kp / 4 + 255) / 256, M);
  hipLaunchKernelGGL(split_f16x3_kernel, grid, dim3(256), 0, (hipStream_t)stream, X, M, K, ldx,
                     bias, alpha, relu, Kp, (_Float16*)out);
  return lnz::check_launch("lnz_split_f16x3");
}
