// Wavefront primitives of the Lanczos / AdaLanczos / readout kernels: THE one implementation of the
// arithmetic (like conv_tiles.hpp and tridiag_eig.hpp for theirs).  The summation tree below is part
// of every result that is compared bit for bit (sequential vs packed scores, forward vs recomputed
// forward of a backward pass): a kernel that needs a wave sum calls this one.
//
// Not here, on purpose — other summation orders, other bits: lnz_tri::wave_sum_butterfly
// (tridiag_eig.hpp, a __shfl_xor butterfly), xhalf_sum (lanczos_ritz.hip), the __shfl_xor
// reductions of the conv kernels.
#pragma once
#include <hip/hip_runtime.h>

namespace lnz {

constexpr double kEpsF64 = 2.220446049250313e-16;  // 2^-52

// value of lane l (wave-uniform l) of a per-lane double
__device__ __forceinline__ double readlane_f64(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// v of the lane that DPP control CTRL pairs this lane with
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}

// sum over the 16 lanes of a DPP row, the same bits in all 16 (symmetric pairings)
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp<0xB1>(v);    // quad_perm [1,0,3,2]
  v += dpp<0x4E>(v);    // quad_perm [2,3,0,1]
  v += dpp<0x141>(v);   // row_half_mirror
  v += dpp<0x140>(v);   // row_mirror
  return v;
}
__device__ __forceinline__ double row16_sum(double v) {
  v += dpp_f64<0xB1>(v);
  v += dpp_f64<0x4E>(v);
  v += dpp_f64<0x141>(v);
  v += dpp_f64<0x140>(v);
  return v;
}

// sum over the 64 lanes, the same bits in every lane: the four row sums by v_readlane, added in a
// fixed order
__device__ __forceinline__ float wave_sum(float v) {
  v = row16_sum(v);
  const float s0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
  const float s1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
  const float s2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
  const float s3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
  return (s0 + s1) + (s2 + s3);
}
__device__ __forceinline__ double wave_sum(double v) {
  v = row16_sum(v);
  const double s0 = readlane_f64(v, 0), s1 = readlane_f64(v, 16);
  const double s2 = readlane_f64(v, 32), s3 = readlane_f64(v, 48);
  return (s0 + s1) + (s2 + s3);
}

// 1 / x: hardware seed + one Newton step
__device__ __forceinline__ double rcp_nr(double x) {
  double y = __builtin_amdgcn_rcp(x);
  return fma(y, fma(-x, y, 1.0), y);
}

// 1 / sqrt(x) for a normal x > 0: v_rsq_f64's seed (~2^-26) + STEPS Newton steps, each of which
// squares the error — three dependent instructions per step instead of the library rsqrt's scaling
// and special cases
template <int STEPS>
__device__ __forceinline__ double rsq_nr(double x) {
  double y = __builtin_amdgcn_rsq(x);
#pragma unroll
  for (int it = 0; it < STEPS; ++it) {
    const double hy = 0.5 * y;
    const double er = fma(-(x * y), hy, 0.5);
    y = fma(y, er, y);
  }
  return y;
}

// When the second classical Gram-Schmidt pass of a full-length Lanczos step runs (lanczos_ritz.hip,
// lanczos_ritz_wg.hip; tests/algo_mirror.py _cgs2 is the same rule in Python).  One pass against a
// basis whose Gram matrix is I + E leaves Q^T x' = -E c behind, |E c| / |x'| relative to the new
// vector, and c lives on the last two vectors (alpha_j, beta_{j-1}).  The loss of orthogonality e
// therefore obeys  e_new <= g max(e_cur, e_prev) + eps |x| / |x'|,  g = |c| / |x'|,
// |x'|^2 = |x|^2 - |c|^2.  "Second pass where the first removed more than 99 % of |x|^2" alone
// bounds g by 10, not by 1: a spectrum spread evenly over its range has alpha ~ 2 beta, g ~ 2.2 at
// every step, and e grows geometrically — 4e-6 after 32 steps, garbage after 64.
// Graph Laplacians have g < 1 at most steps, which is why the 99 % rule held on them.  The rule
// here keeps the single pass wherever it is safe and cannot compound: the bound is carried along
// (in squares, (a + b)^2 <= 9/8 a^2 + 9 b^2: one reciprocal, no square root; every lane holds the
// same numbers, so the decision is wave uniform) and the second pass also runs once it passes
// kBound2 = (1e-9)^2, a sixtieth of an fp32 ulp of the outputs.  After two passes the new vector
// is orthogonal to g e^2 + eps.  A restart vector's c is spread over ALL basis vectors, each within
// the bound: it always takes both passes.  Molecules stay on the single pass (5 extra second passes
// in 4,000 steps), a spread spectrum takes the second one every sixth step.
// a wave-uniform value, told to the compiler: it lives in a scalar register
__device__ __forceinline__ float wave_uniform(float x) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}
__device__ __forceinline__ double wave_uniform(double x) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)),
                          __builtin_amdgcn_readfirstlane(__double2loint(x)));
}

struct CgsBound {
  static constexpr float kBound2 = 1e-18f;
  static constexpr float kFloor = (float)(9.0 * kEpsF64 * kEpsF64);
  // (floats in scalar registers: a bound needs no more, and the vector registers of the Lanczos
  // step are all taken — three more cost the N <= 32 kernel its third wave per SIMD)
  float cur = 0.0f, prev = 0.0f;  // e^2 of the last two accepted basis vectors
  float cand = 0.0f;              // ... of the vector the last call produced
  // The part of |x|^2 the first pass may remove without a second one: `frac` (the pass is repeated
  // beyond it whatever the bound says), or less where the bound would pass kBound2 —
  // g2 (kFloor + 9/8 emax) + kFloor <= kBound2 with g2 = cc2 / (xx - cc2), solved for cc2 / xx.
  // Known BEFORE the pass: the decision behind it stays one product and one comparison.
  __device__ __forceinline__ float threshold(double frac, bool restart) const {
    const float c1 = fmaf(1.125f, fmaxf(cur, prev), kFloor), room = kBound2 - kFloor;
    return restart ? 0.0f : wave_uniform(fminf((float)frac, room * __builtin_amdgcn_rcpf(c1 + room)));
  }
  // Behind the first pass.  xx = |x|^2, cc2 = sum of the squared coefficients.  -> run the second pass
  __device__ __forceinline__ bool second_pass(double xx, double cc2, float thr, bool restart) {
    const bool again = !(cc2 <= (double)thr * xx);
    // (the bound of the new vector: needed by the next step only)
    const float g2 = xx > 0.0 ? (float)(cc2 * rcp_nr(fmax(xx - cc2, 1e-30 * xx))) : 0.0f;
    const float emax = restart ? kBound2 : fmaxf(cur, prev);
    const float ge = 1.125f * g2 * emax;
    cand = wave_uniform(again ? fmaf(ge, emax, kFloor) : fmaf(kFloor, g2, ge + kFloor));
    return again;
  }
  // the vector is taken into the basis (a candidate that broke down is replaced, not accepted)
  __device__ __forceinline__ void accept() { prev = cur, cur = cand; }
};

// The breakdown tolerance of the full-length Lanczos kernels is relative to the matrix: this power
// of two, 2^ceil(log2 max |a_ij|) (0 for the zero matrix), times 1e-8.  A power of two so that a
// matrix times a power of two takes the same decisions step by step; 1 for every matrix whose
// largest entry lies in (1/2, 1] — the L4 Laplacian of a graph with a leaf or an isolated node.
__device__ __forceinline__ double matrix_scale_pow2(double amax) {
  if (!(amax > 0.0)) return 0.0;
  const double s = __builtin_ldexp(1.0, __builtin_amdgcn_frexp_exp(amax));  // amax = m s, 1/2 <= m < 1
  return 0.5 * s == amax ? amax : s;
}

// entry r of the Lanczos start vector: deterministic, strictly positive, non-symmetric — every
// Lanczos kernel starts from the same vector (lnz_tri::start_entry is another hash: probe vectors)
__device__ __forceinline__ double lanczos_start_entry(unsigned r) {
  const unsigned hsh = (r + 1) * 2654435761u;
  return 1.0 + (double)((hsh >> 8) & 0xffff) * (1.0 / 65536.0);
}

// eigenvalue dj (index jj) comes before di (index i): descending |lambda|, ties by ascending lambda,
// then index = np.argsort(-|eig|, kind='mergesort') on eigh's ascending output
// (utils/data_helper.py:218-223)
__device__ __forceinline__ bool abs_desc_before(double dj, int jj, double di, int i) {
  const double aj = fabs(dj), ai = fabs(di);
  return (aj > ai) || (aj == ai && (dj < di || (dj == di && jj < i)));
}

}  // namespace lnz
