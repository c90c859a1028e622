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
