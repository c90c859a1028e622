// What the GGNN kernels share (ggnn.hip: the forward; ggnn_grad.hip: one step of its backward, which
// recomputes the step with the forward's arithmetic): the envelope, the MFMA tile product and sigmoid.
#pragma once
#include "common.hpp"

namespace {

constexpr int GHID = 128;      // message hidden width (model/ggnn.py:59-61)
constexpr int GNW = 8;         // waves per workgroup
constexpr int GNT = 64 * GNW;  // threads
constexpr int GMAXN = 32, GMAXC = 8, GMAXP = 16, GMAXD = 128;
constexpr int HS = GHID + 4;   // row stride of H_c (floats): 16-byte rows, fragment reads spread over the banks

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// acc[t][rt] += (16 RT rows of the LDS operand, K = 16 KB columns) x (16 weight rows of tile t)^T.
// `as` = the operand's row (lane & 15) + 4 (lane >> 4) floats; wp[t] = the weight row of this lane
// + 4 (lane >> 4) floats.  Lane (m, g) multiplies k = 16 kb + 4 g + u in MFMA step u on both operands;
// register e of acc[t][rt] is row 16 rt + m, feature (tile base) + 4 g + e.  The weight fragments are
// loaded PF blocks ahead of the MFMAs that use them.
template <int NT, int KB, int RT>
__device__ __forceinline__ void tile_gemm(const float* as, const int lda, const float* const (&wp)[NT],
                                          f32x4 (*acc)[RT]) {
  constexpr int PF0 = NT >= 3 ? 2 : 4, PF = KB < PF0 ? KB : PF0;
  f32x4 w[KB][NT];
#pragma unroll
  for (int kb = 0; kb < PF; ++kb)
#pragma unroll
    for (int t = 0; t < NT; ++t) w[kb][t] = *reinterpret_cast<const f32x4*>(wp[t] + 16 * kb);
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    f32x4 a[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) a[rt] = *reinterpret_cast<const f32x4*>(as + 16 * rt * lda + 16 * kb);
    if (kb + PF < KB) {
#pragma unroll
      for (int t = 0; t < NT; ++t) w[kb + PF][t] = *reinterpret_cast<const f32x4*>(wp[t] + 16 * (kb + PF));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[t][rt] = mfma16(w[kb][t][u], a[rt][u], acc[t][rt]);
  }
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
inline bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace
