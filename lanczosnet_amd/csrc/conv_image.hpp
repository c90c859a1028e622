// The row image the large-graph conv gathers from (csrc/conv_sparse.hip): THE one definition of its
// format, for every kernel that writes one — lnz_large_sparse_image[_channels] (conv_sparse.hip), the
// K-step compaction pass (ell_image.hpp) and the edge-list kernels (edge_image.hip).
//
//   entries [rows][cap] u32 = bf16(value) << 16 | column, entry k of a row in a fixed order;
//   values  [rows][cap] fp32 (optional): the same entries unrounded (the exact-fp32 gather);
//   counts  [rows]; entries (and values) from a row's count up to the next multiple of eight are zero:
//   the gather walks whole groups of eight (cap is a multiple of 8).
#pragma once
#include <hip/hip_runtime.h>

namespace {

typedef __bf16 lnz_bf16x2 __attribute__((ext_vector_type(2)));
typedef float lnz_f32x2 __attribute__((ext_vector_type(2)));

// bf16(value) << 16 | column; round to nearest even (v_cvt_pk_bf16_f32), as conv_large.hip's pack
__device__ inline unsigned conv_entry(float v, int col) {
  const lnz_bf16x2 p = __builtin_convertvector(lnz_f32x2{v, 0.0f}, lnz_bf16x2);
  return ((unsigned)__builtin_bit_cast(unsigned short, p[0]) << 16) | (unsigned)col;
}

// set bits of the ballot m below this lane: the lane's place among the wave's nonzeros
__device__ inline int lane_rank(unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// the whole wave: zero entries (and values, when kept) from the row's count up to the next multiple of eight
__device__ inline void conv_pad_row(unsigned* ent, float* vals, int cnt, int lane) {
  if (cnt + lane < ((cnt + 7) & ~7)) {
    ent[cnt + lane] = 0u;
    if (vals) vals[cnt + lane] = 0.0f;
  }
}

}  // namespace
