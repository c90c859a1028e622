// What the kernels for graphs of 33..128 nodes share (csrc/conv_mid.hip: the forward;
// csrc/conv_mid_grad.hip: its backward): the LDS row pitches, the v_mfma_f32_16x16x4_f32 wrapper and
// the bounded spin of the four-workgroup exchange (the protocol itself is described in conv_mid.hip).
#pragma once
#include "common.hpp"

namespace {

constexpr int XP = 132;   // row pitch of the node state (floats)
constexpr int TP = 132;   // row pitch of the transposed buffers: rows = 32 columns / slots, entries = nodes
constexpr int PP = 33;    // row pitch of a wave's long-scale partial block
constexpr int AP = 36;    // row pitch of the summed block

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

constexpr int kSpinLimit = 1 << 24;   // x s_sleep(1) (64 clocks): about half a second

// tid 0 of a workgroup: wait until the low byte of *word reaches 4; returns the word
__device__ __forceinline__ int spin_until_four(const int32_t* word) {
  int v, spins = 0;
  while (((v = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) & 0xff) < 4) {
    __builtin_amdgcn_s_sleep(1);
    if (++spins > kSpinLimit) __builtin_trap();   // a peer workgroup never arrived
  }
  return v;
}

}  // namespace
